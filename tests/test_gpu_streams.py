"""Every device entry point on a caller's stream that runs late (harness and reasoning: tests/_late_stream.py).

The stand-alone entry points get S as their hip_stream argument; handles get it through cip_set_stream, each in two orders:
handle A makes the plain (null-stream) run first, has its internal state overwritten by a run on other inputs, moves to S and makes
the late run; handle B is fresh and makes the late run as its very first use, so that whatever it creates lazily -- buffers, side
streams, graphs -- is born under S.  Both must give A's plain bits.  Calls the header documents as not waiting for the GPU are
followed by an assertion that S is still inside its spin: the speculative branch of the pivot-flag logic then runs by
construction.  STREAM_TABLE names the test that covers each entry point; tests/test_stream_table.py keeps it complete."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _late_stream as LS
import problems as P

pytestmark = pytest.mark.gpu

F64 = LS.F64
dev = LS.dev

# entry point -> the tests below that run it with S late
STREAM_TABLE = {
    "cip_gemm_nt_dev": ["test_gemm_nt_on_a_late_stream"],
    "cip_ldlt_factor_dev": ["test_standalone_ldlt_on_a_late_stream", "test_standalone_bad_pivot_is_reported_with_the_stream_late"],
    "cip_ldlt_solve_dev": ["test_standalone_ldlt_on_a_late_stream"],
    "cip_ldlt_solve_many_dev": ["test_standalone_ldlt_on_a_late_stream"],
    "cip_qrcp_dev": ["test_qrcp_and_imcols_on_a_late_stream"],
    "cip_imcols_dev": ["test_qrcp_and_imcols_on_a_late_stream"],
    "cip_set_stream": ["test_mixed_handle_on_a_late_stream"],
    "cip_set_scaling_identity": ["test_mixed_handle_on_a_late_stream"],
    "cip_set_scaling_from_iterate_dev": ["test_mixed_handle_on_a_late_stream", "test_large_s_cone_on_a_late_stream"],
    "cip_factor": ["test_mixed_handle_on_a_late_stream", "test_order_4096_side_prep_on_a_late_stream"],
    "cip_check_factor": ["test_host_pointer_calls_are_valid_on_return", "test_mixed_handle_on_a_late_stream"],
    "cip_solve3x3_dev": ["test_mixed_handle_on_a_late_stream", "test_first_solve_resolves_the_pivot_flag_with_the_stream_late"],
    "cip_solve2x2_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_solve3x3_many_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_solve2x2_many_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_solve4x4_dev": ["test_mixed_handle_on_a_late_stream", "test_all_r_csr_handle_on_a_late_stream"],
    "cip_apply_F_dev": ["test_mixed_handle_on_a_late_stream", "test_large_s_cone_on_a_late_stream"],
    "cip_cone_prod_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_cone_div_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_cone_identity_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_maxstep_dev": ["test_mixed_handle_on_a_late_stream", "test_host_scratch_is_not_mixed_up_between_two_handles"],
    "cip_maxstep_pair_dev": ["test_mixed_handle_on_a_late_stream", "test_large_s_cone_on_a_late_stream"],
    "cip_gemv_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_dots_dev": ["test_mixed_handle_on_a_late_stream", "test_host_scratch_is_not_mixed_up_between_two_handles"],
    "cip_axpby_dev": ["test_mixed_handle_on_a_late_stream"],
    "cip_solve3x3": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_solve2x2": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_solve3x3_many": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_solve2x2_many": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_set_scaling_packed": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_get_scaling_packed": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_get_kkt_matrix": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_assemble_only": ["test_host_pointer_calls_are_valid_on_return"],
    "cip_update_problem": ["test_update_problem_on_a_late_stream"],
    "cip_conicip": ["test_conicip_on_a_late_stream", "test_graph_replay_on_a_late_stream"],
}


@pytest.fixture(scope="module")
def lib():
    import cipkkt
    return cipkkt._lib.load()


def _check(rc):
    from cipkkt import _lib as L
    L.check(rc)


# ============================================================================================ the harness can fail
def _double_seq(consumer_stream):
    """y = 2 x as a plain torch op; consumer_stream(r) -> the stream the op is issued on in the late run"""
    def seq(r):
        r.stage(inputs=["x"], outputs=["y"])
        if r.late:
            with torch.cuda.stream(consumer_stream(r)):
                torch.mul(r["x"], 2.0, out=r["y"])
        else:
            torch.mul(r["x"], 2.0, out=r["y"])
        return {}
    return seq


def _self_check(consumer_stream, label):
    real = {"x": dev(np.arange(1.0, 4097.0))}
    plain = LS.run_plain(_double_seq(None), real, {"y": 4096}, ["x", "y"])
    got = LS.run_late(_double_seq(consumer_stream), real, {"y": 4096}, ["x", "y"], plain[2], label)
    return LS.differences(plain[:2], got)


def test_self_check_a_consumer_on_the_stream_passes():
    assert _self_check(lambda r: r.S, "self-check: consumer on S") == []


def test_self_check_a_consumer_on_the_null_stream_is_caught():
    assert _self_check(lambda r: torch.cuda.default_stream(), "self-check: consumer on the null stream") == ["y"]


def test_self_check_a_consumer_on_another_stream_is_recorded():
    """With four hardware queues two streams may share one, and a shared queue serialises them behind the spin: recorded only."""
    other = torch.cuda.Stream()
    bad = _self_check(lambda r: other, "self-check: consumer on a second stream")
    other.synchronize()
    print("LATE | a consumer on a second fresh stream was %s" % ("caught" if bad else "NOT caught (the two streams shared a queue)"))


def test_self_check_the_stream_is_busy_behind_the_spin():
    S = LS.stream()
    x = dev(np.ones(1024))
    y = torch.full_like(x, LS.NAN)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(LS.SPIN_MIN_MS * LS.cycles_per_ms()))
        y.copy_(x, non_blocking=True)
    busy = not S.query()
    S.synchronize()
    assert busy and S.query() and torch.equal(x, y)
    print("LATE | calibration: %.0f ticks of torch.cuda._sleep per millisecond" % LS.cycles_per_ms())


# ============================================================================================ stand-alone entry points
@pytest.mark.parametrize("M,N,K,lower", [(256, 128, 32, 0), (384, 384, 16, 1)])
def test_gemm_nt_on_a_late_stream(lib, M, N, K, lower):
    rng = np.random.default_rng(M + K)
    real = {"A": dev(rng.standard_normal((K, M))), "B": dev(rng.standard_normal((K, N))), "C": dev(rng.standard_normal((N, M)))}

    def seq(r):
        r.stage(inputs=["A", "B", "C"])
        _check(lib.cip_gemm_nt_dev(r.ptr, M, N, K, -0.75, r["A"].data_ptr(), M, r["B"].data_ptr(), N, r["C"].data_ptr(), M, lower))
        r.still_busy("cip_gemm_nt_dev")
        return {}

    (want, _), _ = LS.compare(seq, real, {}, ["A", "B", "C"], "cip_gemm_nt_dev %dx%dx%d lower=%d" % (M, N, K, lower))
    assert torch.isfinite(want["C"]).all() and not torch.equal(want["C"], real["C"])


def _ldlt_buffers(lib, N, nrhs_list):
    nb = C.c_size_t()
    _check(lib.cip_ldlt_workspace_bytes(N, C.byref(nb)))
    ws = torch.zeros(nb.value // 8 + 8, **F64)
    scratch = {}
    for k in nrhs_list:
        _check(lib.cip_ldlt_solve_many_scratch_bytes(N, k, C.byref(nb)))
        scratch[k] = torch.zeros(max(nb.value // 8, 1), **F64)
    torch.cuda.synchronize()
    return ws, scratch


LDLT_CASES = {"n384_three_launch_chain": (384, 0, 0), "n384_fused_chain": (384, 3, 0), "n1024_two_outer_blocks": (1024, -1, 512)}


@pytest.mark.parametrize("name", list(LDLT_CASES))
def test_standalone_ldlt_on_a_late_stream(lib, name):
    """factor (waits: *info_host is right on return), then the three solves, which do not wait"""
    from test_gpu_ldlt_hard import _with_bad_pivot, knobs
    N, chain, nbo = LDLT_CASES[name]
    rng = np.random.default_rng(N + chain)
    K = _with_bad_pivot(N, [(N // 2 + 1, 2.0)], rng)                      # (a clean matrix of that construction)
    ldb = N + 24
    real = {"K": dev(K), "b": dev(rng.standard_normal(N)), "B3": dev(rng.standard_normal((3, ldb))), "B65": dev(rng.standard_normal((65, ldb)))}

    def seq(r):
        ws, scratch = _ldlt_buffers(lib, N, (3, 65))                       # workspaces: fresh per run, never poisoned
        info = C.c_int(-1)
        r.stage(inputs=["K"])
        _check(lib.cip_ldlt_factor_dev(r.ptr, r["K"].data_ptr(), N, N, ws.data_ptr(), C.byref(info)))
        r.stage(inputs=["b", "B3", "B65"])
        _check(lib.cip_ldlt_solve_dev(r.ptr, r["K"].data_ptr(), N, N, ws.data_ptr(), r["b"].data_ptr()))
        for k in (3, 65):
            _check(lib.cip_ldlt_solve_many_dev(r.ptr, r["K"].data_ptr(), N, N, ws.data_ptr(), scratch[k].data_ptr(),
                                               r["B%d" % k].data_ptr(), ldb, k))
        r.still_busy("cip_ldlt_solve_dev / cip_ldlt_solve_many_dev")
        r.keep = (ws, scratch)
        return {"info": info.value}

    def lower(out):                                                        # the upper triangle of the diagonal blocks is undefined
        dv, host = out
        return dict(dv, K=torch.triu(dv["K"])), host

    with knobs(lib, chain=chain, nbo=nbo):
        dv, host, ms = LS.run_plain(seq, real, {}, list(real))
        got = LS.run_late(seq, real, {}, list(real), ms, "stand-alone LDL' " + name)
    assert host["info"] == 0 and torch.isfinite(dv["b"]).all() and torch.isfinite(dv["B65"][:, :N]).all()
    LS.assert_same_bits(lower((dv, host)), lower(got), name)


@pytest.mark.parametrize("N,nbo,col", [(384, 0, 129), (1024, 512, 512)])
def test_standalone_bad_pivot_is_reported_with_the_stream_late(lib, N, nbo, col):
    from test_gpu_ldlt_hard import _with_bad_pivot, knobs
    K = _with_bad_pivot(N, [(col, 0.0)], np.random.default_rng(col))
    real = {"K": dev(K)}

    def seq(r):
        ws, _ = _ldlt_buffers(lib, N, ())
        info = C.c_int(-1)
        r.stage(inputs=["K"])
        rc = lib.cip_ldlt_factor_dev(r.ptr, r["K"].data_ptr(), N, N, ws.data_ptr(), C.byref(info))
        r.keep = ws
        return {"rc": rc, "info": info.value}

    with knobs(lib, nbo=nbo):
        _, host, ms = LS.run_plain(seq, real, {}, [])
        _, late = LS.run_late(seq, real, {}, [], ms, "bad pivot at column %d of %d" % (col, N))
    assert host == {"rc": 0, "info": col + 1} and late == host, (host, late)


@pytest.mark.parametrize("shape", [(65, 63, 40), (300, 257, 257)], ids=lambda s: "%dx%d_r%d" % s)
def test_qrcp_and_imcols_on_a_late_stream(lib, shape):
    """both calls wait for their result: piv, rdiag, k and rows, nrows, consistent, resid are compared as returned"""
    from cipkkt import _lib as L
    from test_gpu_qrcp import lowrank
    ln, cnt, _ = shape
    M0 = lowrank(*shape)
    kmax = min(ln, cnt)
    A = np.ascontiguousarray(M0.T)                                          # cnt rows of length len
    real = {"M": dev(A), "Mi": dev(A), "bi": dev(A @ np.random.default_rng(ln).standard_normal(ln))}
    nq, ni = C.c_size_t(), C.c_size_t()
    assert lib.cip_qrcp_workspace_bytes(ln, cnt, C.byref(nq)) == 0 and lib.cip_imcols_workspace_bytes(ln, cnt, C.byref(ni)) == 0

    def seq(r):
        wq = torch.zeros(nq.value, dtype=torch.uint8, device="cuda")
        wi = torch.zeros(ni.value, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        piv, rdiag, k = np.full(cnt, -1, dtype=np.int32), np.zeros(kmax), C.c_int(-1)
        r.stage(inputs=["M"], outputs=["tau"])
        _check(lib.cip_qrcp_dev(r.ptr, r["M"].data_ptr(), ln, cnt, ln, 0.0, wq.data_ptr(), r["tau"].data_ptr(),
                                piv.ctypes.data_as(L.c_int_p), rdiag.ctypes.data_as(L.c_double_p), C.byref(k)))
        host = {"piv": piv.copy(), "rdiag": rdiag.copy(), "k": k.value}
        rows, nrows, ok, resid = np.full(cnt, -1, dtype=np.int32), C.c_int(-1), C.c_int(-1), C.c_double(-1.0)
        r.stage(inputs=["Mi", "bi"])
        _check(lib.cip_imcols_dev(r.ptr, r["Mi"].data_ptr(), ln, cnt, ln, r["bi"].data_ptr(), 1e-8, wi.data_ptr(),
                                  rows.ctypes.data_as(L.c_int_p), C.byref(nrows), C.byref(ok), C.byref(resid)))
        host.update(rows=rows.copy(), nrows=nrows.value, consistent=ok.value, resid=resid.value)
        r.keep = (wq, wi)
        return host

    (dv, host), _ = LS.compare(seq, real, {"tau": kmax}, ["M", "tau", "Mi", "bi"], "cip_qrcp_dev / cip_imcols_dev %dx%d" % (ln, cnt))
    assert host["k"] == kmax and sorted(host["piv"]) == list(range(cnt))
    assert host["consistent"] == 1 and host["nrows"] == np.linalg.matrix_rank(A)
    assert torch.equal(dv["Mi"], real["Mi"]) and torch.equal(dv["bi"], real["bi"])


# ============================================================================================ handles
def _interior(cone_dims, rng):
    from oracle.cones import vecm
    xs = []
    for t, k in cone_dims:
        if t == "R":
            xs.append(rng.random(k) + 0.1)
        elif t == "Q":
            x = rng.standard_normal(k)
            x[0] = np.linalg.norm(x[1:]) + 0.5
            xs.append(x)
        else:
            r_ = int(round((np.sqrt(1 + 8 * k) - 1) / 2))
            G = rng.standard_normal((r_, r_))
            xs.append(vecm(G @ G.T / r_ + 0.5 * np.eye(r_)))
    return np.concatenate(xs)


def _handle_ab(make, seq, real, outs, label, scramble=None, history=False):
    """handle A: plain run, scramble, cip_set_stream(S), late run; handle B: fresh, late run as its very first use.  seq(ks, r, warm).
    history=True, for handles whose results depend on their past by design (large S cones: the Jacobi of the NT scaling is
    warm-started from the previous scaling's singular vectors): A's late run follows scramble alone, and is compared with a
    null-stream run on a third handle with that same past; B is compared with the fresh handle's plain run as always."""
    S = LS.stream()
    names = list(real) + list(outs)
    A = make()
    try:
        dv, host, ms = LS.run_plain(lambda r: seq(A, r, False), real, outs, names)
        want = (dv, host)
        if history:
            A.close()
            P1, A = make(), make()
            try:
                for ks in (P1, A):
                    scramble(ks)
                torch.cuda.synchronize()
                want = LS.run_plain(lambda r: seq(P1, r, True), real, outs, names)[:2]
            finally:
                P1.close()
        elif scramble is not None:
            scramble(A)                                   # the handle's internal state no longer matches the plain run's
            torch.cuda.synchronize()
        A.set_stream(S.cuda_stream)
        got = LS.run_late(lambda r: seq(A, r, True), real, outs, names, ms, label + " (handle A)")
        LS.assert_same_bits(want, got, label + " (handle A)")
        A.check_factor()
    finally:
        A.close()
    B = make()
    try:
        B.set_stream(S.cuda_stream)
        got = LS.run_late(lambda r: seq(B, r, False), real, outs, names, ms, label + " (handle B)")
        LS.assert_same_bits((dv, host), got, label + " (handle B)")
        B.check_factor()
    finally:
        B.close()
    return dv, host


MIXED_CONES = [("R", 30), ("Q", 6), ("S", 6), ("Q", 9), ("R", 7), ("S", 10)]
MIXED_N, MIXED_P = 60, 4


def _mixed_problem():
    rng = np.random.default_rng(11)
    n, p = MIXED_N, MIXED_P
    m = sum(k for _, k in MIXED_CONES)
    Mq = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.3)
    Q = Mq.T @ Mq / n + 0.1 * np.eye(n)
    A = rng.standard_normal((m, n)) * 0.3 * (rng.random((m, n)) < 0.5)
    G = rng.standard_normal((p, n))
    return Q, A, G, n, m, p


def _mixed_real(rng, n, m, p):
    rn = rng.standard_normal
    real = {"x": rn(n), "y": rn(p), "z": rn(m), "v": _interior(MIXED_CONES, rng), "s": _interior(MIXED_CONES, rng),
            "X3": rn((3, n)), "Y3": rn((3, p)), "Z3": rn((3, m)), "r4": rn(n + p + 2 * m),
            "u1": _interior(MIXED_CONES, rng), "u2": _interior(MIXED_CONES, rng),
            "gn": rn(n), "gm": rn(m), "gp": rn(p), "yQ": rn(n), "yQt": rn(n), "yA": rn(m), "yAt": rn(n), "yG": rn(p), "yGt": rn(n),
            "ax": rn(m), "ay": rn(m), "w1": _interior(MIXED_CONES, rng), "d1": rn(m), "w2": _interior(MIXED_CONES, rng), "d2": rn(m),
            "dx": rn(n), "dy": rn(n)}
    for mode in range(4):
        real["f%di" % mode] = real["u1"].copy()
    outs = {"a0": n, "b0": p, "c0": m, "lam": m, "a": n, "b": p, "c": m, "dy2": n, "dw2": p, "A3": (3, n), "B3": (3, p), "C3": (3, m),
            "DY3": (3, n), "DW3": (3, p), "dz": n + p + 2 * m, "f0": m, "f1": m, "f2": m, "f3": m, "prod": m, "div": m, "e": m}
    return {k: dev(t) for k, t in real.items()}, outs


def _mixed_seq(ks, r, warm):
    from cipkkt import _lib as L
    schur = ks.route == L.ROUTE_SCHUR
    host = {}
    r.stage(inputs=["x", "y", "z"], outputs=["a0", "b0", "c0"])
    ks.set_scaling_identity()
    ks.factor(check=False)
    if warm:
        r.still_busy("cip_set_scaling_identity / cip_factor")
    ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a0"], r["b0"], r["c0"])    # (a handle's first *_dev solve waits by contract)
    if warm:
        r.still_busy("cip_solve3x3_dev after a factorisation was seen clean")
    r.stage(inputs=["v", "s", "X3", "Y3", "Z3", "r4"],
            outputs=["lam", "a", "b", "c", "dy2", "dw2", "A3", "B3", "C3", "DY3", "DW3", "dz"])
    ks.set_scaling_from_iterate(r["v"], r["s"], r["lam"])
    ks.factor(check=False)
    ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a"], r["b"], r["c"])
    if schur:
        ks.solve2x2_dev(r["x"], r["y"], r["dy2"], r["dw2"])
        ks.solve2x2_many_dev(r["X3"], r["Y3"], r["DY3"], r["DW3"])
    ks.solve3x3_many_dev(r["X3"], r["Y3"], r["Z3"], r["A3"], r["B3"], r["C3"])
    ks.solve4x4_dev(r["lam"], r["r4"], r["dz"])
    r.still_busy("the scaling setter, cip_factor or a *_dev solve (speculative: the flag cannot have landed)")
    r.stage(inputs=["u1", "u2", "f0i", "f1i", "f2i", "f3i", "gn", "gm", "gp", "yQ", "yQt", "yA", "yAt", "yG", "yGt", "ax", "ay"],
            outputs=["f0", "f1", "f2", "f3", "prod", "div", "e"])
    for mode in range(4):
        ks.apply_F(mode, r["u1"], r["f%d" % mode])
        ks.apply_F(mode, r["f%di" % mode], r["f%di" % mode])              # in place
    ks.cone_prod(r["u1"], r["u2"], r["prod"])
    ks.cone_div(r["u1"], r["u2"], r["div"])
    ks.cone_identity(r["e"])
    ks.gemv(L.MAT_Q, 0, 1.5, r["gn"], 0.5, r["yQ"])
    ks.gemv(L.MAT_Q, 1, 1.5, r["gn"], -0.5, r["yQt"])
    ks.gemv(L.MAT_A, 0, -0.75, r["gn"], 2.0, r["yA"])
    ks.gemv(L.MAT_A, 1, 1.25, r["gm"], 0.5, r["yAt"])
    ks.gemv(L.MAT_G, 0, 1.5, r["gn"], 0.25, r["yG"])
    ks.gemv(L.MAT_G, 1, -1.5, r["gp"], 1.0, r["yGt"])
    ks.axpby(0.75, r["ax"], -1.25, r["ay"])
    r.still_busy("cip_apply_F_dev, a cone operation, cip_gemv_dev or cip_axpby_dev")
    r.stage(inputs=["w1", "d1"])
    host["maxstep"] = ks.maxstep(r["w1"], r["d1"], 0.7)
    r.stage(inputs=["d2"])
    host["maxstep_nothing"] = ks.maxstep(r["d2"])
    r.stage(inputs=["w2"])
    host["maxstep_pair"] = ks.maxstep_pair(r["w1"], r["d1"], r["w2"], r["d2"], 0.9)
    r.stage(inputs=["dx", "dy"])
    host["dots"] = ks.dots([(r["dx"], r["dy"]), (r["dx"], r["dx"]), (r["dy"][:7], r["dx"][:7])])
    return host


def _mixed_make(route, a_csr, q_csr):
    import cipkkt
    Q, A, G, n, m, p = _mixed_problem()
    return lambda: cipkkt.KKTSystem(Q, sp.csr_matrix(A) if a_csr else A, G, MIXED_CONES, route=route, sparse_q=q_csr)


def _mixed_scramble(n, m):
    rng = np.random.default_rng(5)
    v, s = dev(_interior(MIXED_CONES, rng)), dev(_interior(MIXED_CONES, rng))

    def scramble(ks):
        ks.set_scaling_from_iterate(v, s)
        ks.factor()
    return scramble


@pytest.mark.parametrize("q_csr", [False, True], ids=["denseQ", "csrQ"])
@pytest.mark.parametrize("a_csr", [False, True], ids=["denseA", "csrA"])
@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_mixed_handle_on_a_late_stream(route, a_csr, q_csr):
    Q, A, G, n, m, p = _mixed_problem()
    real, outs = _mixed_real(np.random.default_rng(3), n, m, p)
    dv, host = _handle_ab(_mixed_make(route, a_csr, q_csr), _mixed_seq, real, outs, "mixed R/Q/S handle %s %s %s" % (
        route, "csrA" if a_csr else "denseA", "csrQ" if q_csr else "denseQ"), scramble=_mixed_scramble(n, m))
    skip = ("dy2", "dw2", "DY3", "DW3") if route == "full3x3" else ()
    for k in outs:
        assert k in skip or torch.isfinite(dv[k]).all(), k
    assert all(np.isfinite(host["dots"])) and host["maxstep"] > 0


def test_all_r_csr_handle_on_a_late_stream():
    """n = 1024, A = I in CSR, one R cone: the fused solve4x4 and the lazy copy of Q into K"""
    import cipkkt
    from cipkkt import workloads as W
    n = 1024
    Q, c, A, b, K = W.c2_problem(n, seed=5, device="cuda")
    rng = np.random.default_rng(8)
    real = {k: dev(t) for k, t in dict(v=rng.random(n) + 0.05, s=rng.random(n) + 0.05, r4=rng.standard_normal(3 * n),
                                       v2=rng.random(n) + 0.05, s2=rng.random(n) + 0.05).items()}
    outs = {"lam": n, "dz": 3 * n, "lam2": n, "dz2": 3 * n}

    def seq(ks, r, warm):
        r.stage(inputs=["v", "s", "r4"], outputs=["lam", "dz"])
        ks.set_scaling_from_iterate(r["v"], r["s"], r["lam"])
        ks.factor(check=False)
        ks.solve4x4_dev(r["lam"], r["r4"], r["dz"])
        if warm:
            r.still_busy("cip_factor / cip_solve4x4_dev")
        r.stage(inputs=["v2", "s2"], outputs=["lam2", "dz2"])
        ks.set_scaling_from_iterate(r["v2"], r["s2"], r["lam2"])
        ks.factor(check=False)
        ks.solve4x4_dev(r["lam2"], r["r4"], r["dz2"])
        r.still_busy("cip_factor / cip_solve4x4_dev")
        return {}

    def scramble(ks):
        ks.set_scaling_from_iterate(real["s"], real["v2"])
        ks.factor()

    dv, _ = _handle_ab(lambda: cipkkt.KKTSystem(Q, A, None, K), seq, real, outs, "all-R CSR handle n = 1024", scramble)
    assert torch.isfinite(dv["dz"]).all() and torch.isfinite(dv["dz2"]).all() and not torch.equal(dv["dz"], dv["dz2"])


def test_order_4096_side_prep_on_a_late_stream():
    """the smallest order at which the solve preparation forks to the handle's side stream: factor, solve, factor, solve"""
    import cipkkt
    import _ldlt_ref as R
    from cipkkt import workloads as W
    n = 4096
    assert R.side_prep_forks(n)
    Q, c, A, b, K = W.c2_problem(n, seed=77, device="cuda")
    rng = np.random.default_rng(9)
    real = {k: dev(t) for k, t in dict(v=rng.random(n) + 0.1, s=rng.random(n) + 0.1, v2=rng.random(n) + 0.1, s2=rng.random(n) + 0.1,
                                       x=rng.standard_normal(n), z=rng.standard_normal(n)).items()}
    outs = {"a": n, "c": n, "a2": n, "c2": n}

    def seq(ks, r, warm):
        r.stage(inputs=["v", "s", "x", "z"], outputs=["a", "c"])
        ks.set_scaling_from_iterate(r["v"], r["s"])
        ks.factor(check=False)
        ks.solve3x3_dev(r["x"], None, r["z"], r["a"], None, r["c"])
        if warm:
            r.still_busy("cip_factor / cip_solve3x3_dev")
        r.stage(inputs=["v2", "s2"], outputs=["a2", "c2"])
        ks.set_scaling_from_iterate(r["v2"], r["s2"])
        ks.factor(check=False)                                            # (overwrites K: the side stream must have been joined)
        ks.solve3x3_dev(r["x"], None, r["z"], r["a2"], None, r["c2"])
        r.still_busy("cip_factor / cip_solve3x3_dev")
        return {}

    def scramble(ks):
        ks.set_scaling_from_iterate(real["s2"], real["v"])
        ks.factor()

    dv, _ = _handle_ab(lambda: cipkkt.KKTSystem(Q, A, None, K), seq, real, outs, "Schur handle of order 4096", scramble)
    assert torch.isfinite(dv["a"]).all() and torch.isfinite(dv["c2"]).all()


@pytest.mark.parametrize("r_", [133, 300])
def test_large_s_cone_on_a_late_stream(r_):
    """one S cone of order 133 (maxstep_pair on its two streams) / 300 (the chip-wide kernels).  The scaling of a large S cone depends
    on the handle's previous scaling (warm start of the Jacobi), so handle A is compared with a handle of the same past."""
    import cipkkt
    k, n = r_ * (r_ + 1) // 2, 4
    cones = [("S", k)]
    rng = np.random.default_rng(r_)
    A = rng.standard_normal((k, n)) * 0.1
    real = {key: dev(t) for key, t in dict(v=_interior(cones, rng), s=_interior(cones, rng), x=rng.standard_normal(n),
                                           z=rng.standard_normal(k), w1=_interior(cones, rng), d1=rng.standard_normal(k),
                                           w2=_interior(cones, rng), d2=rng.standard_normal(k)).items()}
    outs = {"lam": k, "a": n, "c": k, "f": k, "prod": k}

    def seq(ks, r, warm):
        r.stage(inputs=["v", "s", "x", "z"], outputs=["lam", "a", "c", "f", "prod"])
        ks.set_scaling_from_iterate(r["v"], r["s"], r["lam"])
        ks.factor(check=False)
        ks.solve3x3_dev(r["x"], None, r["z"], r["a"], None, r["c"])
        ks.apply_F(1, r["z"], r["f"])
        ks.cone_prod(r["v"], r["s"], r["prod"])
        r.stage(inputs=["w1", "d1", "w2", "d2"])
        return {"maxstep_pair": ks.maxstep_pair(r["w1"], r["d1"], r["w2"], r["d2"], 0.9)}

    def scramble(ks):
        ks.set_scaling_from_iterate(real["w1"], real["w2"])
        ks.factor()

    dv, host = _handle_ab(lambda: cipkkt.KKTSystem(np.eye(n), A, None, cones), seq, real, outs, "S cone of order %d" % r_, scramble,
                          history=True)
    assert torch.isfinite(dv["c"]).all() and all(np.isfinite(host["maxstep_pair"]))


def test_first_solve_resolves_the_pivot_flag_with_the_stream_late():
    """the LP of test_gpu_panel_chain.py::test_first_solve_after_factor_waits_for_the_pivot_flag: with S late the first *_dev solve
    must still resolve the flag, the handle switches to the regularised factor, and the refined solve (a host loop over the
    residual and cip_dots) gives the plain run's bits"""
    import cipkkt
    rng = np.random.default_rng(2)
    n, m, p = 40, 24, 16
    Q, A, G = np.zeros((n, n)), rng.standard_normal((m, n)), rng.standard_normal((p, n))
    real = {k: dev(rng.standard_normal(d)) for k, d in (("x", n), ("y", p), ("z", m))}
    outs = {"a": n, "b": p, "c": m}
    handles = []

    def seq(r):
        ks = cipkkt.KKTSystem(Q, A, G, [("R", m)])
        handles.append(ks)
        if r.late:
            ks.set_stream(r.S.cuda_stream)
        r.stage(inputs=["x", "y", "z"], outputs=["a", "b", "c"])
        ks.set_scaling_identity()
        ks.factor(check=False)
        try:
            ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a"], r["b"], r["c"])
        except cipkkt.CipError as e:                                      # "repeat them": now on the regularised factor
            assert e.code == cipkkt._lib.E_RETRY, str(e)
            ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a"], r["b"], r["c"])
        h = ks.health()
        return {"switched": h["n_regularized"], "rel": h["reg_rel"]}

    try:
        (dv, host), _ = LS.compare(seq, real, outs, list(outs), "LP whose first factorisation meets a zero pivot")
        assert host["switched"] == 1 and host["rel"] > 0 and torch.isfinite(dv["a"]).all()
    finally:
        for ks in handles:
            ks.close()


def test_speculative_solves_come_back_as_retry():
    """One handle whose bad pivot appears only at a later factorisation (the family of test_gpu_lockstep_regularized.py::
    test_group_switched_at_a_later_factorisation: a definite QP and the wrong-sign kind of cip_debug_chain_giveup).  The handle has
    seen a clean factorisation, so the solve enqueued behind the spin goes ahead speculatively; the resolving call reports
    CIP_E_RETRY, and the repeated solve gives the plain run's bits (there the flag is resolved before the solve)."""
    import cipkkt
    from cipkkt import _lib as L
    from test_gpu_lockstep_regularized import _definite_qp
    lib = L.load()
    pr = _definite_qp(12, np.random.default_rng(71))
    n, m, p = 12, 12, 2
    rng = np.random.default_rng(4)
    real = {k: dev(t) for k, t in dict(x=rng.standard_normal(n), y=rng.standard_normal(p), z=rng.standard_normal(m),
                                       v=rng.random(m) + 0.1, s=rng.random(m) + 0.1).items()}
    outs = {"a": n, "b": p, "c": m}
    handles = []

    def seq(r):
        ks = cipkkt.KKTSystem(pr["Q"], pr["A"], pr["G"], pr["cone_dims"])
        handles.append(ks)
        ks.set_scaling_identity()
        ks.factor()                                                       # seen clean: later *_dev solves do not wait
        if r.late:
            ks.set_stream(r.S.cuda_stream)
        lib.cip_debug_chain_giveup(1 | (1 << 28))                         # the next factorisation reports a wrong-sign pivot
        r.stage(inputs=["x", "y", "z", "v", "s"], outputs=["a", "b", "c"])
        ks.set_scaling_from_iterate(r["v"], r["s"])
        ks.factor(check=False)
        codes = []
        if r.late:
            ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a"], r["b"], r["c"])
            r.still_busy("the speculative cip_solve3x3_dev")
        codes.append(lib.cip_check_factor(ks.h))
        ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a"], r["b"], r["c"])
        return {"codes": codes, "switched": ks.health()["n_regularized"], "hook_left": lib.cip_debug_chain_giveup(-1)}

    try:
        dv, host, ms = LS.run_plain(seq, real, outs, list(outs))
        got = LS.run_late(seq, real, outs, list(outs), ms, "bad pivot at a later factorisation")
    finally:
        lib.cip_debug_chain_giveup(0)
        for ks in handles:
            ks.close()
    assert host == {"codes": [0], "switched": 1, "hook_left": 0}, host
    assert got[1] == {"codes": [L.E_RETRY], "switched": 1, "hook_left": 0}, got[1]
    LS.assert_same_bits((dv, None), got, "the repeated solve")


# ============================================================================================ host pointers, waiting calls
def _host_seq(ks, r, warm):
    from cipkkt import _lib as L
    schur = ks.route == L.ROUTE_SCHUR
    hx, hy, hz = (r.real[k].cpu().numpy() for k in ("x", "y", "z"))
    X3, Y3, Z3 = (r.real[k].cpu().numpy().T for k in ("X3", "Y3", "Z3"))
    host = {}

    def scaling(v, s, factor=True):
        r.stage(inputs=[v, s])
        ks.set_scaling_from_iterate(r[v], r[s])
        if factor:
            ks.factor(check=False)

    scaling("v", "s")
    host["solve3x3"] = ks.solve3x3(hx, hy, hz)
    scaling("v2", "s2")
    host["solve2x2"] = ks.solve2x2(hx, hy) if schur else ks.solve3x3(hx, hy, hz)
    scaling("v", "s")
    host["solve3x3_many"] = ks.solve3x3_many(X3, Y3, Z3)
    scaling("v2", "s2")
    host["solve2x2_many"] = ks.solve2x2_many(X3, Y3) if schur else ks.solve3x3(hx, hy, hz)    # (a call that waits, either way)
    scaling("v", "s")                                                     # (K holds the factor for v2, s2 until this one has run)
    host["kkt_factored"] = np.tril(ks.kkt_matrix())
    scaling("v2", "s2", factor=False)
    host["packed"] = ks.get_scaling_packed()
    scaling("v", "s", factor=False)                                       # the upload below must land BEHIND this scaling
    buf = host["packed"].copy()
    ks.set_scaling_packed(buf)
    buf[:] = np.nan                                                       # the call has returned: the host buffer is the caller's again
    host["packed_again"] = ks.get_scaling_packed()
    r.stage()                                                             # a spin alone: K holds the last factor until it is over
    ks.assemble_only()
    host["kkt_assembled"] = np.tril(ks.kkt_matrix())
    scaling("v", "s")
    ks.check_factor()
    host["solve_after_check"] = ks.solve3x3(hx, hy, hz)
    return host


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_host_pointer_calls_are_valid_on_return(route):
    Q, A, G, n, m, p = _mixed_problem()
    real, _ = _mixed_real(np.random.default_rng(3), n, m, p)
    rng = np.random.default_rng(6)
    real = {k: real[k] for k in ("x", "y", "z", "v", "s", "X3", "Y3", "Z3")}
    real.update(v2=dev(_interior(MIXED_CONES, rng)), s2=dev(_interior(MIXED_CONES, rng)))
    dv, host = _handle_ab(_mixed_make(route, False, False), _host_seq, real, {}, "host-pointer calls, " + route, _mixed_scramble(n, m))
    assert np.array_equal(host["packed"], host["packed_again"]) and np.isfinite(host["kkt_factored"]).all()
    assert not np.array_equal(host["kkt_factored"], host["kkt_assembled"])
    assert all(np.isfinite(t).all() for t in host["solve3x3"])


def _host_problem(Q, A, G):
    """cip_problem with HOST pointers (column-major copies kept alive by the caller)"""
    from cipkkt import _lib as L
    keep = [np.asfortranarray(M, dtype=np.float64) for M in (Q, A, G)]
    ct = (C.c_int * len(MIXED_CONES))(*[{"R": 0, "Q": 1, "S": 2}[t] for t, _ in MIXED_CONES])
    cd = (C.c_int * len(MIXED_CONES))(*[k for _, k in MIXED_CONES])
    pr = L.CipProblem()
    pr.n, pr.m, pr.p, pr.ncones, pr.cone_type, pr.cone_dim = Q.shape[0], A.shape[0], G.shape[0], len(MIXED_CONES), ct, cd
    pr.Q, pr.ldq, pr.A, pr.lda, pr.G, pr.ldg = keep[0].ctypes.data, Q.shape[0], keep[1].ctypes.data, A.shape[0], keep[2].ctypes.data, G.shape[0]
    pr.route, pr.flags = L.ROUTE_SCHUR, 0
    return pr, keep + [ct, cd]


@pytest.mark.parametrize("source", ["host", "device", "device_csr"])
def test_update_problem_on_a_late_stream(source):
    """level 1 again behind the spin: from host pointers (overwritten as soon as the call has returned) and from device buffers
    that are themselves filled late on S -- dense, and the CSR arrays of A and Q in device memory, which the library reads back to
    the host; the factorisation and the solve that follow must see the new matrices"""
    from cipkkt import _lib as L
    Q, A, G, n, m, p = _mixed_problem()
    rng = np.random.default_rng(12)
    Q2 = Q + np.diag(rng.random(n))
    A2, G2 = A * 1.5, rng.standard_normal((p, n))
    names = ["Q", "A", "G"]
    real, _ = _mixed_real(np.random.default_rng(3), n, m, p)
    real = {k: real[k] for k in ("x", "y", "z", "v", "s")}
    real.update(Q=dev(Q2.T), A=dev(A2.T), G=dev(G2.T))                    # tensors (cols, rows) = column-major matrices
    outs = {"a": n, "b": p, "c": m}
    csr = source == "device_csr"
    if csr:
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        for key, M in (("Q", sp.csr_matrix(Q2)), ("A", sp.csr_matrix(A2))):
            M.sort_indices()
            assert M.nnz == sp.csr_matrix(Q if key == "Q" else A).nnz     # same pattern as the handle's
            del real[key]
            real.update({key + "_rp": i32(M.indptr), key + "_ci": i32(M.indices), key + "_v": dev(M.data)})
        names = [k for k in real if k[:2] in ("Q_", "A_")] + ["G"]

    def seq(ks, r, warm):
        if csr:
            r.stage(inputs=["x", "y", "z", "v", "s"] + names, outputs=["a", "b", "c"])
            pr, keep = _host_problem(Q2, A2, G2)
            pr.Q, pr.A, pr.G = None, None, r["G"].data_ptr()
            pr.Q_rowptr, pr.Q_colind, pr.Q_val = (r["Q_" + k].data_ptr() for k in ("rp", "ci", "v"))
            pr.A_rowptr, pr.A_colind, pr.A_val = (r["A_" + k].data_ptr() for k in ("rp", "ci", "v"))
            pr.flags = L.FLAG_DEVICE_PTRS | L.FLAG_Q_CSR
            _check(ks.lib.cip_update_problem(ks.h, C.byref(pr)))
        elif source == "device":
            r.stage(inputs=["x", "y", "z", "v", "s"] + names, outputs=["a", "b", "c"])
            pr, keep = _host_problem(Q2, A2, G2)
            pr.Q, pr.A, pr.G, pr.flags = r["Q"].data_ptr(), r["A"].data_ptr(), r["G"].data_ptr(), L.FLAG_DEVICE_PTRS
            _check(ks.lib.cip_update_problem(ks.h, C.byref(pr)))
        else:
            r.stage(inputs=["x", "y", "z", "v", "s"], outputs=["a", "b", "c"])
            pr, keep = _host_problem(Q2, A2, G2)
            _check(ks.lib.cip_update_problem(ks.h, C.byref(pr)))
            for M in keep[:3]:
                M[...] = np.nan
        ks.set_scaling_from_iterate(r["v"], r["s"])
        ks.factor(check=False)
        ks.solve3x3_dev(r["x"], r["y"], r["z"], r["a"], r["b"], r["c"])
        return {}

    def scramble(ks):                                                     # back to the first problem
        if csr:
            return
        pr, keep = _host_problem(Q, A, G)
        _check(ks.lib.cip_update_problem(ks.h, C.byref(pr)))
        ks.set_scaling_identity()
        ks.factor()

    dv, _ = _handle_ab(_mixed_make("schur", csr, csr), seq, real, outs, "cip_update_problem from %s pointers" % source, scramble)
    ah, bh, ch = (dv[k].cpu().numpy() for k in ("a", "b", "c"))
    assert np.isfinite(ah).all() and np.abs(G2 @ ah - real["y"].cpu().numpy()).max() < 1e-9 * (1 + np.abs(ah).max())


def _sol_bits(sol):
    return {"y": sol.y, "w": sol.w, "v": sol.v, "counts": np.array([sol.Iter, sol.n_factor, sol.n_solve])}


@pytest.mark.parametrize("name", ["combined", "psd_projection"])
def test_conicip_on_a_late_stream(name):
    import cipkkt
    Q, c, A, b, K, G, d, _ = getattr(P, name)()
    plain = cipkkt.conicIP(Q, c, A, b, K, G, d)
    assert plain.status == "Optimal"
    ks = cipkkt.KKTSystem(Q, A, G, K)
    try:
        ks.set_stream(LS.stream().cuda_stream)
        LS.spin(LS.SPIN_MIN_MS)
        late = cipkkt.conicIP(Q, c, A, b, K, G, d, system=ks)
    finally:
        ks.close()
    assert late.status == "Optimal"
    assert LS.differences(({}, _sol_bits(plain)), ({}, _sol_bits(late))) == []


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_graph_replay_on_a_late_stream(route, monkeypatch):
    """CIP_GRAPH=1 records nothing on the null stream: on S the factorisation and the solves are captured and replayed"""
    import cipkkt
    Q, c, A, b, K, G, d, _ = P.random_mixed(n=200, nq=3, kq=6, p=4, seed=77)
    monkeypatch.delenv("CIP_GRAPH", raising=False)
    plain = cipkkt.conicIP(Q, c, A, b, K, G, d, kktsolver=route)
    monkeypatch.setenv("CIP_GRAPH", "1")
    ks = cipkkt.KKTSystem(Q, A, G, K, route=route)
    try:
        ks.set_stream(LS.stream().cuda_stream)
        LS.spin(LS.SPIN_MIN_MS)
        late = cipkkt.conicIP(Q, c, A, b, K, G, d, system=ks)
    finally:
        ks.close()
    assert plain.status == late.status == "Optimal"
    assert LS.differences(({}, _sol_bits(plain)), ({}, _sol_bits(late))) == []


def test_host_scratch_is_not_mixed_up_between_two_handles():
    """dots and maxstep come back through host-mapped scratch that all handles of a thread share: two handles on two streams, one of
    them late, calling alternately -- each call returns its own values"""
    import cipkkt
    S = LS.stream()
    S2 = torch.cuda.Stream()
    n = 500
    rng = np.random.default_rng(21)
    mk = lambda: cipkkt.KKTSystem(np.eye(n), sp.identity(n, format="csr"), None, [("R", n)])
    h1, h2 = mk(), mk()
    try:
        x1, y1, x2, y2 = (dev(rng.random(n) + 0.1) for _ in range(4))
        d1, d2 = dev(rng.standard_normal(n)), dev(rng.standard_normal(n))
        want = (h1.dots([(x1, y1)]), h2.dots([(x2, y2), (y2, y2)]), h1.maxstep(x1, d1), h2.maxstep(x2, d2))
        h1.set_stream(S.cuda_stream)
        h2.set_stream(S2.cuda_stream)
        bufs = [torch.full_like(x1, LS.NAN) for _ in range(3)]
        torch.cuda.synchronize()
        got = []
        for which in (0, 1):
            with torch.cuda.stream(S):                                    # h1's inputs arrive late; h2's stream is idle
                torch.cuda._sleep(int(LS.SPIN_MIN_MS * LS.cycles_per_ms()))
                for t, src in zip(bufs, (x1, y1, d1)):
                    t.copy_(src, non_blocking=True)
            if which == 0:
                got += [h2.dots([(x2, y2), (y2, y2)]), h1.dots([(bufs[0], bufs[1])])]
            else:
                got += [h2.maxstep(x2, d2), h1.maxstep(bufs[0], bufs[2])]
            with torch.cuda.stream(S):
                for t in bufs:
                    t.fill_(LS.NAN)
            S.synchronize()
        assert LS.differences(({}, {"dots1": want[0], "dots2": want[1], "max1": want[2], "max2": want[3]}),
                              ({}, {"dots1": got[1], "dots2": got[0], "max1": got[3], "max2": got[2]})) == []
    finally:
        h1.close()
        h2.close()
        S2.synchronize()
