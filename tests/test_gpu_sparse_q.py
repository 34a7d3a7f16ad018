"""A CSR objective matrix Q (CIP_FLAG_Q_CSR, `sparse_q=True`) through every level: the assembly entrywise on both routes
(k_qcsr_fill_cols, k_qcsr_scatter, the Qin-less Schur formation), the mat-vec in both forms, factor and solves against the
true operator and against a dense-Q handle of the same problem, the regularised path, the interior-point loop on the
problems whose Q is structured, lock-step batches, and cip_update_problem.

The Q patterns: `diag` (positive, spread over 1e-3 .. 1e3), `zero` (nnz = 0), `rand` (symmetric, about 5 % dense, one empty
row, diagonally dominant elsewhere: positive semi-definite), `full` (a dense SPD matrix stored as CSR).  No stored zeros."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _kkt_ref as KR
import problems as P
from cipkkt import workloads as W
from oracle import kktsolvers as ok
from oracle.cones import vecm
from oracle.conicip import conicIP as oracle_conicIP, make_cone_ops
from oracle.kktsolvers import assemble3x3
from test_gpu_assembly import CASES, _csr, _gram_dev, _scalings, _syrk_form
from test_gpu_configs import check_optimality
from test_gpu_driver import OPT, TOL, assert_same_trajectory as kat_same_trajectory
from test_gpu_soc_large import _same_as_live_oracle

pytestmark = pytest.mark.gpu
U = np.finfo(np.float64).eps / 2


def q_pattern(kind, n, rng):
    if kind == "diag":
        d = 10.0 ** rng.uniform(-3.0, 3.0, n)
        d[:2] = (1e-3, 1e3)
        Q = sp.diags(d).tocsr()
    elif kind == "zero":
        Q = sp.csr_matrix((n, n))
    elif kind == "rand":
        B = np.triu(rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.05), 1)
        S = B + B.T
        e = n // 3                                            # an empty row (and column)
        S[e, :] = 0.0
        S[:, e] = 0.0
        dg = np.abs(S).sum(axis=1) + 0.1
        dg[e] = 0.0
        Q = sp.csr_matrix(S + np.diag(dg))
        assert Q.indptr[e] == Q.indptr[e + 1]
    else:
        M = rng.standard_normal((n, n))
        Q = sp.csr_matrix(M @ M.T / n + 0.5 * np.eye(n))
        assert Q.nnz == n * n
    Q.eliminate_zeros()
    Q.sort_indices()
    assert not (Q.data == 0).any() and (abs(Q - Q.T)).nnz == 0
    return Q


# ---------------------------------------------------------------------------------------------------------------- 1. assembly
# (route, A, n, p, cone_dims, Q patterns): the smallest shapes that reach each path
ASM = {
    "schur_dense_unsplit": ("schur", "dense", 200, 3, [("R", 150), ("Q", 40), ("Q", 3)], ("diag", "rand", "zero", "full")),
    # npad 256 = 3 tiles, 12 workgroups < 640, mpad 4112 >= 4096 and < 16384: split-K 64, 16 slices
    "schur_dense_splitk64": ("schur", "dense", 256, 0, [("R", 4100)], ("diag", "rand")),
    "schur_csr_many_q": ("schur", "csr", 301, 4, CASES["csr_many_q"][4], ("diag", "rand")),
    # m = 541 odd; k = 300 > 128 loops k_fill_ftf_qbig's gridDim.y
    "full_dense_odd_m": ("full3x3", "dense", 256, 5, [("R", 100), ("Q", 300), ("Q", 3), ("Q", 8), ("Q", 64), ("Q", 65), ("Q", 1)],
                         ("diag", "rand")),
    "full_csr_s_cone": ("full3x3", "csr", 120, 3, [("R", 90), ("Q", 30), ("Q", 4), ("S", 10)], ("diag", "rand")),
}


def test_case_table_reaches_the_named_forms():
    m = lambda name: sum(k for _, k in ASM[name][4])
    assert _syrk_form(200, m("schur_dense_unsplit")) == ("syrkq_64", 1)
    assert _syrk_form(256, m("schur_dense_splitk64")) == ("splitk_64", 16)
    assert m("full_dense_odd_m") == 541
    assert ASM["schur_csr_many_q"][2:5] == CASES["csr_many_q"][2:5]


def _asm_inputs(name, qkind):
    route, akind, n, p, cone_dims, _ = ASM[name]
    rng = np.random.default_rng(sum(map(ord, name + qkind)))
    m = sum(k for _, k in cone_dims)
    Q = q_pattern(qkind, n, rng)
    A = rng.standard_normal((m, n)) if akind == "dense" else _csr(m, n, 0.4 if n > 250 else 0.15, rng)
    G = rng.standard_normal((p, n)) if p else None
    return Q, A, G, cone_dims, route, akind, rng


def _check_assembly(ks, Q, A, G, cone_dims, route, akind, rng, what):
    for label, F in _scalings(cone_dims, rng):
        ks.set_scaling_packed(ks.pack_scaling(F, F.inv_adjoint()))
        ks.assemble_only()
        Kd = ks.kkt_matrix()
        K, copied, bound = KR.reference(Q, A, G, cone_dims, F, route, ks.Npad, csr=akind != "dense", gram=_gram_dev)
        try:
            KR.check(Kd, K, copied, bound)
        except AssertionError as e:
            raise AssertionError("%s, %s scaling: %s" % (what, label, e)) from None


@pytest.mark.parametrize("name, qkind", [(nm, q) for nm in ASM for q in ASM[nm][5]])
def test_assembly_matches_the_reference_entrywise(name, qkind):
    import cipkkt
    Q, A, G, cone_dims, route, akind, rng = _asm_inputs(name, qkind)
    ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route, sparse_q=True)
    try:
        _check_assembly(ks, Q, A, G, cone_dims, route, akind, rng, "%s / %s" % (name, qkind))
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------------------------------- 2. mat-vec
@pytest.mark.parametrize("qkind, n", [("diag", 2048), ("rand", 301), ("full", 200), ("zero", 130)])
def test_matvec_entrywise_and_reproducible(qkind, n):
    """cip_gemv_dev(CIP_MAT_Q) on a CSR Q: |y - (alpha Q x + beta y0)|_i <= 2 (rowlen_i + 2) u (|alpha| |Q| |x| + |beta y0|)_i -- one
    rounding per product, a sum of rowlen_i terms in any order, alpha, beta and the last addition; with beta = 0 y is not read
    (it holds NaN); two runs give the same bits.  diag at 2048 (where a dense handle takes the symmetric mat-vec) and zero run one
    thread per row (longest row <= 8 entries), rand and full one wave per row."""
    import cipkkt
    from cipkkt import _lib as L
    rng = np.random.default_rng(n)
    Q = q_pattern(qkind, n, rng)
    ks = cipkkt.KKTSystem(Q, sp.identity(n, format="csr"), None, [("R", n)], sparse_q=True)
    try:
        x, y0 = rng.standard_normal(n), rng.standard_normal(n)
        rowlen = np.diff(Q.indptr)
        absQx = abs(Q) @ np.abs(x)
        dx = torch.from_numpy(x).cuda()
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)):
            outs = []
            for _ in range(2):
                dy = torch.from_numpy(np.full(n, np.nan) if beta == 0.0 else y0.copy()).cuda()
                ks.gemv(L.MAT_Q, 0, alpha, dx, beta, dy)
                torch.cuda.synchronize()
                outs.append(dy.cpu().numpy())
            assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)), (alpha, beta)
            assert np.isfinite(outs[0]).all(), (alpha, beta)
            want = alpha * (Q @ x) + (beta * y0 if beta != 0.0 else 0.0)
            bound = 2 * (rowlen + 2) * U * (abs(alpha) * absQx + (np.abs(beta * y0) if beta != 0.0 else 0.0))
            err = np.abs(outs[0] - want)
            i = int(np.argmax(err - bound))
            print("%s n=%d (%g, %g): worst |err| %.3g against %.3g" % (qkind, n, alpha, beta, err[i], bound[i]))
            assert (err <= bound).all(), (alpha, beta, i, err[i], bound[i])
    finally:
        ks.close()


def test_device_resident_csr_arrays_are_copied_back_and_checked():
    """CIP_FLAG_DEVICE_PTRS without CIP_FLAG_CSR_HOST: Q's CSR arrays live in device memory; level 1 copies them back, checks them
    (a broken mirror entry is refused) and the handle multiplies with the same bits as one created from host arrays"""
    from cipkkt import _lib as L
    from cipkkt.kkt import make_problem
    lib = L.load()
    dev = torch.device("cuda:0")
    n = 200
    rng = np.random.default_rng(7)
    Q = q_pattern("rand", n, rng)
    A = rng.standard_normal((n, n))
    x = torch.from_numpy(rng.standard_normal(n)).to(dev)

    def product(values, host):
        Qv = Q.copy()
        Qv.data = values
        pr, keep, _ = make_problem(Qv, A, None, [("R", n)], "schur", dev, sparse_q=True)
        if not host:
            dv = [torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
                  for a, dt in ((Qv.indptr, np.int32), (Qv.indices, np.int32), (Qv.data, np.float64))]
            pr.Q_rowptr, pr.Q_colind, pr.Q_val = (C.c_void_p(t.data_ptr()) for t in dv)
            pr.flags = L.FLAG_DEVICE_PTRS | L.FLAG_Q_CSR
            keep.append(dv)
        torch.cuda.synchronize()
        h = C.c_void_p()
        rc = lib.cip_create_ex(C.byref(pr), C.byref(h))
        if rc != 0:
            return rc, lib.cip_last_error()
        y = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        L.check(lib.cip_gemv_dev(h, L.MAT_Q, 0, 1.0, x.data_ptr(), 0.0, y.data_ptr()))
        torch.cuda.synchronize()
        L.check(lib.cip_destroy(h))
        return 0, y.cpu().numpy()

    rc_h, y_host = product(Q.data, True)
    rc_d, y_dev = product(Q.data, False)
    assert rc_h == 0 and rc_d == 0
    assert np.array_equal(y_host.view(np.int64), y_dev.view(np.int64))
    np.testing.assert_allclose(y_dev, Q @ x.cpu().numpy(), rtol=1e-12, atol=1e-13)
    broken = Q.data.copy()
    k = int(np.flatnonzero(Q.indices != np.repeat(np.arange(n), np.diff(Q.indptr)))[0])      # an off-diagonal entry
    broken[k] = np.nextafter(broken[k], np.inf)
    rc, msg = product(broken, False)
    assert rc == -1 and b"mirror entry" in msg, (rc, msg)


# ---------------------------------------------------------------------------------------------------------------- 3. solves
def _berr(Z, sol, rhs, normZ=None):
    normZ = np.linalg.norm(Z, 2) if normZ is None else normZ
    return np.linalg.norm(Z @ sol - rhs) / (normZ * np.linalg.norm(sol) + np.linalg.norm(rhs))


def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M)


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_solves_against_the_true_operator_and_the_dense_handle(route):
    """the same problem as a dense-Q and a CSR-Q handle: factor, solve3x3, solve2x2 (Schur) and solve3x3_many with 3 columns have a
    normwise backward error ||Z x - r|| / (||Z|| ||x|| + ||r||) < 1e-12 against Z = [Q G' -A'; G 0 0; A 0 F'F] formed in numpy, and
    the difference of the two handles' solutions meets the same bound.  Schur: n = 640, A = I in CSR, R cone -- the size at which the
    dense handle takes the lazy copy of Q."""
    import cipkkt
    rng = np.random.default_rng(640)
    if route == "schur":
        n, p = 640, 0
        cone_dims = [("R", n)]
        A, G = sp.identity(n, format="csr"), None
    else:
        n, p = 120, 3
        cone_dims = [("R", 90), ("Q", 30), ("Q", 4), ("S", 10)]
        A, G = _csr(sum(k for _, k in cone_dims), n, 0.2, rng), rng.standard_normal((3, n))
    m = A.shape[0]
    Q = q_pattern("rand", n, rng)
    _, nt_scaling, _, _ = make_cone_ops(cone_dims)

    def interior():
        xs = []
        for t, k in cone_dims:
            if t == "R":
                xs.append(rng.random(k) + 0.1)
            elif t == "Q":
                x = rng.standard_normal(k)
                x[0] = np.linalg.norm(x[1:]) + 0.5
                xs.append(x)
            else:
                r = KR._order(k)
                M = rng.standard_normal((r, r))
                xs.append(vecm(M @ M.T / r + 0.5 * np.eye(r)))
        return np.concatenate(xs)

    F = nt_scaling(interior(), interior())
    Gd = G if G is not None else np.zeros((0, n))
    Z = assemble3x3(_dense(Q), _dense(A), Gd, F)
    normZ = np.linalg.norm(Z, 2)
    X, Y, Zr = rng.standard_normal((n, 3)), rng.standard_normal((p, 3)), rng.standard_normal((m, 3))
    sols = {}
    for form in ("dense", "csr"):
        ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route, sparse_q=form == "csr")
        try:
            ks.set_scaling_packed(ks.pack_scaling(F, F.inv_adjoint()))
            ks.factor()
            assert ks.health()["n_regularized"] == 0
            one = np.concatenate(ks.solve3x3(X[:, 0], Y[:, 0], Zr[:, 0]))
            many = np.vstack(ks.solve3x3_many(X, Y, Zr))
            two = np.concatenate(ks.solve2x2(X[:, 1], Y[:, 1])) if route == "schur" else None
            sols[form] = (one, many, two)
        finally:
            ks.close()
    rhs = np.vstack([X, Y, Zr])
    FtF = Z[n + p:, n + p:]
    S2 = None
    if route == "schur":
        Ad = _dense(A)
        S2 = np.block([[_dense(Q) + Ad.T @ np.linalg.solve(FtF, Ad), Gd.T], [Gd, np.zeros((p, p))]])
    for form, (one, many, two) in sols.items():
        be = [_berr(Z, one, rhs[:, 0], normZ)] + [_berr(Z, many[:, j], rhs[:, j], normZ) for j in range(3)]
        if two is not None:
            be.append(_berr(S2, two, np.concatenate([X[:, 1], Y[:, 1]])))
        print("%s %s Q: backward errors %s" % (route, form, ["%.2g" % b for b in be]))
        assert max(be) < 1e-12, (form, be)
    d1, dm, d2 = (None if a is None else a - b for a, b in zip(sols["dense"], sols["csr"]))
    cross = [np.linalg.norm(Z @ d1) / (normZ * np.linalg.norm(sols["csr"][0]) + np.linalg.norm(rhs[:, 0]))]
    cross += [np.linalg.norm(Z @ dm[:, j]) / (normZ * np.linalg.norm(sols["csr"][1][:, j]) + np.linalg.norm(rhs[:, j])) for j in range(3)]
    if d2 is not None:
        cross.append(np.linalg.norm(S2 @ d2) / (np.linalg.norm(S2, 2) * np.linalg.norm(sols["csr"][2]) + np.linalg.norm(rhs[:n + p, 1])))
    print("%s dense against CSR: %s" % (route, ["%.2g" % b for b in cross]))
    assert max(cross) < 1e-12, cross


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_regularised_path_refines_against_a_csr_q(route):
    """an LP-like system: Q = 0 (nnz = 0) and 16 free variables pinned only by G -- S = A'(F'F)^-1 A is singular, the first
    factorisation meets a bad pivot, the handle switches to the regularised factorisation, and solve3x3 refines with the residual of
    the TRUE operator (kkt3_residual: the Q term through the CSR mat-vec): backward error < 1e-12 against the unregularised Z."""
    import cipkkt
    rng = np.random.default_rng(12)
    n, p, k = 30, 16, 14
    Q = q_pattern("zero", n, rng)
    A = np.zeros((k, n))
    A[np.arange(k), np.arange(k)] = 1.0
    G = rng.standard_normal((p, n))
    cone_dims = [("R", k)]
    _, nt_scaling, _, _ = make_cone_ops(cone_dims)
    F = nt_scaling(rng.random(k) + 0.1, rng.random(k) + 0.1)
    x, y, z = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(k)
    Z = assemble3x3(np.zeros((n, n)), A, G, F)
    ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route, sparse_q=True)
    try:
        ks.set_scaling_packed(ks.pack_scaling(F, F.inv_adjoint()))
        ks.factor()
        sol = np.concatenate(ks.solve3x3(x, y, z))
        hl = ks.health()
        assert hl["n_regularized"] == 1 and hl["reg_rel"] > 0, hl
        be = _berr(Z, sol, np.concatenate([x, y, z]))
        print("regularised, %s: backward error %.2g" % (route, be))
        assert be < 1e-12, be
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the loop
@functools.lru_cache(maxsize=None)
def _oracle(name):
    if name == "soc_single":
        return oracle_conicIP(*W.soc_single(500, seed=42), optTol=1e-6, kktsolver=ok.pivot(ok.kktsolver_2x2))
    if name == "soc_many_small":
        return oracle_conicIP(*W.soc_many_small(500, 250), optTol=1e-6, kktsolver=ok.pivot(ok.kktsolver_2x2))
    if name == "readme":
        return oracle_conicIP(*W.c1_readme_boxqp(1000, seed=42), optTol=1e-6)
    Q, c, A, b, K, G, d, _ = P.lp_doc()
    return oracle_conicIP(Q, c, A, b, K, G, d, optTol=OPT, DTB=0.01, maxRefinementSteps=3)


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_loop_single_soc(route):
    """tests/test_gpu_soc_large.py::test_reference_single_soc_benchmark with Q = I in CSR: 6 iterations, the oracle's trajectory,
    the analytic minimiser c / |c|"""
    import cipkkt
    prob = W.soc_single(500, seed=42)
    ref = _oracle("soc_single")
    assert ref.Iter == 6
    sol = cipkkt.conicIP(*prob, optTol=1e-6, kktsolver=route, sparse_q=True)
    _same_as_live_oracle(sol, ref, "single SOC n=500 %s, CSR Q" % route)
    c = prob[1]
    assert np.linalg.norm(sol.y - c / np.linalg.norm(c)) < 1e-6


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_loop_many_small_socs(route):
    """tests/test_gpu_soc_large.py::test_reference_many_small_socs_benchmark with Q = I in CSR: 9 iterations"""
    import cipkkt
    prob = W.soc_many_small(500, 250)
    ref = _oracle("soc_many_small")
    assert ref.Iter == 9
    sol = cipkkt.conicIP(*prob, optTol=1e-6, kktsolver=route, sparse_q=True)
    _same_as_live_oracle(sol, ref, "250 x Q(3) %s, CSR Q" % route)
    Q, c, A, b, K = prob
    check_optimality(_dense(Q), c, _dense(A), b, K, np.zeros((0, 500)), np.zeros(0), sol, 1e-5)


def test_loop_readme_boxqp():
    """tests/test_gpu_configs_full.py::test_c1_readme_boxqp_n1000_vs_oracle_qr with Q (a product of two sparse draws, rows of
    about 0.63 n entries: the wave-per-row mat-vec) in CSR, both routes"""
    import cipkkt
    Q, c, A, b, K = W.c1_readme_boxqp(1000, seed=42)
    ref = _oracle("readme")
    assert ref.status == "Optimal"
    assert np.diff(sp.csr_matrix(Q).indptr).max() > 64
    for route in ("schur", "full3x3"):
        got = cipkkt.conicIP(Q, c, A, b, K, optTol=1e-6, kktsolver=route, sparse_q=True)
        assert got.status == "Optimal" and got.Iter == ref.Iter and got.n_factor == ref.n_factor
        np.testing.assert_allclose(got.y, ref.y, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(got.v, ref.v, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_loop_documentation_lp(route):
    """tests/test_gpu_driver.py::test_reference_kats[lp_doc] with Q as an empty CSR matrix (what every LP is)"""
    import cipkkt
    Q, c, A, b, K, G, d, expect = P.lp_doc()
    assert sp.issparse(Q) and Q.nnz == 0
    got = cipkkt.conicIP(Q, c, A, b, K, G, d, kktsolver=route, optTol=OPT, DTB=0.01, maxRefinementSteps=3, sparse_q=True)
    assert got.status == "Optimal"
    assert np.linalg.norm(got.y - expect) < TOL
    kat_same_trajectory(got, _oracle("lp_doc"))


# ---------------------------------------------------------------------------------------------------------------- 5. lock-step
def _box_problem(Q, seed):
    n = Q.shape[0]
    rng = np.random.default_rng(seed)
    return dict(Q=Q, c=rng.standard_normal(n), A=sp.identity(n, format="csr"), b=np.zeros(n), cone_dims=[("R", n)], G=None, d=None,
                kwargs={}, sparse_q=True)


def _raw_batch(entry, prs, fill):
    """`entry` (cip_conicip_lockstep / cip_conicip_mixed) on problem structs built with sparse_q, outputs pre-filled with `fill`:
    (rc, ys, vs, res)"""
    from cipkkt import _lib as L
    from cipkkt.kkt import make_problem
    lib = L.load()
    dev = torch.device("cuda:0")
    k = len(prs)
    structs = (L.CipProblem * k)()
    keep = []
    for i, pr in enumerate(prs):
        st, kp, _ = make_problem(pr["Q"], pr["A"], None, pr["cone_dims"], "schur", dev, sparse_q=True)
        structs[i] = st
        keep.append(kp)
    torch.cuda.synchronize()
    vp = C.c_void_p * k
    n = prs[0]["Q"].shape[0]
    cs = [np.ascontiguousarray(pr["c"]) for pr in prs]
    bs = [np.ascontiguousarray(pr["b"]) for pr in prs]
    ys = [np.full(n, fill) for _ in prs]
    vs = [np.full(n, fill) for _ in prs]
    zs = [np.zeros(1) for _ in prs]
    arr = lambda xs: vp(*[x.ctypes.data for x in xs])
    res = (L.CipResult * k)()
    opt = L.CipOptions(1e-6, 0.01, -1.0, -1.0, 3, 100, 0)
    args = [k, structs, arr(cs), arr(bs), arr(zs), C.byref(opt), arr(ys), arr(zs), arr(vs), res]
    rc = getattr(lib, entry)(*(args + ([2] if entry == "cip_conicip_mixed" else [])))
    del keep
    return rc, ys, vs, res


def test_lockstep_bit_identical_and_mixed_forms_refused():
    from cipkkt import _lib as L
    from cipkkt.batch import _solve_problems_native
    lib = L.load()
    dev = torch.device("cuda:0")
    n = 256
    prs = [_box_problem(q_pattern("diag", n, np.random.default_rng(70 + i)), 80 + i) for i in range(3)]
    prev = lib.cip_set_solve_block_max(lib.cip_lockstep_solve_block_for(3))
    try:
        one = _solve_problems_native(prs, dev, 1, "threads")
    finally:
        lib.cip_set_solve_block_max(prev)
    lock = _solve_problems_native(prs, dev, 1, "lockstep")
    assert all(s.status == "Optimal" for s in one)
    for i, (a, b) in enumerate(zip(lock, one)):
        assert (a.status, a.Iter) == (b.status, b.Iter), i
        for f in ("y", "w", "v"):
            assert np.array_equal(getattr(a, f).view(np.int64), getattr(b, f).view(np.int64)), (i, f)
    # one problem with another number of non-zeros: no lock-step, nothing written; the mixed entry point solves all three
    prs[1] = _box_problem(q_pattern("rand", n, np.random.default_rng(99)) + sp.identity(n, format="csr"), 81)
    assert prs[1]["Q"].nnz != prs[0]["Q"].nnz
    rc, ys, vs, res = _raw_batch("cip_conicip_lockstep", prs, -7.5)
    assert rc == L.E_UNSUPPORTED, (rc, lib.cip_last_error())
    assert all((y == -7.5).all() for y in ys) and all((v == -7.5).all() for v in vs)
    rc, ys, vs, res = _raw_batch("cip_conicip_mixed", prs, -7.5)
    assert rc == 0, lib.cip_last_error()
    assert [L.STATUS_NAMES[res[i].status] for i in range(3)] == ["Optimal"] * 3
    np.testing.assert_allclose(ys[0], one[0].y, rtol=1e-9, atol=1e-12)
    # a dense Q beside CSR ones of the same shape is refused the same way
    run = _solve_problems_native
    prs[1] = dict(_box_problem(q_pattern("diag", n, np.random.default_rng(5)), 81), sparse_q=False)
    with pytest.raises(L.CipError) as ei:
        run(prs, dev, 1, "lockstep")
    assert ei.value.code == L.E_UNSUPPORTED
    assert [s.status for s in run(prs, dev, 2, "auto")] == ["Optimal"] * 3


# ---------------------------------------------------------------------------------------------------------------- 6. update
def test_update_problem_same_nnz_new_values_and_refusals():
    import cipkkt
    from cipkkt import _lib as L
    from cipkkt.kkt import make_problem
    name = "schur_csr_many_q"
    Q, A, G, cone_dims, route, akind, rng = _asm_inputs(name, "rand")
    ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route, sparse_q=True)
    try:
        Q2 = Q.copy()
        Q2.data = Q2.data * 1.5                                # same pattern (same nnz), new values, still symmetric
        pr, keep, _ = make_problem(Q2, A, G, cone_dims, route, ks.device, sparse_q=True)
        torch.cuda.synchronize()
        L.check(ks.lib.cip_update_problem(ks.h, C.byref(pr)))
        _check_assembly(ks, Q2, A, G, cone_dims, route, akind, rng, "after cip_update_problem")
        ks.set_scaling_identity()
        ks.assemble_only()
        K0 = ks.kkt_matrix()
        # another nnz, and the dense form: refused, the handle goes on with what it holds
        Q3 = (Q2 + sp.identity(Q.shape[0], format="csr")).tocsr()
        assert Q3.nnz != Q2.nnz
        for Qb, sq in ((Q3, True), (q_pattern("zero", Q.shape[0], rng), True), (Q2, False)):
            prb, keepb, _ = make_problem(Qb, A, G, cone_dims, route, ks.device, sparse_q=sq)
            torch.cuda.synchronize()
            assert ks.lib.cip_update_problem(ks.h, C.byref(prb)) == -1, (Qb.nnz, sq)
            del keepb
        ks.set_scaling_identity()
        ks.assemble_only()
        assert np.array_equal(np.tril(ks.kkt_matrix()).view(np.int64), np.tril(K0).view(np.int64))
        ks.factor()
        x = rng.standard_normal(ks.n)
        a, b, c = ks.solve3x3(x, np.zeros(ks.p), np.zeros(ks.m))
        assert np.isfinite(a).all()
        del keep
    finally:
        ks.close()
