"""A give-up of the fused LDL' panel chain, on every path that runs it.  The fused chain waits inside a launch for workgroups of the
same launch; the wait is bounded and then the factorisation raises info[3] ("K holds a partial factor").  Every consumer must either
redo the factorisation on the three-launch chain or report the give-up.  cip_debug_chain_giveup's POISON kind leaves what a real
give-up can leave -- the flag AND a factor that is wrong by 2^-20 in one 64 x 64 block -- so a path that ignores info[3] computes a
measurably wrong answer here.  Every test checks that the hook fired and compares with a plain reference (numpy, the oracle, or the
run without a give-up)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SKIP = 1 << 16           # n = count + SKIP * skip + kind bits (include/cipkkt.h: cip_debug_chain_giveup)
PIVOT = 1 << 28
POISON = 1 << 29
REDO_PIVOT = 1 << 30
F64 = dict(dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def lib():
    import cipkkt
    return cipkkt._lib.load()


@contextlib.contextmanager
def armed(lib, n):
    lib.cip_debug_chain_giveup(n)
    try:
        yield
    finally:
        lib.cip_debug_chain_giveup(0)


def _fallbacks(ks):
    return ks.lib.cip_get_chain_fallbacks(ks.h)


def _switched_on(ks):
    import cipkkt
    rel, switched = C.c_double(), C.c_int()
    cipkkt._lib.check(ks.lib.cip_get_regularization(ks.h, C.byref(rel), C.byref(switched)))
    return switched.value


# ---------------------------------------------------------------------------------------------------- 1. the handle, one problem and lock-step
def test_poisoned_giveup_on_a_handle_and_in_a_lockstep_group(lib):
    """The scenario of test_gpu_panel_chain.py's give-up test with the POISON kind: the handle redoes the factorisation (same bits as
    the run without a give-up), the lock-step group ejects its problems (each solved alone)."""
    import cipkkt
    from cipkkt.batch import _solve_problems_native
    from cipkkt.workloads import c5_batch
    dev = torch.device("cuda:0")
    prs = c5_batch(count=6, n=640, seed=5100, device=dev)
    pr = prs[0]
    ref = cipkkt.conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], optTol=1e-6)
    assert ref.status == "Optimal"
    ks = cipkkt.KKTSystem(pr["Q"], pr["A"], None, pr["cone_dims"])
    try:
        with armed(lib, 1 | POISON):
            got = cipkkt.conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], optTol=1e-6, system=ks)
            assert lib.cip_debug_chain_giveup(-1) == 0                       # the hook fired
        assert _fallbacks(ks) == 1
    finally:
        ks.close()
    assert (got.status, got.Iter, got.n_solve) == (ref.status, ref.Iter, ref.n_solve)
    assert np.array_equal(got.y, ref.y) and np.array_equal(got.v, ref.v)
    one = _solve_problems_native(prs, dev, 1, "lockstep")
    with armed(lib, 1 | POISON):
        two = _solve_problems_native(prs, dev, 1, "lockstep")
        assert lib.cip_debug_chain_giveup(-1) == 0
    st = (C.c_int * 3)()
    lib.cip_lockstep_stats(st)
    assert st[1] == 6 and st[2] == 6, list(st)
    for a, b in zip(two, one):
        assert (a.status, a.Iter) == (b.status, b.Iter) and a.status == "Optimal"
        assert np.allclose(a.y, b.y, rtol=1e-9, atol=1e-12)                # (alone: another solve block than in the group -> rounding)


# ---------------------------------------------------------------------------------------------------- 2, 3. speculative *_dev solves
def _box_qp(n, seed):
    from cipkkt import workloads as W
    Q, c, A, b, K = W.c2_problem(n, seed=seed)
    return np.asarray(Q), A, K


def _spec_solve(ks, x, y, z, a, b, c):
    """solve3x3_dev right behind an enqueued factorisation, then cip_check_factor: either call may say "repeat them" (CIP_E_RETRY);
    the answer kept is that of the last solve.  Returns how many times the solve was repeated."""
    import cipkkt
    from cipkkt import _lib as L
    repeats = 0
    try:
        ks.solve3x3_dev(x, y, z, a, b, c)
    except cipkkt.CipError as e:
        assert e.code == L.E_RETRY, str(e)
        ks.solve3x3_dev(x, y, z, a, b, c)
        repeats += 1
    rc = ks.lib.cip_check_factor(ks.h)
    if rc == L.E_RETRY:
        ks.solve3x3_dev(x, y, z, a, b, c)
        repeats += 1
    else:
        L.check(rc)
    torch.cuda.synchronize()
    assert repeats <= 1, "repeated twice"
    return repeats


def test_speculative_solve_after_a_poisoned_giveup_is_repeated_or_right(lib):
    """Order 4096, the handle's SECOND factorisation (the first one verified): a solve3x3_dev right behind cip_factor goes ahead
    without waiting for the pivot flag.  With a give-up in that factorisation the library must say "repeat them" (CIP_E_RETRY) --
    from the solve or from cip_check_factor -- and the answer kept must solve the 3x3 system (F = I)."""
    import cipkkt
    n = 4096
    Q, A, K = _box_qp(n, 91)
    ks = cipkkt.KKTSystem(Q, A, None, K)
    try:
        ks.set_scaling_identity()
        ks.factor(check=True)
        rng = np.random.default_rng(4)
        x, z = torch.as_tensor(rng.standard_normal(n), **F64), torch.as_tensor(rng.standard_normal(n), **F64)
        y = torch.zeros(0, **F64)
        a, c = torch.zeros(n, **F64), torch.zeros(n, **F64)
        b = torch.zeros(0, **F64)
        with armed(lib, 1 | POISON):
            ks.factor(check=False)
            _spec_solve(ks, x, y, z, a, b, c)
            assert lib.cip_debug_chain_giveup(-1) == 0
        assert _fallbacks(ks) == 1
        Qd, Ad = torch.as_tensor(Q, **F64), torch.as_tensor(A.toarray(), **F64)
        r1 = Qd @ a - Ad.t() @ c - x
        r3 = Ad @ a + c - z                                   # F = I
        scale = 1 + max(float(torch.linalg.norm(v)) for v in (a, c))
        assert max(float(torch.linalg.norm(r1)), float(torch.linalg.norm(r3))) < 1e-8 * scale
    finally:
        ks.close()


def test_a_bad_pivot_in_the_redo_of_a_giveup_switches_the_regularisation_on(lib):
    """after a give-up with speculative solves outstanding, the redo's own pivot flags must go through the pivot checks
    (here the redo reports a wrong-sign pivot: the automatic regularisation switches on) before "repeat them" is returned.  The
    answer kept must equal the oracle's kktsolver_qr (src/kktsolvers.jl:18-58)."""
    import cipkkt
    from oracle.conicip import make_cone_ops
    from oracle.kktsolvers import kktsolver_qr
    n = 4096
    Q, A, K = _box_qp(n, 92)
    ks = cipkkt.KKTSystem(Q, A, None, K)
    try:
        ks.set_scaling_identity()
        ks.factor(check=True)
        rng = np.random.default_rng(6)
        xh, zh = rng.standard_normal(n), rng.standard_normal(n)
        x, z = torch.as_tensor(xh, **F64), torch.as_tensor(zh, **F64)
        y, b = torch.zeros(0, **F64), torch.zeros(0, **F64)
        a, c = torch.zeros(n, **F64), torch.zeros(n, **F64)
        with armed(lib, 1 | POISON | REDO_PIVOT):
            ks.factor(check=False)
            _spec_solve(ks, x, y, z, a, b, c)
            assert lib.cip_debug_chain_giveup(-1) == 0
        assert _fallbacks(ks) == 1
        assert _switched_on(ks) == 1
        _, nt_scaling, _, _ = make_cone_ops(K)
        e = np.ones(n)
        F = nt_scaling(e, e)                                  # F = I
        ra, _, rc_ = kktsolver_qr(Q, A, np.zeros((0, n)), K)(F, F.inv_adjoint())(xh, np.zeros(0), zh)
        ref = np.concatenate([ra, rc_])
        got = np.concatenate([a.cpu().numpy(), c.cpu().numpy()])
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-10
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------------------- 4. graph replay
def test_giveup_under_graph_replay_redoes_on_the_three_launch_chain(lib, monkeypatch):
    """CIP_GRAPH=1: the factorisation is recorded once and replayed.  A give-up in a replay must be redone on the three-launch chain
    -- a NEW recording; replaying the recorded fused chain again would meet the second armed give-up.  The hook fires on
    replays of a graph that holds the fused chain, and only on those: one of the two give-ups is left."""
    import cipkkt
    from cipkkt import workloads as W
    monkeypatch.setenv("CIP_GRAPH", "1")
    n = 1024
    Q, c, A, b, K = W.c2_problem(n, seed=93)

    def run(arm):
        ks = cipkkt.KKTSystem(Q, A, None, K)
        try:
            if arm:
                with armed(lib, 2 + SKIP * 1 | POISON):              # the first factorisation (recorded, then replayed) is left alone
                    sol = cipkkt.conicIP(Q, c, A, b, K, optTol=1e-6, system=ks)
                    left = lib.cip_debug_chain_giveup(-1)
            else:
                sol, left = cipkkt.conicIP(Q, c, A, b, K, optTol=1e-6, system=ks), None
            return sol, _fallbacks(ks), left
        finally:
            ks.close()
    ref, f0, _ = run(False)
    got, f1, left = run(True)
    assert ref.status == "Optimal" and f0 == 0
    assert left == 1, "give-ups left on the hook: %d (2 = none fired, 0 = the stale fused graph was replayed again)" % left
    assert f1 == 1
    assert (got.status, got.Iter, got.n_solve) == (ref.status, ref.Iter, ref.n_solve)
    assert np.array_equal(got.y, ref.y) and np.array_equal(got.v, ref.v)


# ---------------------------------------------------------------------------------------------------- 5. large S cones
@pytest.fixture(scope="module")
def large_s_refs():
    return {}


@pytest.mark.parametrize("r,n,p,seed", [(256, 24, 0, 639913), (640, 12, 0, 31337)])
def test_large_s_cone_programs_with_a_poisoned_giveup(lib, large_s_refs, r, n, p, seed):
    """The large-S-cone path (order >= 133) factors matrices of its own: Kz / Ks of the NT scaling, the max-step's X = L D L', the
    inertia certificate of the Lanczos max-step.  A give-up armed at the k-th fused factorisation of the run, k = 0 .. 8 (which
    covers every one of those kinds in the first iterations), must leave status, iteration count and iterates exactly as without it,
    within the oracle's trajectory tolerances of test_gpu_sdp.py, with the handle reporting the one fall-back."""
    import cipkkt
    from cipkkt import workloads as W
    from oracle import kktsolvers as ok
    from oracle.conicip import conicIP as oracle_conicIP
    prob = W.c4_sdp(r=r, n=n, p=p, seed=seed)
    Q, c, A, b, K, G, d = prob
    ref = oracle_conicIP(*prob, optTol=1e-6, kktsolver=ok.kktsolver_schur_exact)
    base = cipkkt.conicIP(*prob, optTol=1e-6)
    assert base.status == ref.status == "Optimal" and base.Iter == ref.Iter
    for k in range(9):
        ks = cipkkt.KKTSystem(Q, A, G, K)
        try:
            with armed(lib, 1 + SKIP * k | POISON):
                got = cipkkt.conicIP(Q, c, A, b, K, G, d, optTol=1e-6, system=ks)
                assert lib.cip_debug_chain_giveup(-1) == 0, k
            assert _fallbacks(ks) == 1, k
        finally:
            ks.close()
        assert (got.status, got.Iter) == (base.status, base.Iter), k
        assert np.array_equal(got.y, base.y) and np.array_equal(got.v, base.v), k
        np.testing.assert_allclose(got.y, ref.y, rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(got.v, ref.v, rtol=1e-7, atol=1e-8)


# ---------------------------------------------------------------------------------------------------- 6. the stand-alone entry point
@pytest.mark.parametrize("N", [128, 1024])
def test_standalone_factor_reports_a_poisoned_giveup(lib, N):
    """cip_ldlt_factor_dev after a give-up: either an error (CIP_E_RETRY: K must be supplied again) or a factor that reconstructs
    K to 1e-13 -- never rc 0 / info 0 with the partial factor."""
    from cipkkt import _lib as L
    g = torch.Generator(device="cuda")
    g.manual_seed(N)
    M = torch.randn(N, N, generator=g, **F64)
    Kmat = (M @ M.t() / N + torch.eye(N, **F64)).contiguous()
    nbytes = C.c_size_t()
    L.check(lib.cip_ldlt_workspace_bytes(N, C.byref(nbytes)))
    ws = torch.zeros(nbytes.value // 8 + 8, **F64)
    dK = Kmat.clone()
    info = C.c_int(-1)
    with armed(lib, 1 | POISON):
        rc = lib.cip_ldlt_factor_dev(None, dK.data_ptr(), N, N, ws.data_ptr(), C.byref(info))
        assert lib.cip_debug_chain_giveup(-1) == 0
    torch.cuda.synchronize()
    if rc == 0 and info.value == 0:
        Fm = dK.t()                                             # dK holds the factor column-major: its row-major view is the transpose
        Lf = torch.tril(Fm, -1) + torch.eye(N, **F64)
        D = torch.diagonal(Fm)
        rec = (Lf * D[None, :]) @ Lf.t()
        err = float(torch.tril(rec - Kmat).abs().max() / Kmat.abs().max())
        assert err < 1e-13, "rc 0, info 0 and ||L D L' - K|| / ||K|| = %g" % err
    else:
        assert rc == L.E_RETRY, (rc, info.value)
        assert "partial factor" in lib.cip_last_error().decode()
