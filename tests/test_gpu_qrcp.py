"""The device rank-revealing QR (csrc/qrcp.hip: cip_qrcp_dev, cip_imcols_dev) and the pre-solve on top of it.

Inputs are seeded low-rank products randn(len, r) @ randn(r, cnt) scaled to ||M||_F = 1.  The factorisation is checked against what
a column-pivoted Householder QR promises -- reconstruction, the diagonal of R as a distance from the span of the columns chosen so
far, the greedy pivot rule, the numerical rank -- with scipy's geqp3 as the yardstick for the rounding level, and `imcols_hip` /
`preprocess_conicIP(rank_solver="device")` against the properties and cases of tests/test_preprocess.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import problems as P
import test_preprocess as TP

pytestmark = pytest.mark.gpu

# one lane, one column, wave and workgroup edges, long columns, cnt far above len
SHAPES = [(1, 1, 1), (3, 1, 1), (1, 5, 1), (12, 7, 5), (63, 65, 63), (64, 64, 64), (65, 63, 40), (517, 130, 70), (65, 300, 65),
          (300, 257, 257), (1025, 65, 33), (2051, 96, 96), (4099, 40, 40), (130, 1100, 130)]
# just past the register tile of the column update (24576 rows from the even row at or above the step): the first steps take the
# looped two-read form, the later ones the largest tile; odd and even leading dimension (8-byte and 16-byte accesses)
PAST_TILE = [(24579, 8, 8), (24580, 8, 8)]
IDS = lambda s: "%dx%d_r%d" % s
U = 2.0 ** -52


def lowrank(ln, cnt, r, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * ln + 3 * cnt + r)
    M = rng.standard_normal((ln, r)) @ rng.standard_normal((r, cnt))
    return M / np.linalg.norm(M)


@functools.lru_cache(maxsize=None)
def case(shape, stop=0.0):
    """(M0, device result, scipy's (Q, R, piv)) -- computed once per shape, never modified"""
    import cipkkt
    M0 = lowrank(*shape)
    got = cipkkt.qrcp_hip(M0, stop=stop)
    ref = sla.qr(M0, mode="economic", pivoting=True)
    for a in (M0,) + tuple(x for x in got if isinstance(x, np.ndarray)) + tuple(ref):
        a.setflags(write=False)
    return M0, got, ref


def raw_qrcp(M0, ld=None, stop=0.0, fill=np.nan):
    """cip_qrcp_dev on a buffer with leading dimension ld whose padding rows hold `fill`: (rc, buffer cnt x ld, tau, piv, rdiag, k)"""
    import torch
    from cipkkt import _lib as L
    lib = L.load()
    ln, cnt = M0.shape
    ld = ln if ld is None else ld
    buf = np.full((cnt, ld), fill)
    buf[:, :ln] = M0.T
    dev = torch.from_numpy(buf).cuda()
    nb = C.c_size_t()
    assert lib.cip_qrcp_workspace_bytes(ln, cnt, C.byref(nb)) == 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    kmax = min(ln, cnt)
    tau = torch.zeros(kmax, dtype=torch.float64, device="cuda")
    piv, rdiag, k = np.full(cnt, -1, dtype=np.int32), np.zeros(kmax), C.c_int(-1)
    rc = lib.cip_qrcp_dev(None, dev.data_ptr(), ln, cnt, ld, stop, ws.data_ptr(), tau.data_ptr(), piv.ctypes.data_as(L.c_int_p),
                          rdiag.ctypes.data_as(L.c_double_p), C.byref(k))
    torch.cuda.synchronize()
    return rc, dev.cpu().numpy(), tau.cpu().numpy(), piv, rdiag, k.value


def reconstruct(F, tau, k):
    """Q [R; remainder]: the returned reflectors applied to the returned matrix with zeros below the diagonal in the first k columns.
    In extended precision with plain sums: in fp64 the measure itself costs more than the factorisation (numpy's v @ X over a column
    of 24579 entries alone is wrong by 2e-15 here, and by how much depends on the memory order of F)."""
    X = np.array(F, dtype=np.longdouble)
    for j in range(k):
        X[j + 1:, j] = 0.0
    for j in range(k - 1, -1, -1):
        v = np.zeros(F.shape[0], dtype=np.longdouble)
        v[j] = 1.0
        v[j + 1:] = F[j + 1:, j]
        X[j:] -= np.longdouble(tau[j]) * np.outer(v[j:], (v[j:, None] * X[j:]).sum(axis=0))
    return X


def recon_error(F, tau, k, M0, piv):
    return float(np.linalg.norm((reconstruct(F, tau, k) - M0[:, piv]).astype(np.float64)))


def scipy_error(M0, ref=None):
    """scipy's own error on the same input: the smaller of ||Q R - M P||_F with its explicit Q and of the same measure as the
    device's (its raw reflectors through `reconstruct`)"""
    Qs, Rs, ps = ref if ref is not None else sla.qr(M0, mode="economic", pivoting=True)
    (h, tau), _, p = sla.qr(M0, mode="raw", pivoting=True)
    return min(float(np.linalg.norm(Qs @ Rs - M0[:, ps])), recon_error(h, tau, min(M0.shape), M0, p))


@pytest.mark.parametrize("shape", SHAPES + PAST_TILE, ids=IDS)
def test_reconstruction(shape):
    """||Q R - M P||_F within 8 x max(scipy's own error on the same input, 2^-52): both are a small multiple of the unit roundoff;
    the device sums in trees where LAPACK sums serially."""
    M0, (F, tau, piv, rdiag, k), (Qs, Rs, ps) = case(shape)
    assert k == min(shape[:2]) and sorted(piv) == list(range(shape[1]))
    np.testing.assert_array_equal(rdiag, np.diag(F)[:k])
    err = recon_error(F, tau, k, M0, piv)
    ref = scipy_error(M0, (Qs, Rs, ps))
    print("reconstruction %s: device %.3e scipy %.3e" % (shape, err, ref))
    assert err <= 8 * max(ref, U)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] <= 300], ids=IDS)
def test_rdiag_is_the_distance_and_the_pivot_is_the_largest(shape):
    """For every step j < k: |R_jj| is the distance of input column piv[j] from the span of the columns piv[:j] (twice-projected numpy
    QR) to 4e-15, and that distance is at least (1 - 1e-9) x the largest such distance over the columns still to choose from.  Run
    with stop = 1e-8, so that every step checked is one the factorisation took on data (k = r): past the rank the distances are
    numpy's own rounding noise and say nothing about the pivot rule."""
    M0, (F, tau, piv, rdiag, k), _ = case(shape, 1e-8)
    assert k == shape[2]
    worst_d, worst_p = 0.0, 1.0
    for j in range(k):
        rem = M0[:, piv[j:]].copy()
        if j:
            Qj = np.linalg.qr(M0[:, piv[:j]])[0]
            rem -= Qj @ (Qj.T @ rem)
            rem -= Qj @ (Qj.T @ rem)
        d = np.linalg.norm(rem, axis=0)
        worst_d = max(worst_d, abs(abs(rdiag[j]) - d[0]))
        worst_p = min(worst_p, d[0] / d.max())
    print("rdiag %s: worst deviation %.3e, worst pivot ratio 1 - %.3e" % (shape, worst_d, 1 - worst_p))
    assert worst_d <= 4e-15
    assert worst_p >= 1 - 1e-9


def _rank_inputs():
    out = [("lowrank_" + IDS(s), lowrank(*s)) for s in SHAPES]
    for delta in (1e-5, 1e-11):                 # three rows, the third nearly the first: kept at 1e-5, dropped at 1e-11
        rng = np.random.default_rng(11)
        G = rng.standard_normal((3, 40))
        G[2] = G[0] + delta * rng.standard_normal(40)
        out.append(("near_dependent_%g" % delta, (G / np.linalg.norm(G)).T))
    rng = np.random.default_rng(12)              # rows graded over six decades: all kept
    out.append(("graded", (10.0 ** np.linspace(3, -3, 7)[:, None] * rng.standard_normal((7, 30))).T))
    out.append(("eye_twice", np.vstack([np.eye(4), np.eye(4)[:2]]).T))
    return out


RANK_INPUTS = _rank_inputs()
RANK_EXPECT = {"near_dependent_1e-05": 3, "near_dependent_1e-11": 2, "graded": 7, "eye_twice": 4}


@pytest.mark.parametrize("name,M0", RANK_INPUTS, ids=[n for n, _ in RANK_INPUTS])
def test_rank_matches_scipy(name, M0):
    import cipkkt
    ds = np.abs(np.diag(sla.qr(M0, mode="r", pivoting=True)[0]))
    assert not np.any((ds >= 1e-10) & (ds <= 1e-6)), ds            # nothing near the threshold: the rank is well defined
    rdiag = cipkkt.qrcp_hip(M0)[3]
    assert rdiag.size == min(M0.shape)
    assert np.count_nonzero(np.abs(rdiag) > 1e-8) == np.count_nonzero(ds > 1e-8)
    if name in RANK_EXPECT:
        assert np.count_nonzero(np.abs(rdiag) > 1e-8) == RANK_EXPECT[name]


def test_early_stop():
    import cipkkt
    F, tau, piv, rdiag, k = cipkkt.qrcp_hip(np.zeros((37, 21)))
    assert k == 0 and tau.size == 0 and rdiag.size == 0 and list(piv) == list(range(21)) and not F.any()
    M0 = lowrank(517, 130, 3)
    F, tau, piv, rdiag, k = cipkkt.qrcp_hip(M0, stop=1e-8)
    assert k == 3 and sorted(piv) == list(range(130))
    assert np.all(np.abs(rdiag) > 1e-8)
    assert np.linalg.norm(F[3:, 3:]) <= 1e-8 * np.sqrt(127)         # what is left: every column at most `stop`
    assert recon_error(F, tau, k, M0, piv) <= 8 * max(scipy_error(M0), U)


@pytest.mark.parametrize("shape", [(12, 7, 5), (65, 63, 40), (300, 257, 257), (2051, 96, 96)], ids=IDS)
def test_padding_rows_are_never_touched_and_do_not_change_the_bits(shape):
    """ld = len + 5 with NaN in the padding rows: their bit patterns survive, and every output equals the ld = len run bit for bit
    (one of the two leading dimensions is even, the other odd: 16-byte against 8-byte accesses)"""
    M0 = lowrank(*shape)
    ln = shape[0]
    rc0, B0, tau0, piv0, rd0, k0 = raw_qrcp(M0)
    rc1, B1, tau1, piv1, rd1, k1 = raw_qrcp(M0, ld=ln + 5)
    assert rc0 == 0 and rc1 == 0 and k0 == k1 == min(shape[:2])
    pad = np.full((shape[1], 5), np.nan)
    assert np.array_equal(B1[:, ln:].view(np.uint64), pad.view(np.uint64))
    assert np.array_equal(B1[:, :ln].view(np.uint64), B0.view(np.uint64))
    assert np.array_equal(tau0.view(np.uint64), tau1.view(np.uint64)) and np.array_equal(rd0.view(np.uint64), rd1.view(np.uint64))
    assert np.array_equal(piv0, piv1)


@pytest.mark.parametrize("ln,cnt", [(5, 3), (3, 5)])
def test_the_entry_points_stay_inside_their_advertised_workspaces(ln, cnt):
    """cip_qrcp_dev and cip_imcols_dev on one buffer of exactly cip_*_workspace_bytes plus a 4096-byte tail of 0xA5 (the workspace
    itself starts as 0xA5 too): the tail keeps its bytes -- no member of either layout lies beyond the advertised size, at len > cnt
    and at len < cnt (min(len, cnt) sizes tau / rdiag / y) -- and the results pass the checks of test_reconstruction and
    test_imcols_hip_properties."""
    import torch
    import cipkkt
    from cipkkt import _lib as L
    lib = L.load()
    kmax = min(ln, cnt)
    M0 = lowrank(ln, cnt, kmax)

    def guarded(size_fn):
        nb = C.c_size_t()
        assert size_fn(ln, cnt, C.byref(nb)) == 0
        return torch.full((nb.value + 4096,), 0xA5, dtype=torch.uint8, device="cuda"), nb.value

    ws, nb = guarded(lib.cip_qrcp_workspace_bytes)
    dev = torch.from_numpy(np.ascontiguousarray(M0.T)).cuda()
    tau = torch.zeros(kmax, dtype=torch.float64, device="cuda")
    piv, rdiag, k = np.full(cnt, -1, dtype=np.int32), np.zeros(kmax), C.c_int(-1)
    rc = lib.cip_qrcp_dev(None, dev.data_ptr(), ln, cnt, ln, 0.0, ws.data_ptr(), tau.data_ptr(), piv.ctypes.data_as(L.c_int_p),
                          rdiag.ctypes.data_as(L.c_double_p), C.byref(k))
    torch.cuda.synchronize()
    assert rc == 0 and bool((ws[nb:] == 0xA5).all())
    assert k.value == kmax and sorted(piv) == list(range(cnt))
    assert recon_error(dev.cpu().numpy().T, tau.cpu().numpy(), kmax, M0, piv) <= 8 * max(scipy_error(M0), U)

    A = np.ascontiguousarray(M0.T)                                 # cnt rows of length len, rank min(len, cnt)
    b = A @ np.random.default_rng(ln).standard_normal(ln)
    ws, nb = guarded(lib.cip_imcols_workspace_bytes)
    rows, nrows, ok = np.zeros(cnt, dtype=np.int32), C.c_int(0), C.c_int(0)
    Ad, bd = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    rc = lib.cip_imcols_dev(None, Ad.data_ptr(), ln, cnt, ln, bd.data_ptr(), 1e-8, ws.data_ptr(), rows.ctypes.data_as(L.c_int_p),
                            C.byref(nrows), C.byref(ok), None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((ws[nb:] == 0xA5).all())
    got = [int(i) for i in rows[:nrows.value]]
    assert ok.value == 1 and len(got) == kmax == np.linalg.matrix_rank(A[got]) and got == sorted(set(got))
    want = cipkkt.imcols(A, b)
    assert (len(got), True) == (len(want[0]), want[1])


@pytest.mark.parametrize("shape", [(517, 130, 70), (130, 1100, 130)], ids=IDS)
def test_two_runs_give_identical_bits(shape):
    M0 = lowrank(*shape)
    a, b = raw_qrcp(M0), raw_qrcp(M0)
    assert a[0] == 0 and a[5] == b[5]
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)


def test_non_finite_input_is_refused():
    import cipkkt
    from cipkkt import _lib as L
    M0 = np.array(lowrank(65, 63, 40))
    M0[17, 29] = np.nan
    rc = raw_qrcp(M0)[0]
    assert rc == -1 and b"non-finite" in L.load().cip_last_error()
    with pytest.raises(cipkkt.CipError) as e:
        cipkkt.qrcp_hip(M0)
    assert e.value.code == -1
    with pytest.raises(cipkkt.CipError):
        cipkkt.imcols_hip(M0, np.zeros(65))


# ---- imcols on the device
def test_imcols_hip_properties():
    """`check_imcols` and the body of test_product_imcols_properties (tests/test_preprocess.py) with imcols_hip in place of imcols,
    plus the same properties at shapes with more than one workgroup's worth of rows and columns"""
    import cipkkt
    imcols = cipkkt.imcols_hip
    TP.check_imcols(imcols)
    rng = np.random.default_rng(5)
    for (mr, rk, nc) in [(7, 5, 12), (12, 3, 6), (9, 9, 9), (20, 4, 40), (6, 1, 3), (300, 129, 65), (130, 70, 517)]:
        rk = min(rk, nc)
        A = rng.standard_normal((mr, rk)) @ rng.standard_normal((rk, nc))
        x0 = rng.standard_normal(nc)
        rows, ok = imcols(A, A @ x0)
        r = np.linalg.matrix_rank(A)
        assert ok and len(rows) == r == rk and rows == sorted(set(rows))
        sv = np.linalg.svd(A[rows], compute_uv=False)
        assert sv[-1] > 1e-8 * sv[0]                                   # kept rows independent
        others = [i for i in range(mr) if i not in rows]
        if others:                                                     # dropped rows are combinations of the kept ones
            coef = np.linalg.lstsq(A[rows].T, A[others].T, rcond=None)[0]
            assert np.abs(A[rows].T @ coef - A[others].T).max() < 1e-9 * np.abs(A).max()
        if r < mr:                                                     # b moved off the range of A
            u = np.linalg.svd(A)[0][:, r]
            assert imcols(A, A @ x0 + u) == ([], False)
        assert imcols(1e6 * A, 1e6 * (A @ x0))[0] == rows
    As = sp.csr_matrix(np.vstack([np.eye(4), np.eye(4)[:2]]))
    rows, ok = imcols(As, np.array([1.0, 2, 3, 4, 1, 2]))
    assert ok and len(rows) == 4 and np.linalg.matrix_rank(As.toarray()[rows]) == 4


def test_imcols_hip_takes_column_blocks_of_every_kind():
    import torch
    import cipkkt
    rng = np.random.default_rng(9)
    n = 23
    B1 = rng.standard_normal((n, 4)) @ rng.standard_normal((4, 11))                  # rank 4
    B2 = sp.random(n, 9, density=0.2, random_state=3, format="csr")
    B3 = rng.standard_normal((n, 2))
    full = np.hstack([B1, B2.toarray(), B3])
    b = full @ rng.standard_normal(full.shape[1])
    want = cipkkt.imcols(full, b)
    got = cipkkt.imcols_hip([B1, B2, torch.from_numpy(B3).cuda(), np.zeros((n, 0))], b)
    assert got[1] and want[1] and len(got[0]) == len(want[0]) == np.linalg.matrix_rank(full)
    assert np.linalg.matrix_rank(full[got[0]]) == len(got[0])
    assert cipkkt.imcols_hip(torch.from_numpy(full).cuda(), torch.from_numpy(b).cuda()) == got
    assert cipkkt.imcols_hip([full], b) == got


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("kappa", [1e-8, 1.0, 1e8])
def test_imcols_hip_on_the_miles_problems(k, kappa):
    """G and [Q A' G'] of Miles's counter-examples (test/runtests.jl:592-651; c, A, b all scaled by kappa): row count and verdict of
    the host imcols"""
    import cipkkt
    c, A, b, con, var = P.miles_problem(k)
    Q, cc, Ai, bi, dims, G, d = P.mpb_to_conicip(kappa * c, kappa * A, kappa * b, con, var)
    want = cipkkt.imcols(G.toarray(), d)
    got = cipkkt.imcols_hip(G, d)
    assert (len(got[0]), got[1]) == (len(want[0]), want[1])
    keep = want[0]
    blocks = [Q, Ai.T.tocsr(), G.toarray()[keep, :].T]
    want = cipkkt.imcols(np.hstack([B.toarray() if sp.issparse(B) else B for B in blocks]), cc)
    got = cipkkt.imcols_hip(blocks, cc)
    assert (len(got[0]), got[1]) == (len(want[0]), want[1])


# ---- the pre-solve with the device QR
@pytest.mark.parametrize("check", [TP.check_redundant, TP.check_bad_dual, TP.check_infeasible, TP.check_miles],
                         ids=["redundant", "bad_dual", "infeasible", "miles"])
def test_preprocess_with_the_device_rank_solver(check):
    import cipkkt
    check(functools.partial(cipkkt.preprocess_conicIP, rank_solver="device"))


def test_device_rank_solver_has_no_size_limit(monkeypatch):
    """the counterpart of test_presolve_refuses_a_dense_qr_beyond_the_size_limit: the same rank-deficient program above the
    (lowered) limit solves with rank_solver="device" and is still refused by the default"""
    from cipkkt import preprocess as pp
    monkeypatch.setattr(pp, "DENSE_QR_LIMIT", 500)
    n = 10
    Q = np.zeros((2 * n, 2 * n))
    A = sp.hstack([sp.identity(n), sp.identity(n)], format="csr")
    sol = pp.preprocess_conicIP(Q, -np.ones(2 * n), A, np.zeros(n), [("R", n)], optTol=TP.OPT, rank_solver="device")
    assert np.linalg.norm(sol.y) < TP.TOL
    with pytest.raises(ValueError, match=r"20 x 30"):
        pp.preprocess_conicIP(Q, -np.ones(2 * n), A, np.zeros(n), [("R", n)])
