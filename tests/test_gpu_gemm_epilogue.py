"""The C operand of the fp64 GEMM tile epilogues (csrc/cip_gemm_tile.h: gemm_tile_64, csrc/gemm_f64.hip: gemm_tile_128) and the
y operand of the column-dot gemv (csrc/vecops.hip: k_gemv_t), on EXACT cases.

The epilogues fetch a lane's share of C in one batch -- in the trailing update inside the k-loop, two k-tiles before its end --
and only then update and store.  What such code can get wrong is which fetched value meets which accumulator, the tile edges
and the short k-loops (one, two and three k-tiles, where the fetch has to come before the loop or in its first trip).  With
small-integer operands every product and every partial sum is an integer far below 2^53, so the result does not depend on the
order of summation and has to equal the host's integer arithmetic bit for bit; each case first asserts on the CPU that its
int64 and float64 references agree.

EPI_LAZYC is not repeated here: tests/test_gpu_kernels.py::test_lazy_copy_of_Q_gives_the_same_factor_and_step compares it bit
for bit with the eager copy at n = 1024, 2048 and 4096 (with the lazy copy on, the first trailing update of its factorisation
is cip_gemm_lower_lazyc: the in-loop fetch from Qin and the diagonal from Cdiag).  k_solve_step's tgt operand is covered
by the sweeps' bitwise tests (test_solve4x4_fused_r_path_bitwise, test_side_stream_solve_preparation_bitwise)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    import cipkkt
    return cipkkt._lib.load()


def _padded_colmajor(Mat, ld):
    """flat column-major image of Mat at leading dimension ld, NaN in the padding rows"""
    rows, cols = Mat.shape
    buf = np.full((cols, ld), NAN)
    buf[:, :rows] = Mat.T
    return buf


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# form -> (M, N, lower_only, the kernel the dispatch rules of cip_gemm_lower / cip_gemm_rect choose)
FORMS = {
    "lower_256": (256, 256, 1, "k_ldlt_trailing_64"),
    "rect_256x384": (256, 384, 0, "k_gemm_nt_64"),          # 6 128-tiles < 256
    "rect_2048": (2048, 2048, 0, "k_gemm_nt_128"),          # 256 128-tiles
}
CASES = [(f, K) for f in FORMS for K in (16, 32, 48)] + [("lower_256", 896)]


@pytest.mark.parametrize("form,K", CASES, ids=["%s-K%d" % c for c in CASES])
def test_gemm_nt_exact_on_integers(lib, form, K):
    """C0 + alpha A B' with A, B integers in [-3, 3], C0 integers in [-2^20, 2^20], alpha in {-1, 0.5}: bit for bit the integer
    result; leading dimensions M + 2, N + 6, M + 4 with NaN padding rows that stay NaN; lower form: the lower triangle, and the
    128-tiles above the diagonal (NaN on entry) untouched."""
    from cipkkt import _lib as L
    M, N, lower, _ = FORMS[form]
    rng = np.random.default_rng(1000 * M + N + K)
    Ai = rng.integers(-3, 4, (M, K))
    Bi = rng.integers(-3, 4, (N, K))
    Ci = rng.integers(-2 ** 20, 2 ** 20 + 1, (M, N))
    Pi = Ai @ Bi.T
    Pf = Ai.astype(np.float64) @ Bi.astype(np.float64).T
    assert np.array_equal(Pf, Pi.astype(np.float64)) and np.abs(Pi).max() < 2 ** 20
    C0 = Ci.astype(np.float64)
    above = np.zeros((M, N), dtype=bool)             # lower form: the 128-tiles strictly above the diagonal
    if lower:
        ti = np.arange(M)[:, None] // 128
        tj = np.arange(N)[None, :] // 128
        above = ti < tj
        C0[above] = NAN
    lda, ldb, ldc = M + 2, N + 6, M + 4
    dA = torch.from_numpy(_padded_colmajor(Ai.astype(np.float64), lda)).cuda()
    dB = torch.from_numpy(_padded_colmajor(Bi.astype(np.float64), ldb)).cuda()
    c_img = _padded_colmajor(C0, ldc)
    for alpha in (-1.0, 0.5):
        want = C0 + alpha * Pf
        # the int64 reference, scaled by two so that alpha = 0.5 stays in the integers
        assert np.array_equal((2.0 * want)[~above], (2 * Ci + int(2 * alpha) * Pi)[~above].astype(np.float64))
        dC = torch.from_numpy(c_img.copy()).cuda()
        L.check(lib.cip_gemm_nt_dev(None, M, N, K, alpha, dA.data_ptr(), lda, dB.data_ptr(), ldb, dC.data_ptr(), ldc, lower))
        torch.cuda.synchronize()
        img = dC.cpu().numpy().reshape(N, ldc)
        assert np.isnan(img[:, M:]).all(), "padding rows of C written (alpha %g)" % alpha
        got = img[:, :M].T
        cmp = np.ones((M, N), dtype=bool)
        if lower:
            cmp = np.tri(M, N, dtype=bool)             # the strictly upper part of a diagonal tile is scratch
            assert np.array_equal(_bits(got)[above], _bits(C0)[above]), "a tile above the diagonal was touched (alpha %g)" % alpha
        bad = cmp & (_bits(got) != _bits(want))
        assert not bad.any(), (alpha, int(bad.sum()), np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("n,m", [(200, 72), (201, 72)])
def test_schur_formation_exact_on_integers(n, m):
    """EPI_SYRKQ through a handle: dense integer A, integer symmetric Q at its own pitch n, one R cone with the packed scaling all
    ones, so F = I and the Schur block is Q + A'A exactly.  n = 201: the single-row edge row + 1 == nvalid and an odd pitch."""
    import cipkkt
    rng = np.random.default_rng(n)
    Ai = rng.integers(-3, 4, (m, n))
    Qi = rng.integers(-2 ** 20, 2 ** 20 + 1, (n, n))
    Qi = np.tril(Qi) + np.tril(Qi, -1).T
    Si = Qi + Ai.T @ Ai
    Sf = Qi.astype(np.float64) + Ai.astype(np.float64).T @ Ai.astype(np.float64)
    assert np.array_equal(Sf, Si.astype(np.float64))
    ks = cipkkt.KKTSystem(Qi.astype(np.float64), Ai.astype(np.float64), None, [("R", m)], route="schur")
    try:
        ks.set_scaling_packed(np.ones(m))
        ks.assemble_only()
        Kd = ks.kkt_matrix()
    finally:
        ks.close()
    low = np.tri(n, dtype=bool)
    bad = low & (_bits(Kd[:n, :n]) != _bits(Sf))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("p", [1024, 1152])
def test_gemv_reads_y_only_when_beta_is_not_zero(p):
    """k_gemv_t through cip_gemv_dev(CIP_MAT_G) -- the binding of test_gemv_and_dots -- on integer data, p rows per column dot
    (1024: one trip of the eight-load loop; 1152: plus a 128-row tail) and n = 1280 rows the other way round: beta = 0 with NaN
    in y on entry returns the exact product, beta = 1 the exact sum."""
    import cipkkt
    from cipkkt import MAT_G
    n, m = 1280, 8
    rng = np.random.default_rng(p)
    Gi = rng.integers(-3, 4, (p, n))
    Q = np.eye(n)
    A = np.eye(m, n)
    wi = rng.integers(-5, 6, p)
    xi = rng.integers(-5, 6, n)
    yn = rng.integers(-2 ** 20, 2 ** 20 + 1, n)
    yp = rng.integers(-2 ** 20, 2 ** 20 + 1, p)
    f = lambda v: v.astype(np.float64)
    assert np.array_equal(f(Gi).T @ f(wi), f(Gi.T @ wi)) and np.array_equal(f(Gi) @ f(xi), f(Gi @ xi))
    ks = cipkkt.KKTSystem(Q, A, f(Gi), [("R", m)], route="schur")
    try:
        dw, dx = torch.from_numpy(f(wi)).cuda(), torch.from_numpy(f(xi)).cuda()
        for trans, dv, prod, y0 in ((1, dw, Gi.T @ wi, yn), (0, dx, Gi @ xi, yp)):
            y = torch.full((len(y0),), NAN, dtype=torch.float64, device="cuda")
            ks.gemv(MAT_G, trans, 2.0, dv, 0.0, y)
            got = y.cpu().numpy()
            assert np.isfinite(got).all(), "beta = 0 read y (trans %d)" % trans
            assert np.array_equal(got, f(2 * prod)), trans
            y = torch.from_numpy(f(y0)).cuda()
            ks.gemv(MAT_G, trans, -1.0, dv, 1.0, y)
            assert np.array_equal(y.cpu().numpy(), f(y0 - prod)), trans
    finally:
        ks.close()
