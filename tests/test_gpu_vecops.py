"""The HBM-bound vector kernels of csrc/vecops.hip through the public ABI (cip_gemv_dev, cip_dots_dev, cip_axpby_dev), entrywise
against the exact references and inside the derived bounds of tests/_vec_ref.py:

  a, b  k_gemv_t         every row count of _vec_ref.GEMV_ROWS (tests/test_vec_ref.py shows that the table reaches every class of
                         lane of the aligned path), both orientations of a dense A, the scalar fallback forced by a misaligned x
                         at every count, unit-vector probes around 128 / 512 / 1024 / 2048
  c     k_symv_*         orders 2048 (full groups of eight in the reduction) and 2176 (a ragged last group), graded symmetric Q
  d     k_spmv_csr       A and A' of a 700 x 301 CSR matrix with empty, one-entry and 130-entry rows
  e     k_dots1 / 2      13 lengths around 64, 256 and 8192 in one call, x != y in every pair, half of the pairs cancelling
  f     k_axpby          bit for bit against the exact fused multiply-add, past the 2048-workgroup cap of the grid-stride loop
  g     degenerate       p == 0 and m == 0: y = beta y
  h     k_loop_*         the native loop against the per-operation loop on problems of four workgroups whose section boundaries
                         are no multiple of 64

Every mat-vec call runs twice (equal bits) and, with beta == 0, on a y full of NaN (y is not read).  Each test prints the worst
err / bound it met."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _vec_ref as R
import problems as P

pytestmark = pytest.mark.gpu
AB = ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0))


def dev(a, off=False):
    """the array on the device; off: starting 8 bytes past a 16-byte boundary (a slice of a buffer one element longer)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not off:
        t = torch.from_numpy(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    t = torch.zeros(a.size + 1, dtype=torch.float64, device="cuda")
    t[1:] = torch.from_numpy(a).cuda()
    assert t[1:].data_ptr() % 16 == 8
    return t[1:]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def gemv_checked(ks, which, trans, alpha, dx, beta, y0, want, bound, what, y_off=False):
    """one call, twice: equal bits, finite from a NaN y when beta == 0, inside the bound; returns the worst err / bound"""
    outs = []
    for _ in range(2):
        dy = dev(np.full(len(y0), np.nan) if beta == 0.0 else y0, off=y_off)
        ks.gemv(which, trans, alpha, dx, beta, dy)
        outs.append(host(dy))
    assert same_bits(outs[0], outs[1]), what
    assert np.isfinite(outs[0]).all(), what
    err = np.abs(outs[0].astype(R.LD) - want).astype(np.float64)
    ok = err <= bound
    ratio = err / np.maximum(bound, np.finfo(np.float64).tiny)               # (a zero bound: an empty row, err == 0 there)
    j = int(np.argmax(ratio))
    assert ok.all(), "%s: entry %d of %d is off by %.3g, bound %.3g (%d entries outside)" % (what, j, len(y0), err[j], bound[j], (~ok).sum())
    return float(ratio[j])


def dense_handle(A):
    """a handle whose only large object is the dense A: one R cone over its rows, no G, Q = I in CSR (no dense Q is built)"""
    import cipkkt
    m, n = A.shape
    return cipkkt.KKTSystem(sp.identity(n, format="csr"), A, None, [("R", m)], sparse_q=True)


@functools.lru_cache(maxsize=1)
def _dense_A(m, n):
    return R.graded(np.random.default_rng(1000 * m + n), (m, n))


# ---------------------------------------------------------------------------------------------------------------- a. k_gemv_t
# (m, n): square over the row table, then few columns behind 1409 rows -- 5 (a second workgroup with one live wave) and 1 (one
# workgroup, three waves leave at j >= cols)
GEMV_SHAPES = [(r, r) for r in R.GEMV_ROWS] + [(5, 1409), (1, 1409)]


@pytest.mark.parametrize("m, n", GEMV_SHAPES, ids=lambda v: str(v))
def test_gemv_over_the_row_table(m, n):
    """MAT_A, trans = 0 is k_gemv_t(rows = n, cols = m, lda = npad): the aligned path, with the odd tail for odd n.  trans = 1 is
    k_gemv_t(rows = m, cols = n, lda = m): aligned for even m, the scalar fallback for odd m.  A misaligned x forces the fallback
    whatever the count; once with y misaligned as well."""
    from cipkkt import _lib as L
    A = _dense_A(m, n)
    rng = np.random.default_rng(m + 7 * n)
    ks = dense_handle(A)
    worst = 0.0
    try:
        for trans, Mt in ((0, A.T), (1, A)):                       # Mt[i, j]: row i of the kernel's column j
            rows, cols = Mt.shape
            x, y0 = rng.standard_normal(rows), rng.standard_normal(cols)
            dot = R.exact_matvec_t(Mt, x).astype(R.LD)
            absMx = np.abs(Mt).T @ np.abs(x)
            for x_off in (False, True):
                dx = dev(x, off=x_off)
                for alpha, beta in AB:
                    want = R.LD(alpha) * dot + (R.LD(beta) * y0.astype(R.LD) if beta != 0.0 else 0)
                    bound = R.matvec_bound(rows, alpha, absMx, beta, y0)
                    y_off = x_off and beta == 1.0
                    worst = max(worst, gemv_checked(ks, L.MAT_A, trans, alpha, dx, beta, y0, want, bound,
                                                    "A %dx%d trans=%d x_off=%d (%g, %g)" % (m, n, trans, x_off, alpha, beta), y_off))
    finally:
        ks.close()
    print("gemv %dx%d: worst err / bound %.3g" % (m, n, worst))


# ---------------------------------------------------------------------------------------------------------------- b. probes
def probe_indices(rows):
    ks = {0, rows - 1, rows - 2, rows - 3}            # rows odd: rows - 1 is the last even row (the tail), rows - 3 the last pair's
    for edge in (128, 512, 1024, 2048):
        if edge < rows:
            ks |= {edge - 1, edge}
    return sorted(k for k in ks if 0 <= k < rows)


@pytest.mark.parametrize("r", [129, 513, 1025, 1151, 2561, 2690])
def test_gemv_unit_vector_probes(r):
    """x = e_k, alpha = 1, beta = 0: the result is row k (trans = 0) or column k (trans = 1) of A bit for bit -- every other term
    is an exact zero; `abs` ignores the sign of a zero"""
    from cipkkt import _lib as L
    A = _dense_A(r, r)
    ks = dense_handle(A)
    try:
        for k in probe_indices(r):
            e = np.zeros(r)
            e[k] = 1.0
            for x_off in (False, True):
                dx = dev(e, off=x_off)
                for trans, want in ((0, A[:, k]), (1, A[k, :])):
                    dy = dev(np.full(r, np.nan))
                    ks.gemv(L.MAT_A, trans, 1.0, dx, 0.0, dy)
                    got = host(dy)
                    assert same_bits(np.abs(got), np.abs(want)), (r, k, x_off, trans, int(np.flatnonzero(np.abs(got) != np.abs(want))[0]))
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------------------------------- c. symv
def _graded_symmetric(n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    d = 10.0 ** rng.uniform(-3.0, 3.0, n)
    Q = np.tril(d[:, None] * (M + M.T) * d[None, :])
    return Q + np.tril(Q, -1).T                                    # symmetric bit for bit


@pytest.mark.parametrize("n", [2048, 2176])
def test_symmetric_matvec_entrywise(n):
    """a dense Q of the smallest order that gets the tile tables (2048: nb = 16, two full groups of eight in k_symv_reduce) and of
    2176 (nb = 17: a last group of one).  Q = D M D with D spread over six decades: an entry read from the wrong side of the
    diagonal, or a partial sum from the wrong table, is off by orders of magnitude.  A misaligned x leaves the tiles for
    k_gemv_t (cip_mul_Q); the same bound holds."""
    import cipkkt
    from cipkkt import _lib as L
    assert np.finfo(np.longdouble).eps < 2 ** -60
    Q = _graded_symmetric(n)
    assert np.array_equal(Q, Q.T)
    rng = np.random.default_rng(n + 1)
    x, y0 = rng.standard_normal(n), rng.standard_normal(n)
    Qx = R.ld_matvec(1.0, Q, x, 0.0, None)
    absQx = np.abs(Q) @ np.abs(x)
    ks = cipkkt.KKTSystem(Q, sp.identity(n, format="csr"), None, [("R", n)])
    worst = 0.0
    try:
        for x_off in (False, True):
            dx = dev(x, off=x_off)
            for alpha, beta in AB:
                want = R.LD(alpha) * Qx + (R.LD(beta) * y0.astype(R.LD) if beta != 0.0 else 0)
                bound = R.matvec_bound(n, alpha, absQx, beta, y0)
                worst = max(worst, gemv_checked(ks, L.MAT_Q, 0, alpha, dx, beta, y0, want, bound,
                                                "Q %d x_off=%d (%g, %g)" % (n, x_off, alpha, beta)))
        for k in (0, 127, 128, 2047, n - 1):
            e = np.zeros(n)
            e[k] = 1.0
            for x_off in (False, True):
                dy = dev(np.full(n, np.nan))
                ks.gemv(L.MAT_Q, 0, 1.0, dev(e, off=x_off), 0.0, dy)
                got = host(dy)
                assert same_bits(np.abs(got), np.abs(Q[:, k])), (n, k, x_off, int(np.flatnonzero(np.abs(got) != np.abs(Q[:, k]))[0]))
    finally:
        ks.close()
    print("symv %d: worst err / bound %.3g" % (n, worst))


# ---------------------------------------------------------------------------------------------------------------- d. CSR
def _csr_A(m, n, rng):
    """rows of 130 entries, of one entry and empty rows in turn; row 0 holds column 0 and column n - 1"""
    rows, cols = [], []
    for i in range(m):
        if i % 3 == 0:
            c = rng.choice(n, 130, replace=False)
            if i == 0:
                c[:2] = (0, n - 1)
                c = np.unique(c)
        elif i % 3 == 1:
            c = np.array([(7 * i) % n])
        else:
            c = np.zeros(0, dtype=np.int64)
        rows += [i] * len(c)
        cols += list(c)
    A = sp.csr_matrix((R.graded(rng, len(rows)), (rows, cols)), shape=(m, n))
    A.sort_indices()
    return A


def test_csr_matvec_with_A_and_its_transpose():
    """700 x 301: three workgroups of rows for A x, two for A'v (the CSR of A' is the library's own).  cip_create_ex accepts empty
    rows: a third of the rows of A have none, y = beta y there."""
    import cipkkt
    from cipkkt import _lib as L
    m, n = 700, 301
    rng = np.random.default_rng(700301)
    A = _csr_A(m, n, rng)
    lens = np.diff(A.indptr)
    assert set(lens.tolist()) >= {0, 1, 130} and A[0, 0] != 0 and A[0, n - 1] != 0 and m > 256 and n > 256
    T = A.T.tocsr()
    T.sort_indices()
    ks = cipkkt.KKTSystem(sp.identity(n, format="csr"), A, None, [("R", m)], sparse_q=True)
    worst = 0.0
    try:
        for trans, Mx in ((0, A), (1, T)):
            rows, cols = Mx.shape
            x, y0 = rng.standard_normal(cols), rng.standard_normal(rows)
            dot = R.exact_csr_matvec(Mx.indptr, Mx.indices, Mx.data, x).astype(R.LD)
            absMx = abs(Mx) @ np.abs(x)
            dx = dev(x)
            for alpha, beta in AB:
                want = R.LD(alpha) * dot + (R.LD(beta) * y0.astype(R.LD) if beta != 0.0 else 0)
                bound = R.matvec_bound(np.diff(Mx.indptr), alpha, absMx, beta, y0)
                worst = max(worst, gemv_checked(ks, L.MAT_A, trans, alpha, dx, beta, y0, want, bound,
                                                "CSR A trans=%d (%g, %g)" % (trans, alpha, beta)))
    finally:
        ks.close()
    print("spmv: worst err / bound %.3g" % worst)


# ---------------------------------------------------------------------------------------------------------------- e. dots
DOT_LENS = (0, 1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 16385, 100003)


@pytest.fixture(scope="module")
def small():
    """a small handle for the calls that use none of its matrices"""
    import cipkkt
    ks = cipkkt.KKTSystem(np.eye(5), np.eye(5), None, [("R", 5)])
    yield ks
    ks.close()


def _raw_dots(ks, pairs, fill=None):
    k = len(pairs)
    xs = (C.c_void_p * k)(*[p[0].data_ptr() for p in pairs])
    ys = (C.c_void_p * k)(*[p[1].data_ptr() for p in pairs])
    ln = (C.c_int * k)(*[p[0].numel() for p in pairs])
    out = (C.c_double * k)(*([fill] * k if fill is not None else []))
    return ks.lib.cip_dots_dev(ks.h, k, xs, ys, ln, out), list(out)


def test_dots_against_the_exact_dot(small):
    """13 pairs in one call, every pair with x != y (a kernel that read x twice fails); the odd-numbered pairs have y
    orthogonalised against x, so that the exact dot is about u sum |x_i y_i| and nothing but the bound's own scale passes; the
    last pair again as misaligned slices"""
    rng = np.random.default_rng(13)
    hx, hy = [], []
    for i, n in enumerate(DOT_LENS):
        x, y = R.graded(rng, n, 2.0), R.graded(rng, n, 2.0)
        if i % 2 == 1 and n > 1:
            y = R.orthogonalised(x, y)
        hx.append(x)
        hy.append(y)
    empty = dev(np.zeros(2))[:0]                                              # length 0 at a real address
    pairs = [(dev(x), dev(y)) if len(x) else (empty, empty) for x, y in zip(hx, hy)]
    hx.append(hx[-1])
    hy.append(hy[-1])
    pairs.append((dev(hx[-1], off=True), dev(hy[-1], off=True)))
    k = len(pairs)
    assert k == 14 and all(px.data_ptr() != py.data_ptr() for px, py in pairs[1:])
    got = small.dots(pairs)
    again = small.dots(pairs)
    assert same_bits(got, again)
    worst = 0.0
    for i in range(k):
        want, bound = R.exact_dot(hx[i], hy[i]), R.dot_bound(hx[i], hy[i])
        err = abs(got[i] - want)
        assert err <= bound, "pair %d (length %d): %.17g against %.17g, off by %.3g, bound %.3g" % (i, len(hx[i]), got[i], want, err, bound)
        if len(hx[i]) > 1 and i % 2 == 1 and i < len(DOT_LENS):
            assert abs(want) < 1e-12 * np.abs(hx[i] * hy[i]).sum(), i     # the pair does cancel
        worst = max(worst, err / bound if bound > 0 else 0.0)
    assert got[0] == 0.0
    print("dots: worst err / bound %.3g" % worst)


def test_dots_unit_vector_probes(small):
    """x = e_k: the dot is y_k exactly, at the first and last element of a thread's, a workgroup's and the grid's stride"""
    n = DOT_LENS[-1]
    rng = np.random.default_rng(14)
    y = R.graded(rng, n, 2.0)
    dy = dev(y)
    probes = (0, 255, 256, 8191, 8192, n - 1)
    pairs = []
    for k in probes:
        e = np.zeros(n)
        e[k] = 1.0
        pairs.append((dev(e), dy))
    got = small.dots(pairs)
    assert same_bits(np.abs(got), np.abs(y[list(probes)])), (got, y[list(probes)])


def test_dots_count_limit(small):
    """32 pairs in one call pass; 33 are refused and nothing is written"""
    rng = np.random.default_rng(15)
    hx = [rng.standard_normal(65 + i) for i in range(33)]
    hy = [rng.standard_normal(65 + i) for i in range(33)]
    pairs = [(dev(a), dev(b)) for a, b in zip(hx, hy)]
    rc, got = _raw_dots(small, pairs[:32], fill=-7.5)
    assert rc == 0
    for i in range(32):
        assert abs(got[i] - R.exact_dot(hx[i], hy[i])) <= R.dot_bound(hx[i], hy[i]), i
    rc, got = _raw_dots(small, pairs, fill=-7.5)
    assert rc != 0 and got == [-7.5] * 33, (rc, got)


# ---------------------------------------------------------------------------------------------------------------- f. axpby
def _bitwise_indices(n):
    return np.unique(np.array([i for i in [0, 255, 256, 257] + list(range(max(0, n - 300), n)) + list(range(0, n, 4099)) if i < n], dtype=np.int64))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 524288, 524289, 1048583])
def test_axpby_is_one_rounded_product_and_one_fused_multiply_add(n, small):
    """y = fma(alpha, x, fl(beta y)) (vecops.hip: axpby_op): bit for bit against the exact fused multiply-add at the first
    elements, around 256, at the last 300 and at every 4099th element, within u |want| (1 + 2^-10) of the extended value everywhere.
    Above 524288 elements the grid stops at 2048 workgroups and every thread strides."""
    assert np.finfo(np.longdouble).eps < 2 ** -60
    rng = np.random.default_rng(n + 3)
    x, y0 = R.graded(rng, n, 2.0), R.graded(rng, n, 2.0)
    alpha, beta = 1.0 / 3.0, -2.7
    if n == 0:
        guard = dev(np.array([1.5, 2.5]))
        from cipkkt import _lib as L
        L.check(small.lib.cip_axpby_dev(small.h, 0, alpha, guard.data_ptr(), beta, guard.data_ptr()))
        assert host(guard).tolist() == [1.5, 2.5]
        return
    dx, dy = dev(x), dev(y0)
    small.axpby(alpha, dx, beta, dy)
    got = host(dy)
    t = beta * y0                                                     # the rounded product
    idx = _bitwise_indices(n)
    want_bits = R.exact_fma(alpha, x[idx], t[idx])
    assert same_bits(got[idx], want_bits), int(idx[np.flatnonzero(got[idx] != want_bits)[0]])
    want = R.ld_fma(alpha, x, t)
    err = np.abs(got.astype(R.LD) - want)
    lim = R.U * np.abs(want) * (1 + 2.0 ** -10)
    i = int(np.argmax(err - lim))
    assert (err <= lim).all(), (n, i, float(err[i]), float(lim[i]))
    print("axpby %d: worst err / (u |want|) %.3g" % (n, float(np.max(err / np.maximum(lim, np.finfo(np.float64).tiny)))))
    # beta == 0: y is not read
    dy = dev(np.full(n, np.nan))
    small.axpby(alpha, dx, 0.0, dy)
    assert same_bits(host(dy), alpha * x)
    # y aliased to x, as cip_gemv_dev itself calls it: y = beta y
    dy = dev(y0)
    small.axpby(0.0, dy, beta, dy)
    assert same_bits(host(dy), beta * y0)


# ---------------------------------------------------------------------------------------------------------------- g. degenerate
def _beta_only(ks, which, n, xlen):
    """alpha op(M) x + beta y with a matrix of no rows: 0 (from a NaN y), y and 0.5 y"""
    rng = np.random.default_rng(n)
    y0 = rng.standard_normal(n)
    dx = dev(np.full(max(xlen, 1), np.nan))
    for beta, start, want in ((0.0, np.full(n, np.nan), np.zeros(n)), (1.0, y0, y0), (0.5, y0, 0.5 * y0)):
        dy = dev(start)
        ks.gemv(which, 1, 1.25, dx, beta, dy)
        assert same_bits(host(dy), want), (which, beta)
    # the other orientation has no output rows: nothing is touched
    guard = dev(np.array([1.5, 2.5]))
    ks.gemv(which, 0, 1.25, dev(rng.standard_normal(n)), 0.0, guard)
    assert host(guard).tolist() == [1.5, 2.5]


def test_gemv_with_no_equalities(small):
    from cipkkt import _lib as L
    assert small.p == 0
    _beta_only(small, L.MAT_G, small.n, 0)


def test_gemv_with_no_cone_rows():
    import cipkkt
    from cipkkt import _lib as L
    rng = np.random.default_rng(0)
    n = 7
    M = rng.standard_normal((n, n))
    ks = cipkkt.KKTSystem(M.T @ M + np.eye(n), np.zeros((0, n)), None, [])
    try:
        assert ks.m == 0
        _beta_only(ks, L.MAT_A, n, 0)
    finally:
        ks.close()


# ---------------------------------------------------------------------------------------------------------------- h. the loop
LOOP = {
    # every cone an R cone: the fused kernels form the cone terms themselves (f != NULL) and the fused solve4x4 pre / post run
    "all_r_dense": (dict(n=300, nq=0, kq=0, p=7, dense_A=True), 907),
    "all_r_csr": (dict(n=300, nq=0, kq=0, p=7, dense_A=False), 907),
    # with Q cones the cone results are passed in (f == NULL)
    "with_q_cones": (dict(n=300, nq=3, kq=6, p=7, dense_A=True), 943),
}


@pytest.mark.parametrize("name", list(LOOP))
def test_fused_loop_kernels_across_workgroups(name):
    """tests/test_gpu_driver.py::test_native_driver_matches_per_operation_driver on problems whose n + p + 2 m elements fill four
    workgroups of k_loop_resid / k_loop_corr / k_loop_refine, with the sections y | w | v | s starting at 300, 307 and 607 (or
    625): no boundary on a multiple of 64.  Same fields, same 1e-12."""
    import cipkkt
    kw, total = LOOP[name]
    Q, c, A, b, K, G, d = P.random_mixed(**kw)[:7]
    n, m, p = Q.shape[0], A.shape[0], G.shape[0]
    assert n + p + 2 * m == total and 768 < total <= 1024
    assert all(s % 64 for s in (n, n + p, n + p + m))
    assert all(t == "R" for t, _ in K) == (kw["nq"] == 0)
    sols = [cipkkt.conicIP(Q, c, A, b, K, G, d, optTol=1e-7, driver=drv) for drv in ("native", "python")]
    nat, py = sols
    assert nat.status == py.status == "Optimal"
    assert (nat.Iter, nat.n_factor, nat.n_solve, len(nat.trace)) == (py.Iter, py.n_factor, py.n_solve, len(py.trace))
    for tn, tp in zip(nat.trace, py.trace):
        assert set(tn) == set(tp)
        for key in tn:
            assert tn[key] == pytest.approx(tp[key], rel=1e-12, abs=1e-300), (key, tn["Iter"])
    for xn, xp in ((nat.y, py.y), (nat.w, py.w), (nat.v, py.v)):
        np.testing.assert_allclose(xn, xp, rtol=1e-12, atol=0, equal_nan=True)
    for f in ("Mu", "prFeas", "duFeas", "muFeas", "pobj", "dobj"):
        assert getattr(nat, f) == pytest.approx(getattr(py, f), rel=1e-12)
