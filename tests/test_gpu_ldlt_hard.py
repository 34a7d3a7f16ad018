"""The blocked LDL' (csrc/ldlt.hip, csrc/diag.hip, the trailing update of csrc/gemm_f64.hip) and the triangular sweeps on stored
block inverses (cip_ldlt_solve, k_solve_step, csrc/solve_many.hip), ENTRYWISE on graded quasi-definite matrices: the factor
read back from the device against K within |K - L D L'| <= C_F N u |L||D||L'| + the micro-inverse term, every solve against the
factor within the block-inverse bound, both derived in tests/_ldlt_ref.py.  The matrices come from there too (Schur
complements with weights over 12 decades, literal 3x3 matrices with |L| up to 1e6, a regularised singular system); the table
GPU_CASES picks orders and knobs by the dispatch rules (tests/test_ldlt_ref.py checks the table against the rules and shows
every member to be factorisable, so nothing here skips).  Also: pivot reporting at every boundary of the blocking, the GEMM
entry point on row-scaled operands, and handles with hard Nesterov-Todd scalings.

Residuals are evaluated in long double on the host: the whole lower triangle up to order 1024, above it a fixed row sample
(two rows of every 64-row band and the last 128 rows) and, additionally, the whole lower triangle on the device in fp64 --
that checker's own rounding, gamma_(N+2) (|K| + |L||D||L'|) <= (2 N + 4) u |L||D||L'|, is added to the bound.

Every solve prints a line "SOLVE | case | order | Bs | form | x plain substitution bound | backward error" (pytest -s): the
table in DESIGN_LOG.md ("The LDL' and its solves on graded matrices") is made of them.  Wall time of this file on an MI355X
host: 65 s for 31 of its 33 tests (measured without the order-4608 handle row and the case full6_1536_bs512), 24 s of it the
order-8192 case and 10 s the order-4608 case (long-double row samples on the host)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _ldlt_ref as R

pytestmark = pytest.mark.gpu

F64 = dict(dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def lib():
    import cipkkt
    return cipkkt._lib.load()


@contextlib.contextmanager
def knobs(lib, chain=-1, nbo=0, bs=0, fused=-1, side=-1):
    prev = (lib.cip_set_ldlt_fused_chain(chain), lib.cip_set_solve_block_max(bs), lib.cip_set_solve_fused(fused),
            lib.cip_set_ldlt_side_prep(side), lib.cip_set_ldlt_outer_block(-1))      # (-1 is no width: the setter only reports)
    lib.cip_set_ldlt_outer_block(nbo)
    try:
        yield
    finally:
        lib.cip_set_ldlt_fused_chain(prev[0])
        lib.cip_set_solve_block_max(prev[1])
        lib.cip_set_solve_fused(prev[2])
        lib.cip_set_ldlt_side_prep(prev[3])
        lib.cip_set_ldlt_outer_block(prev[4])


class Standalone:
    """K (numpy, symmetric) in an (N x ld) device buffer, factored by cip_ldlt_factor_dev; rows N .. ld-1 hold NaN"""

    def __init__(self, lib, K, pad=0, expect_info=0):
        from cipkkt import _lib as L
        self.lib, self.N, self.ld = lib, K.shape[0], K.shape[0] + pad
        nb = C.c_size_t()
        L.check(lib.cip_ldlt_workspace_bytes(self.N, C.byref(nb)))
        self.ws = torch.zeros(nb.value // 8 + 8, **F64)
        self.buf = torch.full((self.N, self.ld), float("nan"), **F64)             # column j = row j of the tensor
        self.buf[:, :self.N] = torch.as_tensor(K, **F64).t()
        info = C.c_int(-1)
        self.rc = lib.cip_ldlt_factor_dev(None, self.buf.data_ptr(), self.N, self.ld, self.ws.data_ptr(), C.byref(info))
        torch.cuda.synchronize()
        self.info = info.value
        if expect_info == 0:
            L.check(self.rc)
            assert self.info == 0, "bad pivot reported at column %d" % self.info
            assert torch.isnan(self.buf[:, self.N:]).all()                          # rows N .. ld-1 are never touched

    def factor(self):
        return self.buf[:, :self.N].t().cpu().numpy()

    def solve(self, b):
        from cipkkt import _lib as L
        x = torch.as_tensor(b, **F64).clone()
        L.check(self.lib.cip_ldlt_solve_dev(None, self.buf.data_ptr(), self.N, self.ld, self.ws.data_ptr(), x.data_ptr()))
        torch.cuda.synchronize()
        return x.cpu().numpy()

    def many(self, B):
        """B: (nrhs, N) numpy, one right-hand side per row"""
        from cipkkt import _lib as L
        nrhs, ldb = B.shape[0], self.N + 24
        nb = C.c_size_t()
        L.check(self.lib.cip_ldlt_solve_many_scratch_bytes(self.N, nrhs, C.byref(nb)))
        scratch = torch.empty(max(nb.value // 8, 1), **F64)
        X = torch.full((nrhs, ldb), float("nan"), **F64)
        X[:, :self.N] = torch.as_tensor(B, **F64)
        L.check(self.lib.cip_ldlt_solve_many_dev(None, self.buf.data_ptr(), self.N, self.ld, self.ws.data_ptr(), scratch.data_ptr(),
                                                 X.data_ptr(), ldb, nrhs))
        torch.cuda.synchronize()
        assert torch.isnan(X[:, self.N:]).all()
        return X[:, :self.N].cpu().numpy()


def _device_factor_check(K, F):
    """the whole lower triangle in fp64 on the device, the checker's rounding added to the bound (module docstring)"""
    N = K.shape[0]
    Kd, Fd = torch.as_tensor(K, **F64), torch.as_tensor(F, **F64)
    eye = torch.eye(N, **F64)
    Ld = torch.tril(Fd, -1) + eye
    d = torch.diagonal(Fd).clone()
    del Fd, eye
    E = torch.tril(Kd - (Ld * d) @ Ld.t()).abs()
    del Kd
    G = Ld.abs() * d.abs()
    B = G @ Ld.abs().t()
    Mx, _ = R.micro_matrices(R.split_factor(F)[0])
    X = torch.einsum("rbk,bkj->rbj", G.view(N, N // 16, 16), torch.as_tensor(Mx, **F64))
    below = torch.arange(N, device="cuda")[:, None] >= (torch.arange(N // 16, device="cuda")[None, :] + 1) * 16
    X = (X * below[:, :, None]).reshape(N, N)
    bound = ((R.C_F + 2) * N + 4) * R.U * (1.0 + 2.0 * N * R.U) * B + 34.0 * R.U * X
    low = torch.ones(N, N, dtype=torch.bool, device="cuda").tril()
    bad = low & ~(E <= bound)
    ratio = torch.where(low & (bound > 0), E / torch.where(bound > 0, bound, torch.ones_like(bound)), torch.zeros_like(E))
    k = int(torch.argmax(ratio))
    return dict(ok=not bool(bad.any()), ratio=float(ratio.flatten()[k]), at=(k // N, k % N), nbad=int(bad.sum()))


def _check_factor(label, K, F):
    N = K.shape[0]
    assert np.isfinite(np.tril(F)).all(), label
    if N <= 1024:
        fc = R.factor_check(K, F)
    else:
        dc = _device_factor_check(K, F)
        print("FACTOR | %s | %d | device fp64, whole triangle: |E| <= %.3g x bound at %s" % (label, N, dc["ratio"], dc["at"]))
        assert dc["ok"], (label, dc)
        fc = R.factor_check(K, F, rows=R.sample_rows(N), wide_B=N <= 2048)
    print("FACTOR | %s | %d | long double%s: |E| <= %.3g x bound at %s, %.1f u B, micro |L11||inv L11| <= %.3g"
          % (label, N, "" if N <= 1024 else " (row sample)", fc["ratio"], fc["at"], fc["textbook"], fc["micro"]))
    assert fc["ok"], (label, fc)


def _report(label, N, Bs, form, sc):
    print("SOLVE | %s | %d | %d | %s | %.3g | %.2g | (%.3g x bound)" % (label, N, Bs, form, sc["plain"], sc["nbe"], sc["ratio"]))
    assert sc["ok"], (label, form, {k: v for k, v in sc.items() if k not in ("r", "bound")})


@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_standalone_factor_and_solves_meet_the_entrywise_bounds(lib, name):
    c = R.GPU_CASES[name]
    case = R.build_case(name)
    K, N = case.K, case.K.shape[0]
    widths, Bs, fused = R.dispatch(N, c["chain"], c["nbo"], c["bs"], c["fused"])
    rng = np.random.default_rng(sum(map(ord, name)))
    knorm = np.linalg.norm(K)
    with knobs(lib, c["chain"], c["nbo"], c["bs"], c["fused"]):
        f = Standalone(lib, K, pad=c.get("pad", 0))
        F = f.factor()
        _check_factor(name, K, F)
        assert np.array_equal(np.sign(np.diag(F)), R.expected_signs(case)), name
        if not c.get("solve", True):
            return
        sb = R.SolveBound(F, Bs, knorm)
        form = "one launch per step" if fused else "two launches per step"
        for trial in range(2):
            b = rng.standard_normal(N) * (10.0 ** rng.uniform(-3.0, 3.0, N) if trial else 1.0)
            _report(name, N, Bs, form, sb.check(b, f.solve(b), R.C_S["fused" if fused else "gemv"]))
        for nrhs in c.get("many", ()):
            Bm = rng.standard_normal((nrhs, N))
            Xm = f.many(Bm)
            for j in sorted({0, nrhs - 1, min(63, nrhs - 1), min(64, nrhs - 1)}):
                one = nrhs == 1                                          # cipkkt.h: nrhs == 1 is the single solve
                _report("%s col %d of %d" % (name, j, nrhs), N, Bs, form if one else "k_gemm_tn",
                        sb.check(Bm[j], Xm[j], R.C_S[("fused" if fused else "gemv") if one else "many"]))


# ------------------------------------------------------------------------------------------------------ pivot reporting
def _spd_cheap(n, rng):
    """symmetric, eigenvalues within 2 +- 0.9 (a scaled Wigner matrix + 2 I): no product to form at large orders"""
    if n == 0:
        return np.zeros((0, 0))
    Rm = rng.uniform(-1.0, 1.0, (n, n))
    return (Rm + Rm.T) / (2.0 * np.sqrt(n)) + 2.0 * np.eye(n)


def _with_bad_pivot(N, cols, rng):
    """[[S1, 0], [0, S2]] with S2[0, 0] replaced at column cols[0] = c: S1 factors without touching S2, so pivot c is exactly
    what was planted (0.0: then Inf / NaN follow in S2, whose first column is full); further entries of cols: (column, value)
    planted on the diagonal as well"""
    (c, v0), more = cols[0], cols[1:]
    K = np.zeros((N, N))
    K[:c, :c] = _spd_cheap(c, rng)
    K[c:, c:] = _spd_cheap(N - c, rng)
    K[c, c] = v0
    for j, v in more:
        K[j, j] = v
    return K


# 0-based columns: the last column of a micro-panel and the first of the next (15 | 16), the same for a panel (127 | 128) and an
# outer block of nbo 512 (511 | 512), their neighbours 17 and 129, the first and the last column
PIVOT_1024 = [0, 15, 16, 17, 127, 128, 129, 511, 512, 1023]


@pytest.mark.parametrize("chain", [0, 3])
def test_first_bad_pivot_is_reported_at_its_own_column(lib, chain):
    """cip_ldlt_factor_dev stores the first zero / non-finite pivot, 1-based, whatever follows it (diag.hip: the 0 * NaN guard)"""
    rng = np.random.default_rng(7)
    plans = [(1024, 512, [(c, 0.0)]) for c in PIVOT_1024]
    plans += [(1024, 512, [(c, v)]) for c in (17, 512, 1023) for v in (float("nan"), float("inf"))]
    plans += [(1024, 512, [(129, 0.0), (600, float("nan"))]), (1024, 512, [(129, float("inf")), (130, 0.0)])]   # two: the earlier one
    # inside the automatic wide last block of order 4608 (columns 1792 ..), and its last column
    plans += [(4608, 0, [(3000, 0.0)]), (4608, 0, [(3001, float("nan"))]), (4608, 0, [(4607, 0.0)])]
    for N, nbo, cols in plans:
        K = _with_bad_pivot(N, cols, rng)
        with knobs(lib, chain=chain, nbo=nbo):
            f = Standalone(lib, K, expect_info=cols[0][0] + 1)
        assert f.rc == 0, (N, cols, f.rc)
        assert f.info == cols[0][0] + 1, "order %d, planted %r: reported column %d" % (N, cols, f.info)
    # and a clean matrix of the same construction reports none
    with knobs(lib, chain=chain, nbo=512):
        assert Standalone(lib, _with_bad_pivot(1024, [(512, 2.0)], rng)).info == 0


# ----------------------------------------------------------------------------------------------------------------- GEMM
# C += alpha A B': every entry is C_ij + alpha sum_k a_ik b_jk, K fused multiply-adds in some order (at most K additions of
# terms and K merges of partial sums), one product with alpha and one addition to C: (2 K + 2) u <= 3 K u for K >= 16, relative
# to |C| + |alpha| |A||B|'.
GEMM_C = 3
GEMM_FORMS = {          # (M, N, lower_only): 128-tiles -> kernel, by the rules of cip_gemm_lower / cip_gemm_rect (gemm_f64.hip)
    "k_gemm_nt_128": (2048, 2048, 0),            # 256 tiles: not "skinny"
    "k_gemm_nt_64": (1920, 2048, 0),             # 240 tiles < 256: quarter tiles
    "k_ldlt_trailing_64": (1024, 1024, 1),       # lower only
}


def test_gemm_table_reaches_the_named_kernels():
    for name, (M, N, lower) in GEMM_FORMS.items():
        tiles = (M // 128) * (N // 128)
        got = "k_ldlt_trailing_64" if lower else ("k_gemm_nt_64" if tiles < 256 else "k_gemm_nt_128")
        assert got == name and M % 128 == 0 and N % 128 == 0 and (not lower or M == N)


@pytest.mark.parametrize("form", list(GEMM_FORMS))
@pytest.mark.parametrize("Kd", [16, 48, 896])
def test_gemm_entrywise_on_row_scaled_operands(lib, form, Kd):
    from cipkkt import _lib as L
    M, N, lower = GEMM_FORMS[form]
    rng = np.random.default_rng(M + N + Kd)
    A = rng.standard_normal((M, Kd)) * 10.0 ** rng.uniform(-6.0, 6.0, (M, 1))
    B = rng.standard_normal((N, Kd)) * 10.0 ** rng.uniform(-6.0, 6.0, (N, 1))
    C0 = rng.standard_normal((M, N)) * 10.0 ** rng.uniform(-6.0, 6.0, (M, 1))
    alpha = -0.75
    lda, ldb, ldc = M + 128, N + 256, M + 384
    dA, dB, dC = (torch.full((cols, ld), float("nan"), **F64) for cols, ld in ((Kd, lda), (Kd, ldb), (N, ldc)))
    dA[:, :M], dB[:, :N], dC[:, :M] = (torch.as_tensor(np.ascontiguousarray(X.T), **F64) for X in (A, B, C0))
    L.check(lib.cip_gemm_nt_dev(None, M, N, Kd, alpha, dA.data_ptr(), lda, dB.data_ptr(), ldb, dC.data_ptr(), ldc, lower))
    torch.cuda.synchronize()
    assert torch.isnan(dC[:, M:]).all()
    got = dC[:, :M].t().cpu().numpy()
    mag = torch.as_tensor(np.abs(C0), **F64) + abs(alpha) * (torch.as_tensor(np.abs(A), **F64) @ torch.as_tensor(np.abs(B), **F64).t())
    if Kd > 48:
        # every entry against an fp64 product on the device; that checker's own rounding, (2 K + 2) u mag, is added to the bound
        dref = torch.as_tensor(C0, **F64) + alpha * (torch.as_tensor(A, **F64) @ torch.as_tensor(B, **F64).t())
        derr = (dC[:, :M].t() - dref).abs()
        dbound = (GEMM_C * Kd + 2 * Kd + 2) * R.U * mag * (1.0 + 2 * Kd * R.U)
        if lower:
            keep = torch.ones(M, N, dtype=torch.bool, device="cuda").tril()
            derr, dbound = derr[keep], dbound[keep]
        assert bool((derr <= dbound).all()), (form, Kd, float((derr / dbound).max()))
        del dref, derr, dbound
    del mag
    rows = np.arange(M) if Kd <= 48 else R.sample_rows(M)               # long double: every row, or the row sample for the long K
    ref = C0[rows].astype(R.LD) + alpha * R._abt(A[rows].astype(R.LD), B.astype(R.LD))
    bound = GEMM_C * Kd * R.U * (np.abs(C0[rows]) + abs(alpha) * (np.abs(A[rows]) @ np.abs(B).T) * (1.0 + 2 * Kd * R.U))
    err = np.abs(got[rows].astype(R.LD) - ref)
    if lower:
        # the 128 x 128 tiles above the diagonal are left untouched (cipkkt.h); the lower triangle is what is promised
        above = (rows[:, None] // 128) < (np.arange(N)[None, :] // 128)
        assert np.array_equal(got[rows][above], C0[rows][above])
        tri = rows[:, None] >= np.arange(N)[None, :]
        err, bound = err[tri], bound[tri]
    print("GEMM | %s | K %d | max |err| / bound %.3g" % (form, Kd, float(np.max(err / bound))))
    assert np.all(err <= bound), (form, Kd, float(np.max(err / bound)))


@pytest.mark.parametrize("Kd", [16, 144])
def test_gemm_lower_and_rectangular_forms_share_one_tile_body(lib, Kd):
    """The rectangular quarter-tile form (k_gemm_nt_64, operands staged through registers) and the lower form (k_ldlt_trailing_64,
    operands global -> LDS directly) run the same 64 x 64 tile body from a zero accumulator in the same k order on the same LDS
    image: on equal inputs they agree bit for bit on every 64 x 64 tile with block row >= block column, and the lower form leaves
    the 128-tiles above the diagonal as they were."""
    from cipkkt import _lib as L
    M = N = 256
    rng = np.random.default_rng(4000 + Kd)
    A, B, C0 = (torch.as_tensor(rng.standard_normal(shape), **F64) for shape in ((Kd, M), (Kd, N), (N, M)))   # column-major M x Kd, N x Kd, M x N
    out = []
    for lower in (0, 1):
        dC = C0.clone()
        L.check(lib.cip_gemm_nt_dev(None, M, N, Kd, -0.75, A.data_ptr(), M, B.data_ptr(), N, dC.data_ptr(), M, lower))
        torch.cuda.synchronize()
        out.append(dC.t().cpu().numpy())                       # [row, column]
    rect, low = out
    C0h = C0.t().cpu().numpy()
    assert not np.array_equal(rect, C0h)
    for bi in range(M // 64):
        for bj in range(bi + 1):
            t = np.s_[64 * bi:64 * bi + 64, 64 * bj:64 * bj + 64]
            assert np.array_equal(low[t], rect[t]), (Kd, bi, bj)
    above = (np.arange(M)[:, None] // 128) < (np.arange(N)[None, :] // 128)
    assert np.array_equal(low[above], C0h[above])


# -------------------------------------------------------------------------------------------------------------- handles
def _hard_iterates(cone_dims, rng):
    """as tests/test_gpu_assembly.py: an interior pair whose Nesterov-Todd scaling has R entries over 1e-6 .. 1e6 and Q
    iterates with x0 - |x1| = 1e-6 x0"""
    vs, ss = [], []
    for t, k in cone_dims:
        if t == "R":
            e = rng.uniform(-6.0, 6.0, k)
            e[:min(k, 2)] = (-6.0, 6.0)[:min(k, 2)]
            vs.append(10.0 ** -e * (0.5 + rng.random(k)))
            ss.append(10.0 ** e * (0.5 + rng.random(k)))
            continue
        assert t == "Q"
        for out in (vs, ss):
            x = rng.standard_normal(k)
            x[0] = np.linalg.norm(x[1:]) / (1.0 - 1e-6) if k > 1 else 0.5 + rng.random()
            out.append(x)
    return np.concatenate(vs), np.concatenate(ss)


@pytest.mark.parametrize("name", list(R.HANDLES))
def test_handle_factor_and_solves_on_hard_scalings(lib, name):
    """cip_assemble_only -> K, cip_factor -> the factor of that K: the factor bound; then solve2x2 / solve3x3 against the
    downloaded K: the solve bound plus the factor bound times |x^|.  A row with side settings runs under each of them --
    solve preparation beside the last panels on the handle's side stream, and behind them -- and must give the same bits."""
    import cipkkt
    from cipkkt.workloads import c2_dense_qp
    from oracle.conicip import make_cone_ops
    route, akind, n, p, cone_dims, lazy, sides = R.HANDLES[name]
    rng = np.random.default_rng(sum(map(ord, name.replace("_eager", "").replace("_lazy", ""))))
    m = sum(k for _, k in cone_dims)
    if akind == "identity":
        Q = np.asarray(c2_dense_qp(n, 4000)[0])
        A = sp.identity(n, format="csr")
    else:
        M = rng.standard_normal((n, n))
        Q = M @ M.T / n + 0.5 * np.eye(n)
        A = rng.standard_normal((m, n))
        if akind == "csr":
            A = A * (rng.random((m, n)) < 0.15)
            A[np.arange(m), rng.integers(0, n, m)] = 1.0
            A = sp.csr_matrix(A)
    G = rng.standard_normal((p, n)) if p else None
    boxqp = akind == "identity" and all(t == "R" for t, _ in cone_dims)
    prev_lazy = lib.cip_set_lazy_copy(lazy) if lazy is not None else None
    prev_side = lib.cip_set_ldlt_side_prep(-1)
    ks = None
    try:
        ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route)
        Np = ks.Npad
        assert Np == R.handle_order(name) and (sides is not None) == R.side_prep_forks(Np)
        _, nt_scaling, _, _ = make_cone_ops(cone_dims)
        Fs = nt_scaling(*_hard_iterates(cone_dims, rng))
        packed = ks.pack_scaling(Fs, Fs.inv_adjoint())
        rhs_list = []
        for trial in range(2):
            x, y, z = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
            rhs_list.append((x * 10.0 ** rng.uniform(-3.0, 3.0, n) if trial else x, y, z))
        first = None
        for side in sides or (None,):
            tag = name if side is None else "%s side %d" % (name, side)
            if side is not None:
                lib.cip_set_ldlt_side_prep(side)
            ks.set_scaling_packed(packed)
            ks.assemble_only()
            K = np.tril(ks.kkt_matrix())
            K = K + np.tril(K, -1).T
            ks.factor()
            assert ks.health()["n_regularized"] == 0, "the hard scaling made the handle regularise: the factor is not K's"
            F = np.tril(ks.kkt_matrix())
            if first is None:
                _check_factor(name, K, F)
                Bs = R.dispatch(Np, 3, 0, 1024, 0)[1]
                sb = R.SolveBound(F, Bs, np.linalg.norm(K))
                Kq = K.astype(R.LD)
            else:
                assert np.array_equal(F.view(np.int64), first[0].view(np.int64)), "side preparation changed the factor"

            def judge(label, rhs, xh, more=0.0, report=True):
                rhs_p, x_p, more_p = np.zeros(Np, dtype=R.LD), np.zeros(Np), np.zeros(Np, dtype=R.LD)
                rhs_p[:ks.N], x_p[:ks.N] = rhs, xh
                more_p[:ks.N] = more
                _, yy = sb.residual(rhs_p, x_p)
                big, plain = sb.bounds(x_p, yy)
                bound = R.C_S["gemv"] * Np * R.U * big + R.factor_bound_times(F, np.abs(x_p)).astype(R.LD) + more_p
                sc = R._judge(rhs_p - Kq @ x_p.astype(R.LD), bound, plain, x_p, sb.knorm)
                if report:
                    _report("%s %s" % (tag, label), Np, Bs, "two launches per step", sc)
                assert sc["ok"], (tag, label, sc["ratio"])

            sols = []
            for x, y, z in rhs_list:
                if route == "schur":
                    dy, dw = ks.solve2x2(x, y)
                    judge("solve2x2", np.concatenate([x, y]), np.concatenate([dy, dw]))
                    sols += [dy, dw]
                    if boxqp:
                        # solve3x3 reduces to [x + A' (F'F)^-1 z; y]: with R cones and A = I that is x + z / d^2, formed here in
                        # long double; the device's own rounding of it -- the scaling of z, the product, the sum: at most 8
                        # roundings on |x| + |z| / d^2 -- is added to the bound
                        d = np.concatenate([np.asarray(b.diag, dtype=np.float64).reshape(-1) for b in Fs.Blocks]).astype(R.LD)
                        t = z.astype(R.LD) / (d * d)
                        a, b, c3 = ks.solve3x3(x, y, z)
                        judge("solve3x3", np.concatenate([x.astype(R.LD) + t, y.astype(R.LD)]), np.concatenate([a, b]),
                              more=np.concatenate([8.0 * R.U * (np.abs(x) + np.abs(t)), np.zeros(p)]))
                    else:
                        # with Q cones the reduced right-hand side passes through the hard scaling on the device and is not
                        # reproduced here: z = 0, where the LDL' solve sees (x, y) itself (the 3x3 path's plumbing; not a table row)
                        a, b, c3 = ks.solve3x3(x, y, np.zeros(m))
                        judge("solve3x3 z=0", np.concatenate([x, y]), np.concatenate([a, b]), report=False)
                    sols += [a, b, c3]
                else:
                    a, b, c3 = ks.solve3x3(x, y, z)                     # [-F'F -A 0; -A' Q G'; 0 G 0] [c; a; b] = [-z; x; y]
                    judge("solve3x3", np.concatenate([-z, x, y]), np.concatenate([c3, a, b]))
                    sols += [a, b, c3]
            if first is None:
                first = (F, sols)
            else:
                # cipkkt.h, cip_set_ldlt_side_prep: "Same bits"
                for u0, u1 in zip(first[1], sols):
                    assert np.array_equal(u0.view(np.int64), u1.view(np.int64)), "side preparation changed a solve"
        assert ks.health()["n_regularized"] == 0
    finally:
        if ks is not None:
            ks.close()
        lib.cip_set_ldlt_side_prep(prev_side)
        if prev_lazy is not None:
            lib.cip_set_lazy_copy(prev_lazy)
