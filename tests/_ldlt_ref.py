"""Graded quasi-definite matrices, entrywise rounding bounds and an fp64 model for the blocked LDL' (csrc/ldlt.hip,
csrc/diag.hip, the trailing update of csrc/gemm_f64.hip) and the triangular sweeps built on stored block inverses
(build_solve_blocks, cip_ldlt_solve, k_solve_step, csrc/solve_many.hip).  No GPU here; tests/test_ldlt_ref.py checks
this module, tests/test_gpu_ldlt_hard.py applies it to the device.

Notation.  u = 2^-53, gamma_c = c u / (1 - c u).  L^, D^ are a computed factor (unit lower, diagonal), x^ a computed
solution.  Extended precision is numpy.longdouble (64-bit significand): its own rounding, 2^-11 u per operation, is
below every bound here by a factor 2000 and is not accounted for.

Matrix families (seeded numpy, in the library's static pivot order, padded with an identity to a multiple of 128;
quasi-definite by construction, so the LDL' exists without pivoting)
  benign           M M'/n + I with a G border                            the suite's baseline: |L| <= 1, pivots within 3 decades
  schur_graded     [[Q + A'WA, G'], [G, 0]], Q = M M'/n, A n/2 dense rows, W = diag(10^U(0, 2 spread))
  full3x3_graded   [[-W, -A, 0], [-A', Q, G'], [0, G, 0]], W = diag(10^U(-spread, spread)), A 20 % dense
  regularised      schur_graded(spread 3) whose last equality row repeats the first; every row gets the library's
                   static regularisation K_ii + s_i rel max_j |K_ij| (cipkkt.h: cip_set_regularization), which turns the
                   repeated row's zero pivot into one of about -2 rel rowmax

Factor bound (factor_check).  Entry (i, j), i >= j, of K is reproduced by sum_{k <= j} l_ik d_k l_jk.  Whatever the
blocking, every term of that sum is one rounded product w_ik = l_ik d_k and one fused multiply-add, the terms and the
partial sums of panels, in-block updates and trailing updates are added in some order (at most j additions of terms and
at most j merges of partial sums), the multiplier is one more product with the reciprocal rho_j, and the stored pivot
d_j = fl(1 / rho_j) differs from the reciprocal that was used by at most 12 u (diag.hip: one Newton step on the chain,
the stored pivot defined from it).  That is at most 2 N + 16 rounding errors, each relative to a term of
B = |L^| |D^| |L^|', so with N >= 128
    |K - L^ D^ L^'|_ij <= gamma_(2N + 16) B_ij <= C_F N u B_ij,   C_F = 3                        (textbook, Higham 10.3 form)
One step is not of that form.  Below a 16 x 16 diagonal micro-block with unit-lower factor L11 the panel is not
obtained by substitution but by a product with the explicit inverse X^ of L11 (diag.hip step B, k_trsm_subst, the
strips of k_ldlt_panel): w^ = fl(v X^'), v the updated row of the panel.  X^ comes from forward elimination on the
identity, whose residual is |L11 X^ - I| <= gamma_16 |L11| |X^|, and the product adds |dw| <= gamma_16 |v| |X^|'.  Hence
    |w^ L11' - v| <= 2 gamma_16 |v| (|L11| |X^|)',     |v| <= |w^| |L11|' (1 + O(u)),   w^ = l^ d
and the rows i below micro-block J carry the extra term
    34 u (|L^_iJ| |D^_J| |L11_J|') (|L11_J| |inv(L11_J)|)'                                       (34 = 2 * 17: gamma_16 and the O(u))
with the inverse formed in extended precision.  It vanishes from the textbook bound only while |L11||inv(L11)| is of
order one; on a graded matrix it is the larger part.

Solve bound (solve_check).  With t = L^' x^, y = D^ t, r = b - L^ y in extended precision (the residual against the
factor: the factor's own error is judged by factor_check) and P block diagonal with blocks |inv(L_JJ)| |L_JJ| of the
solve block Bs in force,
    |r| <= C_S N u ( |L^| P |y| + |L^| |D^| |L^'| P' |x^| ).
A block step forms y_J = X^_J (b_J - sum_{I<J} L_JI y_I).  With R_J = X^_J L_JJ - I the left residual of the stored
inverse, L_JJ y^_J - (b_J - ...) = L_JJ (R_J y_J + dy), |dy| <= gamma_Bs |X^_J| |L_JJ| |y_J|: both are of the form
|L_JJ| (c u P_J) |y_J| as long as |R_J| <= c u |X^_J| |L_JJ|; the update of the rows below adds gamma |L^| |y| <= gamma
|L^| P |y| (P >= I entrywise).  The backward sweep is the mirror image, carried to r through L^ D^.  The constant counts
the rounding errors on the longest path behind one entry, in units of N (Bs <= N, N >= 128):
    updates of the rows below / above    at most N terms and N merges of partial sums                     2 N
    product with the block inverse       Bs terms                                                           N
    the block inverse itself             16 (micro) + 128 (block rows) + 2 (Bs - 128) (doubling levels)   2 N
    1 / d, the stored d against it, the final subtraction                                                 < N / 8
  two launches per step (cip_gemv_t)   C_S = 6
  many columns (k_gemm_tn)             C_S = 6   (the same sums, cut into wave partials: merges, already counted)
  one launch per step (k_solve_step)   C_S = 8   (the neighbour block X_J L_(J,J-1) is a product of length Bs formed at
                                                  factorisation time and applied with another Bs terms)
What is derived and what is not.  The argument above is a proof only under its hypothesis |R_J| <= c u |X^_J||L_JJ|, which
holds for inverses obtained by substitution.  The doubling X21 = -X22 L21 X11 gives a residual bounded by products
P_(level) P_(level below) instead, and the pre-multiplied neighbours of k_solve_step put |L_JJ||X_J| on the other side of
L_(J,J-1): a term |L_JJ||X_J||L_(J,J-1)||y_(J-1)| that no expression of the form |L| P |y| covers.  For the doubled
inverses, and for the one-launch form altogether, the assertion is therefore HEURISTIC: the form of the bound is the
one-P form, the constants are counts of operations, and the factor N is all there is to absorb the missing P.  It
catches a wrong term, a short sum or a wrong block (errors of the order of the solution), not a loss of a few digits;
the figure that shows such a loss is the ratio to the plain substitution bound u |L^||D^||L^'||x^|, which solve_check
returns and the tests record without asserting it.

The model (model_factor, model_solve) is the algorithm as it ships in plain fp64 numpy: 16-wide micro blocks with
explicit micro inverses, 128-wide panels, outer blocks with one trailing update each, solves by block inverses of width
Bs built by doubling.  It shows that an independent implementation meets the bounds; it is never compared bit for bit.
"""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
C_F = 3
C_S = {"gemv": 6, "many": 6, "fused": 8}
MICRO, NB = 16, 128
REG_AUTO = 1e-13                       # the library's automatic static regularisation (include/cipkkt.h)

Case = namedtuple("Case", "name K N pos")      # K: padded, full symmetric; N: order before padding; pos: [p0, p1) positive pivots


def _pad(K):
    N = K.shape[0]
    Np = -(-N // NB) * NB
    out = np.zeros((Np, Np))
    out[:N, :N] = K
    out[np.arange(N, Np), np.arange(N, Np)] = 1.0
    return out


def expected_signs(case):
    s = -np.ones(case.K.shape[0])
    s[case.pos[0]:case.pos[1]] = 1.0
    s[case.N:] = 1.0
    return s


def _gram_scaled(M, n, mm):
    return mm(M, M.T) / n


def benign(N, quasi=0, seed=0, mm=np.matmul):
    rng = np.random.default_rng([seed, N, quasi])
    M = rng.standard_normal((N, N))
    K = _gram_scaled(M, N, mm) + np.eye(N)
    if quasi:
        K[N - quasi:, N - quasi:] = 0.0
    return Case("benign(%d,%d)" % (N, quasi), _pad(0.5 * (K + K.T)), N, (0, N - quasi))


def schur_graded(n, p, spread, seed=0, mm=np.matmul):
    rng = np.random.default_rng([seed, n, p, spread])
    M = rng.standard_normal((n, n))
    A = rng.standard_normal((n // 2, n))
    w = 10.0 ** rng.uniform(0.0, 2.0 * spread, n // 2)
    S = _gram_scaled(M, n, mm) + mm(A.T * w, A)
    K = np.zeros((n + p, n + p))
    K[:n, :n] = 0.5 * (S + S.T)
    G = rng.standard_normal((p, n))
    K[n:, :n] = G
    K[:n, n:] = G.T
    return Case("schur_graded(%d,%d,%d)" % (n, p, spread), _pad(K), n + p, (0, n))


def full3x3_graded(m, n, p, spread, seed=0, mm=np.matmul):
    rng = np.random.default_rng([seed, m, n, p, spread])
    M = rng.standard_normal((n, n))
    Q = _gram_scaled(M, n, mm)
    A = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.2)
    w = 10.0 ** rng.uniform(-spread, spread, m)
    w[:2] = 10.0 ** -spread, 10.0 ** spread
    G = rng.standard_normal((p, n))
    N = m + n + p
    K = np.zeros((N, N))
    K[np.arange(m), np.arange(m)] = -w
    K[m:m + n, :m] = -A.T
    K[:m, m:m + n] = -A
    K[m:m + n, m:m + n] = 0.5 * (Q + Q.T)
    K[m + n:, m:m + n] = G
    K[m:m + n, m + n:] = G.T
    return Case("full3x3_graded(%d,%d,%d,%d)" % (m, n, p, spread), _pad(K), N, (m, m + n))


def regularised(n, p, rel=REG_AUTO, seed=0, mm=np.matmul):
    base = schur_graded(n, p, 3, seed=seed, mm=mm)
    K = base.K.copy()
    N = n + p
    K[N - 1, :n] = K[n, :n]                        # the last equality row repeats the first: an exactly singular matrix
    K[:n, N - 1] = K[n, :n]
    rowmax = np.abs(K[:N, :N]).max(axis=1)
    i = np.arange(N)
    K[i, i] += np.where(i < n, 1.0, -1.0) * rel * rowmax
    return Case("regularised(%d,%d,%g)" % (n, p, rel), K, N, (0, n))


# ------------------------------------------------------------------------------------------------ extended precision
def _abt(A, B):
    """A B' (rows of both contiguous: the fast orientation of numpy's long-double loops)"""
    return np.einsum("ik,jk->ij", A, B)


def unit_lower_inverse(Lb):
    """inverse of a stack (nb, b, b) of unit-lower blocks (diagonal taken as 1, upper part ignored), in the dtype of Lb:
    forward substitution on 16 x 16 blocks, then doubling inv([A 0; C B]) = [Ai 0; -Bi C Ai, Bi]"""
    nb, b, _ = Lb.shape
    X = np.zeros_like(Lb)
    h = min(b, MICRO)
    for o in range(0, b, h):
        T = Lb[:, o:o + h, o:o + h]
        Xo = np.zeros((nb, h, h), dtype=Lb.dtype)
        for i in range(h):
            Xo[:, i, i] = 1.0
            if i:
                Xo[:, i, :i] = -np.einsum("bk,bkj->bj", T[:, i, :i], Xo[:, :i, :i])
        X[:, o:o + h, o:o + h] = Xo
    while h < b:
        for o in range(0, b, 2 * h):
            A = X[:, o:o + h, o:o + h]
            B = X[:, o + h:o + 2 * h, o + h:o + 2 * h]
            Cm = Lb[:, o + h:o + 2 * h, o:o + h]
            T = np.einsum("bik,bjk->bij", Cm, np.ascontiguousarray(np.swapaxes(A, 1, 2)))       # C Ai
            X[:, o + h:o + 2 * h, o:o + h] = -np.einsum("bik,bjk->bij", B, np.ascontiguousarray(np.swapaxes(T, 1, 2)))
        h *= 2
    return X


def split_factor(F):
    """(L unit lower, d) of a factor stored as the device stores it: L strictly below the diagonal, D on it"""
    F = np.asarray(F)
    L = np.tril(F, -1)
    L[np.arange(F.shape[0]), np.arange(F.shape[0])] = 1.0
    return L, np.diag(F).copy()


def _diag_blocks(L, b):
    N = L.shape[0]
    return np.stack([L[o:o + b, o:o + b] for o in range(0, N, b)])


def sample_rows(N):
    """the fixed row sample of the long-double factor check above order 1024: the first and the last row of every 64-row
    band and the whole last 128-block"""
    r = set(range(N - NB, N))
    for o in range(0, N, 64):
        r.update((o, o + 63))
    return np.array(sorted(r))


def factor_check(K, F, c_f=C_F, rows=None, threads=8, wide_B=True):
    """The factor bound on the lower triangle (all rows, or the given sorted rows).  Returns a dict: ok, ratio = max
    |E| / bound, textbook = max |E| / (u B) (the scale to expect: a few units), micro = the largest entry of
    |L11||inv(L11)| over the 16 x 16 micro-blocks, at = (i, j) of the worst ratio.  wide_B False forms B in fp64 (a sum of
    non-negative terms: relative error below gamma_N, which the bound is inflated by)."""
    K = np.asarray(K)
    N = K.shape[0]
    L, d = split_factor(F)
    rows = np.arange(N) if rows is None else np.asarray(rows)
    Lq, dq = L.astype(LD), d.astype(LD)
    La, da = np.abs(L), np.abs(d)
    Laq = La.astype(LD) if wide_B else La
    daq = da.astype(LD) if wide_B else da
    Mx, pmax = micro_matrices(L)                                                    # |L11|' (|L11||inv(L11)|)'
    groups = [rows[(rows >= o) & (rows < o + NB)] for o in range(0, N, NB)]
    groups = [g for g in groups if len(g)]

    def one(g):
        r1 = int(g[-1]) + 1
        r16 = -(-r1 // MICRO) * MICRO
        E = K[g, :r1].astype(LD) - _abt(Lq[g, :r1] * dq[:r1], Lq[:r1, :r1])
        B = _abt(Laq[g, :r1] * daq[:r1], Laq[:r1, :r1]).astype(LD)
        if not wide_B:
            B = B * (1.0 + 2.0 * N * U)
        Gm = (np.abs(Lq[g, :r16]) * np.abs(dq[:r16])).reshape(len(g), r16 // MICRO, MICRO)
        X = np.einsum("rbk,bkj->rbj", Gm, Mx[:r16 // MICRO])
        below = g[:, None] >= (np.arange(r16 // MICRO)[None, :] + 1) * MICRO       # rows under the micro-block only
        X = (X * below[:, :, None]).reshape(len(g), r16)[:, :r1]
        bound = c_f * N * U * B + 34.0 * U * X
        low = np.arange(r1)[None, :] <= g[:, None]
        E = np.abs(E)
        bad = low & ~(E <= bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(low & (bound > 0), E / np.where(bound > 0, bound, 1), np.where(low & (E > 0), np.inf, 0.0))
            text = np.where(low & (B > 0), E / (U * np.where(B > 0, B, 1)), 0.0)
        k = int(np.argmax(ratio))
        return bool(bad.any()), float(ratio.flat[k]), (int(g[k // r1]), k % r1), float(text.max())

    with ThreadPoolExecutor(max_workers=threads) as ex:
        res = list(ex.map(one, groups))
    worst = max(res, key=lambda t: t[1])
    return dict(ok=not any(t[0] for t in res), ratio=worst[1], at=worst[2], textbook=max(t[3] for t in res),
                micro=pmax)


def micro_matrices(L):
    """(Mx, pmax): Mx[J] = |L11_J|' (|L11_J| |inv(L11_J)|)' of every 16 x 16 diagonal micro-block, inverse in extended
    precision, rounded to fp64; pmax the largest entry of |L11||inv(L11)|"""
    L16 = _diag_blocks(np.asarray(L).astype(LD), MICRO)
    Pm = np.einsum("bik,bkj->bij", np.abs(L16), np.abs(unit_lower_inverse(L16)))
    return np.einsum("bki,bjk->bij", np.abs(L16), Pm).astype(np.float64), float(Pm.max())


def factor_bound_times(F, xabs, c_f=C_F):
    """(bound matrix of factor_check, symmetrised) |x|, formed in fp64 and inflated by its own rounding: what an error of
    the factor within its bound can add to a residual against K"""
    L, d = split_factor(F)
    N = L.shape[0]
    La, da = np.abs(L), np.abs(d)
    Mx, _ = micro_matrices(L)
    G = (La * da).reshape(N, N // MICRO, MICRO)
    X = np.einsum("rbk,bkj->rbj", G, Mx)
    X *= (np.arange(N)[:, None] >= (np.arange(N // MICRO)[None, :] + 1) * MICRO)[:, :, None]
    X = X.reshape(N, N)
    low = c_f * N * U * np.tril((La * da) @ La.T) + 34.0 * U * np.tril(X)
    full = low + np.tril(low, -1).T
    return (full @ np.asarray(xabs, dtype=np.float64)) * (1.0 + 4.0 * N * U)


class SolveBound:
    """The solve bound for one factor and one solve block Bs; check(b, x, c_s) judges one right-hand side."""

    def __init__(self, F, Bs, knorm=None):
        L, d = split_factor(F)
        self.N, self.Bs, self.knorm = L.shape[0], Bs, knorm
        self.Lq, self.dq = L.astype(LD), d.astype(LD)
        self.Lt = np.ascontiguousarray(self.Lq.T)
        self.La, self.Lta, self.da = np.abs(self.Lq), np.abs(self.Lt), np.abs(self.dq)
        self.Xa = np.abs(unit_lower_inverse(_diag_blocks(self.Lq, Bs)))             # (nbk, Bs, Bs)
        self.Ld = _diag_blocks(self.La, Bs)

    def _P(self, v):                                                                # P v = |X| (|L_JJ| v)
        v = v.reshape(-1, self.Bs)
        return np.einsum("bij,bj->bi", self.Xa, np.einsum("bij,bj->bi", self.Ld, v)).reshape(-1)

    def _Pt(self, v):                                                               # P' v = |L_JJ|' (|X|' v)
        v = v.reshape(-1, self.Bs)
        return np.einsum("bji,bj->bi", self.Ld, np.einsum("bji,bj->bi", self.Xa, v)).reshape(-1)

    def residual(self, b, x):
        """(r, y): r = b - L^ (D^ (L^' x)) in extended precision"""
        y = self.dq * (self.Lt @ np.asarray(x).astype(LD))
        return np.asarray(b).astype(LD) - self.Lq @ y, y

    def bounds(self, x, y):
        """(bound / (c_s N u), plain): the two magnitudes of the module docstring"""
        xa = np.abs(np.asarray(x).astype(LD))
        big = self.La @ self._P(np.abs(y)) + self.La @ (self.da * (self.Lta @ self._Pt(xa)))
        return big, U * (self.La @ (self.da * (self.Lta @ xa)))

    def check(self, b, x, c_s, more=None):
        """dict: ok, ratio = max |r| / bound, plain = max |r| / (u |L^||D^||L^'||x^|) (recorded, not asserted), nbe = |r|_2 /
        (|K|_F |x^|_2) when knorm was given, bound (fp64).  more: a vector added to the bound."""
        r, y = self.residual(b, x)
        big, plain = self.bounds(x, y)
        bound = c_s * self.N * U * big
        if more is not None:
            bound = bound + np.asarray(more).astype(LD)
        return _judge(r, bound, plain, x, self.knorm)


def _judge(r, bound, plain, x, knorm):
    ra = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(bound > 0, ra / np.where(bound > 0, bound, 1), np.where(ra > 0, np.inf, 0.0))))
        pl = float(np.max(np.where(plain > 0, ra / np.where(plain > 0, plain, 1), 0.0)))
    out = dict(ok=bool(np.all(ra <= bound)) and bool(np.all(np.isfinite(np.asarray(x, dtype=np.float64)))), ratio=ratio,
               plain=pl, bound=bound.astype(np.float64), r=r.astype(np.float64))
    if knorm is not None:
        out["nbe"] = float(np.linalg.norm(out["r"]) / (knorm * np.linalg.norm(np.asarray(x, dtype=np.float64))))
    return out


def solve_check(F, b, x, Bs, c_s, knorm=None):
    return SolveBound(F, Bs, knorm).check(b, x, c_s)


# ---------------------------------------------------------------------------------------------------- the fp64 model
def outer_widths(N, nbo):
    return [min(nbo, N - c) for c in range(0, N, nbo)]


def model_factor(K, widths=None):
    """(F, rho, Xm, info): the blocked LDL' as it ships, fp64.  F holds L below the diagonal and D on it, rho the
    reciprocals the multipliers were formed with, Xm the 16 x 16 micro inverses, info the first zero / non-finite pivot
    (1-based; 0: none).  widths: the outer blocks (default: 512 wide)."""
    A = np.array(K, dtype=np.float64)
    N = A.shape[0]
    widths = outer_widths(N, 512) if widths is None else list(widths)
    assert sum(widths) == N and all(w % NB == 0 for w in widths)
    rho = np.zeros(N)
    Xm = np.zeros((N // MICRO, MICRO, MICRO))
    info = 0
    C0 = 0
    with np.errstate(all="ignore"):
        for w in widths:
            Wb = np.zeros((N, w))
            for c0 in range(C0, C0 + w, NB):
                e = c0 + NB
                for c in range(c0, e, MICRO):
                    T = A[c:c + MICRO, c:c + MICRO]
                    X = np.eye(MICRO)
                    for j in range(MICRO):
                        r = 1.0 / T[j, j]
                        dj = 1.0 / r                                       # the stored pivot is defined from the reciprocal
                        if info == 0 and not (abs(dj) > 0.0 and abs(dj) < 1.7e308):
                            info = c + j + 1
                        rho[c + j] = r
                        uj = T[j + 1:, j].copy()
                        lj = uj * r
                        T[j + 1:, j + 1:] -= np.outer(uj, lj)
                        T[j + 1:, j] = lj
                        T[j, j] = dj
                        X[j + 1:, :] -= np.outer(lj, X[j, :])
                    Xm[c // MICRO] = X
                    if c + MICRO < N:
                        Wm = A[c + MICRO:, c:c + MICRO] @ X.T              # W = U inv(L11)'
                        Lr = Wm * rho[c:c + MICRO]
                        A[c + MICRO:, c:c + MICRO] = Lr
                        Wb[c + MICRO:, c - C0:c - C0 + MICRO] = Wm
                        if c + MICRO < e:
                            A[c + MICRO:, c + MICRO:e] -= Wm @ Lr[:e - c - MICRO].T
                e2 = C0 + w
                if e < e2:                                                 # the rest of the outer block's panel columns
                    A[e:, e:e2] -= Wb[e:, c0 - C0:e - C0] @ A[e:e2, c0:e].T
            r0 = C0 + w
            if r0 < N:                                                     # ONE trailing update per outer block
                A[r0:, r0:] -= Wb[r0:, :] @ A[r0:, C0:r0].T
            C0 = r0
    return np.tril(A), rho, Xm, info


def model_block_inverses(F, Xm, Bs):
    """inverses of the Bs-wide unit-lower diagonal blocks by doubling from the micro inverses, fp64"""
    N = F.shape[0]
    L = np.tril(F, -1)
    X = np.zeros((N // Bs, Bs, Bs))
    for J in range(N // Bs):
        o = J * Bs
        XJ = X[J]
        for q in range(Bs // MICRO):
            XJ[q * MICRO:(q + 1) * MICRO, q * MICRO:(q + 1) * MICRO] = Xm[o // MICRO + q]
        h = MICRO
        while h < Bs:
            for a in range(0, Bs, 2 * h):
                Tt = XJ[a:a + h, a:a + h].T @ L[o + a + h:o + a + 2 * h, o + a:o + a + h].T     # Tt = X11' L21'
                XJ[a + h:a + 2 * h, a:a + h] = -XJ[a + h:a + 2 * h, a + h:a + 2 * h] @ Tt.T    # X21 = -X22 Tt'
            h *= 2
    return X


def model_solve(F, rho, X, b):
    """both sweeps with the block inverses X (nbk, Bs, Bs), two products per block step as cip_ldlt_solve, fp64"""
    N = F.shape[0]
    Bs = X.shape[1]
    L = np.tril(F, -1)
    rhs = np.array(b, dtype=np.float64)
    y = np.zeros(N)
    for J in range(N // Bs):
        o = J * Bs
        y[o:o + Bs] = X[J] @ rhs[o:o + Bs]
        rhs[o + Bs:] -= L[o + Bs:, o:o + Bs] @ y[o:o + Bs]
    z = y * rho
    x = np.zeros(N)
    for J in range(N // Bs - 1, -1, -1):
        o = J * Bs
        x[o:o + Bs] = X[J].T @ z[o:o + Bs]
        z[:o] -= L[o:o + Bs, :o].T @ x[o:o + Bs]
    return x


# ------------------------------------------------------------------------------- the table of tests/test_gpu_ldlt_hard.py
FAMILIES = {"benign": benign, "schur_graded": schur_graded, "full3x3_graded": full3x3_graded, "regularised": regularised}

# name -> family, its arguments, and the knobs the case runs under.  chain: cip_set_ldlt_fused_chain; nbo:
# cip_set_ldlt_outer_block (0 automatic); bs: cip_set_solve_block_max; fused: cip_set_solve_fused; pad: ld - N; many: the
# column counts of cip_ldlt_solve_many_dev; solve False:
# the factor only.  "expect" restates what the dispatch rules make of the knobs at this order -- (outer-block widths,
# solve block, one-launch block steps) -- and is checked against dispatch() below, which restates the rules themselves.
GPU_CASES = {
    # one outer block, no trailing update; 384 = 3 x 128: only the 128-wide solve block divides it
    "benign_384": dict(fam="benign", args=(384, 38), chain=0, nbo=0, bs=1024, fused=0, expect=([384], 128, False)),
    # four outer blocks with K = 128 trailing updates; ONE solve block over the positive and the equality part (448 | 64)
    "schur3_512_nbo128": dict(fam="schur_graded", args=(448, 64, 3), chain=3, nbo=128, bs=512, fused=0,
                              expect=([128] * 4, 512, False)),
    # trailing update K = 512 then a 256 block; solve block 256, the boundary 704 inside the last one; one-launch steps
    "schur6_768_bs256_fused": dict(fam="schur_graded", args=(704, 64, 6), chain=0, nbo=512, bs=256, fused=2,
                                   many=(1, 3, 64, 100), expect=([512, 256], 256, True)),
    # ld > N; boundaries 256 (on a solve-block edge) and 640 (inside one); two launches per step; k_gemm_tn with 4 waves
    "full6_768_bs256_ld": dict(fam="full3x3_graded", args=(256, 384, 128, 6), chain=3, nbo=512, bs=256, fused=0, pad=128,
                               many=(3,), expect=([512, 256], 256, False)),
    "full3_768_bs128_fused": dict(fam="full3x3_graded", args=(300, 400, 68, 3), chain=0, nbo=0, bs=128, fused=2,
                                  expect=([512, 256], 128, True)),
    # ONE 1024-wide solve block over both parts: fused mode 2 has nothing to fuse with a single block
    "schur6_1024_bs1024": dict(fam="schur_graded", args=(896, 128, 6), chain=3, nbo=512, bs=1024, fused=2,
                               expect=([512, 512], 1024, False)),
    # outer block 1024: a K = 1024 trailing update in front of the last 128 columns; 1152 = 9 x 128
    "schur3_1152_nbo1024": dict(fam="schur_graded", args=(1024, 128, 3), chain=3, nbo=1024, bs=1024, fused=2,
                                expect=([1024, 128], 128, True)),
    # solve block 512: boundaries 512 (edge) and 1280 (inside the last block); widths 1024 | 512; both sweep forms on one factor
    "full6_1536_bs512": dict(fam="full3x3_graded", args=(512, 768, 256, 6), chain=0, nbo=1024, bs=512, fused=0,
                             expect=([1024, 512], 512, False)),
    "full6_1536_bs512_fused": dict(fam="full3x3_graded", args=(512, 768, 256, 6), chain=0, nbo=1024, bs=512, fused=2,
                                   many=(64,), expect=([1024, 512], 512, True)),
    # two 1024-wide solve blocks (k_gemm_tn with 8 waves: Kr >= 512), both boundaries inside a block; both sweep forms
    "full3_2048_bs1024": dict(fam="full3x3_graded", args=(768, 1024, 256, 3), chain=3, nbo=0, bs=1024, fused=0,
                              many=(1, 3, 64, 100), expect=([512] * 4, 1024, False)),
    "full3_2048_bs1024_fused": dict(fam="full3x3_graded", args=(768, 1024, 256, 3), chain=3, nbo=0, bs=1024, fused=2,
                                    expect=([512] * 4, 1024, True)),
    "reg_512_auto": dict(fam="regularised", args=(448, 64, REG_AUTO), chain=3, nbo=0, bs=1024, fused=0,
                         expect=([512], 512, False)),
    "reg_512_1e-8": dict(fam="regularised", args=(448, 64, 1e-8), chain=0, nbo=0, bs=1024, fused=0,
                         expect=([512], 512, False)),
    # the automatic width from order 4096 on: 896, 896, then the wide last block (2816 columns left <= the tail limit);
    # solve block 512 with the boundaries 2560 and 4096 on block edges.  (The stand-alone entry has no side stream: the solve
    # preparation beside the last panels is reached by the handle row boxqp_4608_side below.)
    "full6_4608_auto": dict(fam="full3x3_graded", args=(2560, 1536, 512, 6), chain=3, nbo=0, bs=1024, fused=0,
                            expect=([896, 896, 2816], 512, False)),
    # six 896-wide blocks with a trailing update each in front of the wide last block
    "full3_8192_auto": dict(fam="full3x3_graded", args=(4096, 3584, 512, 3), chain=3, nbo=0, bs=1024, fused=0, solve=False,
                            expect=([896] * 6 + [2816], 1024, False)),
}


def build_case(name, mm=np.matmul):
    c = GPU_CASES[name]
    return FAMILIES[c["fam"]](*c["args"], mm=mm)


def dispatch(N, chain, nbo, bs_max, fused):
    """(outer-block widths, solve block, one-launch block steps): the rules of ldlt.hip at their defaults, restated
    independently (tests/test_ldlt_plan.py compares the widths with the library's own plan) --
    cip_ldlt_plan.h: ldlt_outer_block / width_at (automatic: 896 from order 4096 on with the fused chain, else 512; the
    last block takes what is left once that is at most 2816 columns, automatic widths of 640 and more only),
    cip_solve_block (the largest of 1024 .. 128 within the limit that divides N) and solve_fused_for"""
    width = nbo if nbo else (896 if (N >= 4096 and chain) else 512)
    widths, c = [], 0
    while c < N:
        left = N - c
        w = left if (nbo == 0 and width >= 640 and left <= 2816) else min(left, width)
        widths.append(w)
        c += w
    Bs = next(b for b in (1024, 512, 256, 128) if b <= max(bs_max, 128) and N % b == 0)
    return widths, Bs, bool(N // Bs >= 2 and (fused == 2 or (fused == 1 and Bs <= 512)))


# Handles (KKTSystem) with hard Nesterov-Todd scalings: name -> (route, A, n, p, cone_dims, lazy copy, side).  side: the
# cip_set_ldlt_side_prep settings the row is factored and solved under, bits compared between them.  Only a handle owns a side
# stream, and the preparation forks only in a wide last block (side_prep_forks below): order >= 4096 on the default chain.
HANDLES = {
    "schur_dense": ("schur", "dense", 700, 20, [("R", 400), ("Q", 60), ("Q", 5), ("R", 200)], None, None),   # order 720 -> 768, Bs 256
    "schur_csr": ("schur", "csr", 380, 4, [("R", 300), ("Q", 30), ("R", 50)], None, None),                  # order 384, Bs 128
    "boxqp_2048_lazy": ("schur", "identity", 2048, 0, [("R", 2048)], 1, None),                              # EPI_LAZYC trailing update
    "boxqp_2048_eager": ("schur", "identity", 2048, 0, [("R", 2048)], 0, None),
    "boxqp_4608_side": ("schur", "identity", 4608, 0, [("R", 4608)], None, (1, 0)),                         # 896 | 896 | 2816, Bs 512
    "full3x3": ("full3x3", "dense", 256, 5, [("R", 100), ("Q", 120), ("Q", 3), ("R", 60)], None, None),     # order 544 -> 640, Bs 128
}


def handle_order(name):
    route, _, n, p, cone_dims, _, _ = HANDLES[name]
    N = n + p + (sum(k for _, k in cone_dims) if route == "full3x3" else 0)
    return -(-N // NB) * NB


def side_prep_forks(Npad):
    """does a handle's factorisation of this order prepare solve blocks on the side stream (cip_ldlt_plan.h: ldlt_plan, at the
    defaults: fused chain, automatic outer block, solve-block limit 1024)?  The last outer block must be at least two automatic
    widths wide and wider than the solve block, the solve block wider than 128, and there must be two solve blocks."""
    widths, Bs, _ = dispatch(Npad, 3, 0, 1024, 0)
    auto = 896 if Npad >= 4096 else 512
    return Bs > NB and Npad // Bs >= 2 and widths[-1] >= 2 * auto and widths[-1] > Bs
