"""Reference KKT matrices for entrywise parity tests of the device assembly (csrc/assemble.hip).

``reference(Q, A, G, cone_dims, F, route, Npad)`` returns ``(K, copied, bound)``, three Npad x Npad arrays laid out
as the device's K: the Schur route ``[Q + A'(F'F)^-1 A, G'; G, 0]`` or the full 3x3 route in the device's symmetrised
(v, y, w) order ``[-F'F, -A, 0; -A', Q, G'; 0, G, 0]``, padded with an identity.  Only the lower triangle is meant.

``copied`` marks the entries the kernels only copy or negate (Q and G, -A', zeros, the padding identity): they must
come back bit-identical, signed zeros included (a dense A's zeros negate to -0.0, a CSR A leaves +0.0 off its pattern).  Every other entry of the lower triangle is computed, and ``|K_dev - K| <= bound`` there.

Bound.  Write u for the unit roundoff and gamma_c = c u / (1 - c u).  A dot product of length c computed in any order
(sequential, blocked, split-K slices added afterwards, MFMA partial sums) satisfies |fl(x'y) - x'y| <= gamma_c |x|'|y|.

* Schur block.  K = Q + W'W with W = F^-T A.  W is computed per row r of A (one cone at a time) with an error
  |dW_ri| <= gamma_cw What_ri, where What is the magnitude of the terms W is formed of and cw the number of operations
  behind one entry of W (2 for an R cone, k + 4 for a Q cone of dimension k, 2 r + 4 for an S cone of order r).
  Then |fl(Q + W'W) - (Q + W'W)| <= gamma_(m+1) (|Q| + |W|'|W|) + 2 gamma_cw What'What (first order), and What >= |W|.
  The reference carries an error of the same bound, so device and reference differ by at most
  2 (m + 1 + 2 cw) u (|Q| + What'What), with m the reduction length (the padded row count of A).
  - R cone: W_r = a_r / d_r, What_r = |a_r| / d_r.
  - Q cone, F = diag(-beta, beta, ..) + w w'.  Its rows cancel, so What is not |W|:
    t = (w_0 a_0 - sum_e w_e a_e) / beta, W_0 = (w_0 t - a_0) / beta, W_e = (a_e - w_e t) / beta, and
    What_e = (|a_e| + |w_e| that) / beta with that = sum_e |w_e| |a_e| / beta.
  - S cone: W = vecm(Ri mat(a) Ri') with Ri = R^-1 as packed, What = vecm(|Ri| |mat(a)| |Ri|').
  For a CSR A the device splits (F'F)^-1 of a Q cone into J / beta^2 row weights and a rank-one column
  Gm_i = sqrt2 / beta sum_e (J wbar)_e a_ei (k_schur_rows, k_schur_qcols).  Those terms are bounded by |a|/beta <= What
  and by Ghat_i = sqrt2 / beta sum_e |J wbar|_e |a_ei|, so Ghat Ghat' is added to the magnitude and nq to the length.
* -F'F blocks of the full route, per cone:
  - R: -d^2, one rounding each side: 2 u d^2.
  - Q: -beta^2 (2 wbar_i wbar_j - J_ij), wbar_0 = w_0^2 / beta - 1, wbar_i = w_0 w_i / beta: 16 u beta^2 (2 |wbar|^ |wbar|^' + 1)
    with |wbar|^_0 = w_0^2 / beta + 1, |wbar|^_i = |w_0 w_i| / beta.
  - S: F'F = the symmetric Kronecker product of M = R R' on vecm coordinates, two congruences of order r on each side:
    2 (4 r + 8) u symkron(|R| |R|').

The Q-cone formulas are the ones the device evaluates: F^-1 = J F J / beta^2 and F^2 = beta^2 (2 wbar wbar' - J) hold
for the Nesterov-Todd scaling because QF(w) = w_0^2 - |w_1:|^2 = 2 beta.  The oracle's Woodbury inverse and square
of the same block agree with them to the rounding of that identity; tests/test_kkt_ref.py checks the agreement
against oracle.kktsolvers.schur2x2 / assemble3x3.  R and S cones go through the oracle's blocks directly.
"""
import numpy as np

from oracle.block import SymWoodbury, VecCongurance

U = np.finfo(np.float64).eps / 2
SQRT2 = np.sqrt(2.0)


def _dense(M):
    return np.asarray(M.toarray() if hasattr(M, "toarray") else M, dtype=np.float64)


def _order(k):
    return int(round((np.sqrt(1 + 8 * k) - 1) / 2))


def q_params(blk, k):
    """(beta, w) of a Q-cone block, F = diag(-beta, beta, ..) + w w' -- what the device is handed (cipkkt.kkt.pack_scaling)"""
    if isinstance(blk, SymWoodbury):
        return -float(blk.A[0]), blk.B[:, 0] * np.sqrt(blk.D[0, 0])
    d = float(np.asarray(blk.diag).reshape(-1)[0])          # a uniform Diagonal d I = diag(-d, d, ..) + 2 d e1 e1'
    w = np.zeros(k)
    w[0] = np.sqrt(2.0 * d)
    return d, w


def _s_R(blk, r):
    if isinstance(blk, VecCongurance):
        return blk.R
    return np.sqrt(float(np.asarray(blk.diag).reshape(-1)[0])) * np.eye(r)


def mat_cols(X, r):
    """mat of every column of X (k x n) -> (n, r, r)"""
    iu = np.triu_indices(r)
    scale = np.where(iu[0] == iu[1], 1.0, SQRT2)
    Z = np.zeros((X.shape[1], r, r))
    V = (X / scale[:, None]).T
    Z[:, iu[0], iu[1]] = V
    Z[:, iu[1], iu[0]] = V
    return Z


def vecm_cols(Z):
    """vecm of every matrix of Z (n, r, r) -> (k, n)"""
    r = Z.shape[1]
    iu = np.triu_indices(r)
    scale = np.where(iu[0] == iu[1], 1.0, SQRT2)
    return (Z[:, iu[0], iu[1]] * scale[None, :]).T


def symkron(M):
    """the matrix of x -> vecm(M mat(x) M) for a symmetric M (k x k, k = r (r + 1) / 2)"""
    r = M.shape[0]
    I, J = np.triu_indices(r)
    d = np.where(I == J, 1.0, SQRT2)            # rows: vecm scales the off-diagonal entries by sqrt2
    c = np.where(I == J, 0.5, 1.0 / SQRT2)      # columns: mat(e_b) holds 1/sqrt2 twice, or 1 once (counted twice below)
    k = len(I)
    out = np.empty((k, k))
    for b0 in range(0, k, 512):
        b = slice(b0, min(k, b0 + 512))
        out[:, b] = (M[np.ix_(I, I[b])] * M[np.ix_(J, J[b])] + M[np.ix_(I, J[b])] * M[np.ix_(J, I[b])]) * d[:, None] * c[None, b]
    return out


def scaled_rows(A, cone_dims, F):
    """(W, What, Ghat, cw): W = F^-T A, What its term magnitudes, Ghat (n x nq) the magnitude of the CSR route's rank-nq
    columns, cw the largest operation count behind one entry of W"""
    Ad = _dense(A)
    m, n = Ad.shape
    W = np.empty((m, n))
    What = np.empty((m, n))
    gh = []
    cw = 2
    off = 0
    for (t, k), blk in zip(cone_dims, F.Blocks):
        a = Ad[off:off + k]
        if t == "R":
            W[off:off + k] = blk.inv().adjoint().mul(a)
            What[off:off + k] = np.abs(a) / np.abs(np.asarray(blk.diag, dtype=np.float64).reshape(k))[:, None]
        elif t == "Q":
            beta, w = q_params(blk, k)
            tt = (w[0] * a[0] - w[1:] @ a[1:]) / beta
            W[off] = (w[0] * tt - a[0]) / beta
            W[off + 1:off + k] = (a[1:] - w[1:, None] * tt[None, :]) / beta
            that = np.abs(w) @ np.abs(a) / beta
            What[off:off + k] = (np.abs(a) + np.abs(w)[:, None] * that[None, :]) / beta
            jwb = np.abs(w[0] * w) / beta
            jwb[0] = w[0] * w[0] / beta + 1.0
            gh.append(SQRT2 / beta * (jwb @ np.abs(a)))
            cw = max(cw, k + 4)
        else:
            r = _order(k)
            W[off:off + k] = blk.inv().adjoint().mul(a) if isinstance(blk, VecCongurance) else a / float(blk.diag[0])
            Ri = np.abs(np.linalg.inv(_s_R(blk, r)))
            What[off:off + k] = vecm_cols(Ri @ np.abs(mat_cols(a, r)) @ Ri.T)
            cw = max(cw, 2 * r + 4)
        off += k
    Ghat = np.stack(gh, axis=1) if gh else np.zeros((n, 0))
    return W, What, Ghat, cw


def _gram(X):
    return X.T @ X


def reference(Q, A, G, cone_dims, F, route, Npad, csr=False, gram=_gram):
    """(K, copied, bound), see the module docstring.  ``gram(X)`` computes X'X (fp64); ``csr``: the device assembles
    from a CSR A (the Schur route then adds the rank-nq bound terms)."""
    Qd = _dense(Q)
    n = Qd.shape[0]
    Ad = _dense(A).reshape(-1, n)
    m = Ad.shape[0]
    Gd = _dense(G).reshape(-1, n) if G is not None else np.zeros((0, n))
    p = Gd.shape[0]
    K = np.zeros((Npad, Npad))
    copied = np.ones((Npad, Npad), dtype=bool)
    bound = np.zeros((Npad, Npad))
    if route == "schur":
        N = n + p
        W, What, Ghat, cw = scaled_rows(Ad, cone_dims, F)
        K[:n, :n] = Qd + gram(W)
        mag = np.abs(Qd) + gram(What)
        if csr and Ghat.shape[1]:
            mag += gram(Ghat.T)
        length = -(-max(m, 1) // 16) * 16 + 1 + 2 * cw + (Ghat.shape[1] if csr else 0)
        bound[:n, :n] = 2 * length * U * mag
        copied[:n, :n] = False
        K[n:N, :n] = Gd
    else:
        N = n + p + m
        off = 0
        for (t, k), blk in zip(cone_dims, F.Blocks):
            s = slice(off, off + k)
            if t == "R":
                d = np.asarray(blk.diag, dtype=np.float64).reshape(k)
                K[s, s] = np.diag(-d * d)
                bound[s, s] = np.diag(2 * U * d * d)
            elif t == "Q":
                beta, w = q_params(blk, k)
                wb = w[0] * w / beta
                wb[0] = w[0] * w[0] / beta - 1.0
                J = np.full(k, -1.0)
                J[0] = 1.0
                K[s, s] = -beta * beta * (2.0 * np.outer(wb, wb) - np.diag(J))
                wh = np.abs(w[0] * w) / beta
                wh[0] = w[0] * w[0] / beta + 1.0
                bound[s, s] = 16 * U * beta * beta * (2.0 * np.outer(wh, wh) + 1.0)
            else:
                r = _order(k)
                R = _s_R(blk, r)
                K[s, s] = -symkron(R @ R.T)
                Ra = np.abs(R)
                bound[s, s] = 2 * (4 * r + 8) * U * symkron(Ra @ Ra.T)
            copied[s, s] = False
            off += k
        K[m:m + n, :m] = -Ad.T
        if hasattr(A, "tocsr"):                 # a CSR A scatters its stored entries only: +0.0 elsewhere (dense: -0.0)
            pat = A.tocsr().copy()
            pat.data = np.ones_like(pat.data)
            K[m:m + n, :m][pat.toarray().T == 0] = 0.0
        K[m:m + n, m:m + n] = Qd
        K[m + n:N, m:m + n] = Gd
    K[N:, N:] = np.eye(Npad - N)
    return K, copied, bound


def check(Kd, K, copied, bound, stripe=1024):
    """assert the device matrix Kd against reference(...): copied entries bit-identical, computed ones within the bound,
    on the lower triangle (in row stripes, to keep the temporaries small at large orders)"""
    Np = K.shape[0]
    for r0 in range(0, Np, stripe):
        r1 = min(Np, r0 + stripe)
        low = np.arange(r0, r1)[:, None] >= np.arange(Np)[None, :]
        kd, kr, cp, bd = Kd[r0:r1], K[r0:r1], copied[r0:r1], bound[r0:r1]
        bad = low & cp & (kd.view(np.int64) != kr.view(np.int64))
        if bad.any():
            i, j = np.argwhere(bad)[0]
            raise AssertionError("%d copied entries differ, first (%d, %d): %r != %r"
                                 % (bad.sum(), r0 + i, j, kd[i, j], kr[i, j]))
        bad = low & ~cp & ~(np.abs(kd - kr) <= bd)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            raise AssertionError("%d computed entries outside the bound, first (%d, %d): %r vs %r, |err| %g > %g"
                                 % (bad.sum(), r0 + i, j, kd[i, j], kr[i, j], abs(kd[i, j] - kr[i, j]), bd[i, j]))
