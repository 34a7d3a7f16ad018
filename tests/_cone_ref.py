"""High-precision references and entrywise error bounds for the per-cone kernels (csrc/cones.hip, csrc/sdp.hip,
csrc/sdp_large.hip), for the hard iterates of tests/test_gpu_cone_edges.py.

Exact values.  R and Q cones: every operation is evaluated in mpmath at 50 digits on the given fp64 inputs, with the
closed forms of the reference (nestod_soc, maxstep_rp / maxstep_soc, xsoc! / dsoc!, src/ConicIP.jl:165-194,
:212-270, :317-345).  At 50 digits the reference's own error is below 1e-45 relative: it is exact for these tests.

Bounds (R and Q).  Each kernel output is a straight-line formula of its inputs -- the formula of cones.hip, which is
the reference's, cancellations included: QF(z) = z0^2 - |z1|^2, 1 + zbar.sbar, sbar_e - zbar_e, the quadratic of
maxstep_soc.  The class ``Ev`` carries, beside each exact intermediate value v, a first-order bound e on the error of
its fp64 evaluation (a running error analysis), with u = 2^-53:

  fl(a +- b): e = e_a + e_b + u |a +- b|          fl(a b): e = |a| e_b + |b| e_a + u |a b|
  fl(a / b):  e = (e_a + |a / b| e_b) / |b| + u |a / b|          fl(sqrt a): e = e_a / (2 sqrt a) + u sqrt a
  a reduction sum_{i<n} a_i b_i in ANY order (sequential, xor-shuffles of a pack segment, the 256-lane LDS hop):
      e = sum_i (|a_i| e_bi + |b_i| e_ai) + n u sum_i |a_i b_i|          (gamma_n to first order)

So e is u times the same formula evaluated on magnitudes, and the condition factors come out of the propagation
itself: QF(z) = z0^2 - |z1|^2 carries (k + 1) u (z0^2 + |z1|^2), relative (k + 1) u (z0^2 + |z1|^2) / QF(z), and every
quantity divided by QF or by its square root inherits that factor.  A fused multiply-add rounds once where the model
rounds twice, so it only lowers the error.  The bound is ``C * e`` with C = 4: a factor 2 covers an evaluation of
the same closed form whose scalar steps are arranged with up to twice as many roundings (the oracle's nestod_soc forms
zbar = z / sqrt(QF(z)) and sqrt(2 beta) / sqrt(2 w0) where the kernel multiplies by 1 / sqrt(QF) and takes one
sqrt(beta / w0)), the other factor 2 the second-order terms, which are below (u kappa)^2 with kappa <= 1e10 here.

Exact cases.  The R cone's max step (one rounding of d * scale, one of x / de, an exact min), its product and
division (one rounding) and its NT scaling (sqrt(s / v): two roundings; lambda = d v: one more) are compared bit for
bit with the same operations in fp64 numpy.  ``r_maxstep`` restates Julia's NaN rule: a NaN in x / de (d > 0)
or in x (the `nothing` form) makes the result NaN.

S cones.  The S references are evaluated in x87 extended precision (np.longdouble, 64-bit significand, unit roundoff
2^-64 = u / 2048) at test time, at every order up to 200, in well under a second per case.  That is why there is no
mpmath fixture for the large orders: mpmath's eigensolvers take minutes at order 200, while the S-cone kernels are
norm-wise accurate (Cholesky, Householder, Jacobi, GEMM), so a reference 2048 times finer than fp64 settles every
bound below with a margin, and the hard inputs never leave the seeds they are drawn from.  The checks are
certificates or norm-wise bounds, with c = 8 throughout:
  * max step: lambda_min(X - alpha scale D) within +-b, certified by two extended-precision Choleskys (the matrix
    plus b I is positive semidefinite, minus b I it is not positive definite).  The device computes
    1 / lambda_max(L^-1 D L^-T) (X = L L') through a Cholesky, two triangular solves and a Householder tridiagonal
    with a Sturm multisection; each step is norm-wise backward stable, so the computed alpha is exact for some
    X + dX, D + dD with |dX| <= c r u |X|_F, |dD| <= c r u |D|_F, and then |lambda_min(X - alpha s D)| <=
    c r u (|X|_F + alpha s |D|_F) (a Cholesky and a triangular solve each contribute at most 2 r u |.|_F, the
    tridiagonalisation and the bisection to its stop at 4.4e-16 the rest).  ``lambda_min_ratio`` bisects the
    certificate for |lambda_min| / b.
  * lambda_min(X) of the `nothing` form: the same certificate with b = c r u |X|_F.
  * congruences vecm(P' X P) (apply_F, four modes) and the product vecm(X Y + Y X): per entry
    C (2 r + 2) u (|P|' |X| |P|) resp. C (r + 2) u (|X| |Y| + |Y| |X|) (two resp. one GEMM of length r; the sqrt2
    scalings of mat / vecm), evaluated with the device's packed R and R^-1 as exact inputs.  F'F x = vecm(P X P),
    P = R R', is two such congruences: C (4 r + 4) u vecm(|R| |R|' |X| |R| |R|').
  * division by lambda = vecm(diag(Lambda)) (the loop's divisor): element-wise, out_ij = x_ij / (L_i + L_j),
    3 roundings per entry plus the sqrt2 scalings: C 5 u |out|.  A general divisor goes through the Jacobi
    eigensolver; it is checked by its residual |Y O + O Y - X|_F <= c r u (2 |Y|_F |O|_F + |X|_F).
  * NT scaling, Lambda: the singular values of G = Lz' Ls, with Lz, Ls, G and the singular values (one-sided
    Jacobi, ``svals_ld``) all in extended precision.  The device's Lambda_i are within b = c r u |Lz|_F |Ls|_F:
    its two Choleskys and the GEMM are norm-wise stable, and singular values are 1-Lipschitz in the 2-norm.
  * NT scaling, R and R^-1.  The device forms R = Lz^-T U Lambda^1/2 and, separately, R^-1 = Lambda^-1/2 U' Lz'.
    R' Z R = diag(Lambda) within 2 b entrywise.  Row i of R^-1 carries a relative error of order c r u
    |Lz|_F / Lambda_i^1/2 through U and Lz, and column j of S R^-T = Ls V Lambda^1/2 has norm at most
    |Ls|_F Lambda_j^1/2, so (R^-1 S R^-T)_ij is within b (sqrt(Lambda_i / Lambda_j) + sqrt(Lambda_j / Lambda_i))
    of diag(Lambda): the diagonal within 2 b, like R' Z R.

S cones above order ~300 (the last section of this file).  A full extended-precision product and the extended-precision
Jacobi are no longer affordable there; Choleskys, a few rows of a product and matrix-vector products are.  The same
quantities with the same bounds are evaluated on sampled rows (entrywise bound) and against +-1 probe vectors (row sums
of the entrywise bound), Lambda against LAPACK within 2 b, and the max step by the certificate alone.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
C = 4
UM = mp.mpf(2) ** -53
SQRT2 = np.sqrt(2.0)
LD = np.longdouble


# ------------------------------------------------------------------------------------------ running error arithmetic
class Ev:
    """exact value v and a first-order bound e on the error of its fp64 evaluation"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = mp.mpf(v)
        self.e = mp.mpf(e)

    @staticmethod
    def _c(o):
        return o if isinstance(o, Ev) else Ev(o)

    def __add__(self, o):
        o = Ev._c(o)
        v = self.v + o.v
        return Ev(v, self.e + o.e + UM * abs(v))
    __radd__ = __add__

    def __sub__(self, o):
        o = Ev._c(o)
        v = self.v - o.v
        return Ev(v, self.e + o.e + UM * abs(v))

    def __rsub__(self, o):
        return Ev._c(o) - self

    def __neg__(self):
        return Ev(-self.v, self.e)

    def __mul__(self, o):
        o = Ev._c(o)
        v = self.v * o.v
        return Ev(v, abs(self.v) * o.e + abs(o.v) * self.e + UM * abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Ev._c(o)
        v = self.v / o.v
        return Ev(v, (self.e + abs(v) * o.e) / abs(o.v) + UM * abs(v))

    def __rtruediv__(self, o):
        return Ev._c(o) / self

    def bound(self):
        return float(C * self.e)


def esqrt(a):
    v = mp.sqrt(a.v)
    return Ev(v, (a.e / (2 * v) if v > 0 else mp.inf if a.e > 0 else 0) + UM * v)


def edot(a, b):
    """sum_i a_i b_i of n terms in any order"""
    a = [Ev._c(x) for x in a]
    b = [Ev._c(x) for x in b]
    n = len(a)
    if n == 0:
        return Ev(0)
    v = mp.fsum(x.v * y.v for x, y in zip(a, b))
    e = mp.fsum(abs(x.v) * y.e + abs(y.v) * x.e for x, y in zip(a, b)) + n * UM * mp.fsum(abs(x.v * y.v) for x, y in zip(a, b))
    return Ev(v, e)


def ev(x):
    return [Ev(float(t)) for t in np.asarray(x, dtype=np.float64)]


def values(evs):
    return np.array([float(t.v) for t in evs])


def bounds(evs):
    return np.array([t.bound() for t in evs])


# ------------------------------------------------------------------------------------------ Q cone (k_nt_scaling ..)
def q_nt(z, s):
    """nestod_soc(z, s) as k_nt_scaling evaluates it: beta, w (k entries), lambda = F z (k entries)"""
    z, s = ev(z), ev(s)
    k = len(z)
    zz, ss, zs = edot(z[1:], z[1:]), edot(s[1:], s[1:]), edot(z[1:], s[1:])
    z0, s0 = z[0], s[0]
    qfz, qfs = z0 * z0 - zz, s0 * s0 - ss
    beta = esqrt(esqrt(qfs / qfz))
    rz, rs = 1 / esqrt(qfz), 1 / esqrt(qfs)
    zdots = (z0 * s0 + zs) * rz * rs
    gamma = esqrt((1 + zdots) * 0.5)
    h = 1 / (2 * gamma)
    wb0 = h * (s0 * rs + z0 * rz)
    c = esqrt(beta / (wb0 + 1))
    wdotz = c * (h * ((z0 * s0 + zs) * rs + qfz * rz) + z0)
    w = [c * (wb0 + 1)] + [c * h * (s[e] * rs - z[e] * rz) for e in range(1, k)]
    lam = [-beta * z0 + w[0] * wdotz] + [beta * z[e] + w[e] * wdotz for e in range(1, k)]
    return beta, w, lam


def q_apply(beta, w, x, inv):
    """F x (F = F') or F^-1 x (= F^-T x) of k_apply with the packed (beta, w) as exact inputs"""
    beta, w, x = Ev(float(beta)), ev(w), ev(x)
    k = len(x)
    if not inv:
        t = edot([w[0]] + w[1:], [x[0]] + x[1:])
        return [-beta * x[0] + w[0] * t] + [beta * x[e] + w[e] * t for e in range(1, k)]
    t = (w[0] * x[0] - edot(w[1:], x[1:])) / beta
    ib = 1 / beta
    return [(w[0] * t - x[0]) * ib] + [(x[e] - w[e] * t) * ib for e in range(1, k)]


def q_prod(x, y):
    x, y = ev(x), ev(y)
    return [edot(x, y)] + [x[0] * y[e] + y[0] * x[e] for e in range(1, len(x))]


def q_div(x, y):
    """out with y o out = x (dsoc!, k_cone_div)"""
    x, y = ev(x), ev(y)
    yy, yx = edot(y[1:], y[1:]), edot(y[1:], x[1:])
    y1, x1 = y[0], x[0]
    alpha = y1 * y1 - yy
    b1 = (-x1 / alpha) + yx / (y1 * alpha)
    b2 = 1 / y1
    return [(y1 * x1 - yx) / alpha] + [y[e] * b1 + x[e] * b2 for e in range(1, len(x))]


def q_maxstep(x, d, scale):
    """the alpha of maxstep_soc (step = 1 / alpha, Inf when alpha < 0) as k_maxstep evaluates it"""
    x = ev(x)
    sc = mp.mpf(float(scale))
    sd = [Ev(-sc * mp.mpf(float(t)), 0 if scale == 1.0 else UM * abs(sc * mp.mpf(float(t)))) for t in d]
    xx, xd = edot(x[1:], x[1:]), edot(x[1:], sd[1:])
    x0, d0 = x[0], sd[0]
    gam = x0 * x0 - xx
    rg = 1 / esqrt(gam)
    bet = (x0 * d0 - xd) * rg
    rho1 = bet * rg
    mu = (bet + d0) / (x0 * rg + 1)
    t = [sd[e] - mu * x[e] * rg for e in range(1, len(x))]
    r2 = edot(t, t)
    return esqrt(r2) * rg - rho1


def step_of(alpha):
    """(step, bound of step) from the Ev alpha; None when the sign of alpha is not determined by its bound"""
    a, b = alpha.v, C * alpha.e
    if abs(a) <= b:
        return None
    if a < 0:
        return mp.inf, mp.mpf(0)
    st = 1 / a
    return st, b / (a * a - a * b) + 2 * UM * st


def q_step_errors(alpha, got):
    """[(label, err, bound)] of a device step `got` against the Ev alpha of maxstep_soc (step = 1 / alpha, Inf for
    alpha <= 0).  The alpha the device stands for (1 / got, or some alpha <= 0 for Inf) must lie within the bound of
    alpha, whether or not that bound settles the sign; where it does, the step itself is held to its own bound."""
    a, b = alpha.v, C * alpha.e
    if got == np.inf:
        return [("maxstep Q alpha", max(a, 0), b)]
    out = [("maxstep Q alpha", abs(1 / mp.mpf(got) - a), b + 2 * UM / mp.mpf(got))]
    st = step_of(alpha)
    if st is not None and st[0] != mp.inf:
        out.append(("maxstep Q", abs(mp.mpf(got) - st[0]), st[1]))
    return out


def q_maxstep_none(x):
    x = ev(x)
    a = esqrt(edot(x[1:], x[1:])) - x[0]
    return a


def q_distance(x, d, scale, step):
    """x - step scale d in mpmath: (x0' - |x1'|, |scale d0| + |scale d1|), the second a bound on |d dist / d step|"""
    s = mp.mpf(float(scale)) * mp.mpf(float(step))
    y = [mp.mpf(float(a)) - s * mp.mpf(float(b)) for a, b in zip(x, d)]
    n1 = mp.sqrt(mp.fsum(t * t for t in y[1:]))
    sd = abs(mp.mpf(float(scale)))
    return y[0] - n1, sd * (abs(mp.mpf(float(d[0]))) + mp.sqrt(mp.fsum(mp.mpf(float(t)) ** 2 for t in d[1:])))


# ------------------------------------------------------------------------------------------ R cone (bit for bit)
def r_maxstep(x, d, scale):
    """k_maxstep on an R cone in fp64 numpy, with Julia's NaN rule"""
    x = np.asarray(x, dtype=np.float64)
    if d is None:
        if np.isnan(x).any():
            return np.nan
        mn = x.min() if x.size else np.inf
        return 0.0 if mn > 0 else -1.0 + mn
    de = np.asarray(d, dtype=np.float64) * np.float64(scale)
    pos = de > 0
    if not pos.any():
        return np.inf
    q = x[pos] / de[pos]
    return np.nan if np.isnan(q).any() else float(q.min())


def r_distance_bound(x, d, scale, step):
    """(distance min_i (x_i - step scale d_i) in mpmath, its bound): the step carries two roundings, so the entries
    whose ratio lies within 4u of it may move by 3 u x_i"""
    s = mp.mpf(float(scale)) * mp.mpf(float(step))
    dist = min(mp.mpf(float(a)) - s * mp.mpf(float(b)) for a, b in zip(x, d))
    de = np.asarray(d) * scale
    pos = de > 0
    near = pos & (np.asarray(x) / np.where(pos, de, 1.0) <= step * (1 + 4 * U))
    return dist, 3 * U * float(np.max(np.asarray(x)[near])) if near.any() else 0.0


# ------------------------------------------------------------------------------------------ S cone (extended precision)
def order(k):
    return int(round((np.sqrt(1 + 8 * k) - 1) / 2))


def mat(x, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    r = order(len(x))
    Z = np.zeros((r, r), dtype=dtype)
    iu = np.triu_indices(r)
    v = np.where(iu[0] == iu[1], x, x / dtype(SQRT2) if dtype is np.float64 else x / np.sqrt(LD(2)))
    Z[iu] = v
    Z[iu[1], iu[0]] = v
    return Z


def vecm(Z):
    r = Z.shape[0]
    iu = np.triu_indices(r)
    x = Z[iu].copy()
    x[iu[0] != iu[1]] *= np.sqrt(LD(2)) if Z.dtype == LD else SQRT2
    return x


def chol_ld(M):
    """lower Cholesky factor in extended precision, None if M is not positive definite"""
    A = np.array(M, dtype=LD)
    r = A.shape[0]
    L = np.zeros_like(A)
    for j in range(r):
        p = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not p > 0:
            return None
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lambda_min_within(M, centre, b):
    """certificate: lambda_min(M) in [centre - b, centre + b] (M extended precision, symmetric)"""
    I = np.eye(M.shape[0], dtype=LD)
    lo_ok = chol_ld(M - LD(centre - b) * I) is not None         # M - (centre - b) I > 0: lambda_min > centre - b
    hi_ok = chol_ld(M - LD(centre + b) * I) is None             # M - (centre + b) I not > 0: lambda_min <= centre + b
    return lo_ok and hi_ok


def fro(M):
    return float(np.sqrt(np.sum(np.asarray(M, dtype=np.float64) ** 2)))


def s_congruence(P, x, tr):
    """vecm(P' X P) (tr False) or vecm(P X P') in extended precision, and the per-entry bound"""
    P = np.asarray(P, dtype=np.float64)
    Pl = P.astype(LD)
    X = mat(x, LD)
    r = P.shape[0]
    if tr:
        Pl, Pa = Pl.T, np.abs(P).T
    else:
        Pa = np.abs(P)
    Y = Pl.T @ X @ Pl
    Ya = Pa.T @ np.abs(mat(x)) @ Pa
    return vecm(Y).astype(np.float64), C * (2 * r + 2) * U * vecm(Ya)


def s_prod(x, y):
    X, Y = mat(x, LD), mat(y, LD)
    r = X.shape[0]
    Xa, Ya = np.abs(mat(x)), np.abs(mat(y))
    return vecm(X @ Y + Y @ X).astype(np.float64), C * (r + 2) * U * vecm(Xa @ Ya + Ya @ Xa)


def s_div_diag(x, lam):
    """out with Y O + O Y = X for Y = diag(lam): O_ij = X_ij / (lam_i + lam_j)"""
    X = mat(x, LD)
    lam = np.asarray(lam, dtype=LD)
    O = X / (lam[:, None] + lam[None, :])
    o = vecm(O).astype(np.float64)
    return o, C * 5 * U * np.abs(o)


def s_div_residual(x, y, o):
    """(|Y O + O Y - X|_F, its bound) for a general divisor, O the device's quotient"""
    X, Y, O = mat(x, LD), mat(y, LD), mat(o, LD)
    r = X.shape[0]
    res = fro((Y @ O + O @ Y - X).astype(np.float64))
    return res, 8 * r * U * (2 * fro(mat(y)) * fro(mat(o)) + fro(mat(x)))


def svals_ld(G):
    """singular values of G, ascending, by one-sided Jacobi in extended precision (round-robin pairs, vectorised)"""
    A = np.array(G, dtype=LD)
    n = A.shape[1]
    if n % 2:
        A = np.hstack([A, np.zeros((A.shape[0], 1), dtype=LD)])
    m = A.shape[1]
    eps = LD(np.finfo(LD).eps)
    for _ in range(80):
        rotated = False
        for t in range(m - 1):
            k = np.arange(1, m // 2)
            p = np.concatenate([[m - 1], (t + k) % (m - 1)])
            q = np.concatenate([[t], (t - k) % (m - 1)])
            Ap, Aq = A[:, p], A[:, q]
            a, b, c = (Ap * Ap).sum(0), (Aq * Aq).sum(0), (Ap * Aq).sum(0)
            live = np.abs(c) > eps * np.sqrt(a * b)
            if not live.any():
                continue
            rotated = True
            cc = np.where(live, c, LD(1))
            zeta = (b - a) / (2 * cc)
            tt = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            cs = np.where(live, 1 / np.sqrt(1 + tt * tt), LD(1))
            sn = np.where(live, cs * tt, LD(0))
            A[:, p] = cs * Ap - sn * Aq
            A[:, q] = sn * Ap + cs * Aq
        if not rotated:
            break
    return np.sort(np.sqrt((A[:, :n] * A[:, :n]).sum(0)))


def s_nt(z, s):
    """(Lambda sorted ascending, its bound b, Lz, Ls) of nestod_sdc, all in extended precision"""
    Lz, Ls = chol_ld(mat(z, LD)), chol_ld(mat(s, LD))
    r = Lz.shape[0]
    sv = svals_ld(Lz.T @ Ls).astype(np.float64)
    return sv, 8 * r * U * fro(Lz) * fro(Ls), Lz, Ls


def s_rinv_bound(lam, b):
    """entrywise bound of R^-1 S R^-T - diag(Lambda) (lam: the device's Lambda in R's column order)"""
    q = np.sqrt(np.asarray(lam, dtype=np.float64))
    return b * (q[:, None] / q[None, :] + q[None, :] / q[:, None])


def s_ftf(R, x):
    """F'F x = vecm(P X P), P = R R', in extended precision, and its per-entry bound"""
    R = np.asarray(R, dtype=np.float64)
    r = R.shape[0]
    Rl = R.astype(LD)
    P = Rl @ Rl.T
    Pa = np.abs(R) @ np.abs(R).T
    return vecm(P @ mat(x, LD) @ P).astype(np.float64), C * (4 * r + 4) * U * vecm(Pa @ np.abs(mat(x)) @ Pa)


def lambda_min_ratio(M, b):
    """|lambda_min(M)| / b to within a factor 2^(1/8), by bisecting the certificate (1.0 when it fails at b)"""
    if not lambda_min_within(M, 0.0, b):
        return np.inf
    lo, hi = -40.0, 0.0                                        # log2 of the ratio
    while hi - lo > 0.125:
        mid = 0.5 * (lo + hi)
        if lambda_min_within(M, 0.0, b * 2.0 ** mid):
            hi = mid
        else:
            lo = mid
    return 2.0 ** hi


def s_maxstep_bound(x, d, scale, step):
    r = order(len(x))
    return 8 * r * U * (fro(mat(x)) + step * abs(scale) * fro(mat(d)))


# ------------------------------------------------------------------------------------------ hard iterates
def q_point(k, gap, rng):
    """a Q-cone point with relative gap (x0 - |x1|) / x0 = gap"""
    x = rng.standard_normal(k) * 10.0 ** rng.uniform(-3, 3)
    if k == 1:
        x[0] = abs(x[0]) + 0.1
        return x
    x[0] = np.linalg.norm(x[1:]) / (1.0 - gap)
    return x


def q_boundary_near(x, rng, eps=1e-3):
    """a point y on the boundary of Q near x (y0 = |y1|)"""
    y = x.copy()
    if len(x) == 1:
        y[0] = 0.0
        return y
    y[1:] = x[1:] * (1 + eps * rng.standard_normal(len(x) - 1))
    y[0] = np.linalg.norm(y[1:])
    return y


def q_direction(x, kind, rng):
    """d with x - alpha d crossing the boundary near alpha = 1 ('one'), near alpha = 1e6 ('far') or never ('never')"""
    if kind == "never":
        p = q_point(len(x), 0.5, rng)
        return -p
    d = x - q_boundary_near(x, rng)
    return d if kind == "one" else d * 1e-6


def s_point(r, span, rng):
    """vecm of U diag(lam) U' with lam log-spaced over [1, span] (times a random scale), U random orthogonal"""
    Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
    lam = np.logspace(0.0, np.log10(span), r) * 10.0 ** rng.uniform(-2, 2) if r > 1 else np.array([1.0 + rng.random()])
    M = (Q * rng.permutation(lam)) @ Q.T
    return vecm(0.5 * (M + M.T))


# ------------------------------------------------------------------------------------------ S cone above order ~300
# A full extended-precision product costs r^3 (18 s at order 1025) and the extended-precision Jacobi minutes; Choleskys, a
# few rows of a product (|S| r^2) and matrix-vector products stay cheap at every order.  The forms below evaluate the same
# quantities and the same entrywise bounds as s_congruence, s_ftf, s_prod and the two NT identities above, on a set of
# rows and against probe vectors.  Values are np.longdouble and in matrix form: the caller compares rows S of
# mat(device output, LD) (resp. mat(device output, LD) @ W) with them.  In matrix form the sqrt2 of vecm is gone from value
# and bound alike, so the bound of entry (i, j) is the bound of its vecm entry divided by the same factor.
def sample_rows(r, seed, extra=8):
    """the first and the last row of every band of 64 rows (clipped to r), rows 0 and r - 1, and `extra` rows drawn from
    `seed`: every 64 x 64 tile of an r x r result is crossed by at least two full rows"""
    S = {0, r - 1}
    for b0 in range(0, r, 64):
        S.update((b0, min(b0 + 63, r - 1)))
    S.update(int(i) for i in np.random.default_rng(seed).integers(0, r, extra))
    return np.array(sorted(S))


def probe_vectors(r, seed, count=2):
    """`count` columns of +-1 drawn from `seed` (r x count, extended precision)"""
    return np.where(np.random.default_rng(seed).random((r, count)) < 0.5, -1.0, 1.0).astype(LD)


def _mm(A, B):
    """A @ B.  numpy has no BLAS for np.longdouble and walks B down its columns: with B' laid out first the same
    sums, accumulated in extended precision, run several times faster"""
    if A.dtype != LD:
        return A @ B
    return np.einsum("ik,jk->ij", A, np.ascontiguousarray(B.T))


def _rows_of(terms, S):
    """rows S of sum_t A_1 A_2 .. A_k over the factor lists `terms`: |S| r^2 per factor"""
    out = 0
    for mats in terms:
        T = mats[0][S, :]
        for M in mats[1:]:
            T = _mm(T, M)
        out = out + T
    return out


def _applied(terms, W):
    """(sum_t A_1 A_2 .. A_k) W by matrix-vector products, right to left"""
    out = 0
    for mats in terms:
        T = W
        for M in reversed(mats):
            T = _mm(M, T)
        out = out + T
    return out


def _magnitudes(terms):
    return [[np.abs(M).astype(np.float64) for M in mats] for mats in terms]


def _congruence_terms(P, x, tr):
    Pl = np.asarray(P, dtype=np.float64).astype(LD)
    r = Pl.shape[0]
    return [[Pl, mat(x, LD), Pl.T] if tr else [Pl.T, mat(x, LD), Pl]], C * (2 * r + 2) * U


def _ftf_terms(R, x):
    Rl = np.asarray(R, dtype=np.float64).astype(LD)
    r = Rl.shape[0]
    return [[Rl, Rl.T, mat(x, LD), Rl, Rl.T]], C * (4 * r + 4) * U


def _prod_terms(x, y):
    X, Y = mat(x, LD), mat(y, LD)
    return [[X, Y], [Y, X]], C * (X.shape[0] + 2) * U


def _sampled(terms_const, S):
    terms, const = terms_const
    return _rows_of(terms, S), const * _rows_of(_magnitudes(terms), S)


def _probed(terms_const, W):
    """the per-row bound is the row sum of the entrywise bound, |(E w)_i| <= sum_j |E_ij| for w in {+-1}^r: deterministic and
    valid, about r times coarser than the entrywise bound (which is why there are sampled rows as well)"""
    terms, const = terms_const
    r = terms[0][0].shape[0]
    return _applied(terms, W), const * _applied(_magnitudes(terms), np.ones(r))


def s_congruence_rows(P, x, tr, S):
    """(rows S of P' X P (tr False) or P X P', rows S of the entrywise bound of s_congruence), matrix form"""
    return _sampled(_congruence_terms(P, x, tr), S)


def s_congruence_probe(P, x, tr, W):
    """((P' X P) W by matrix-vector products, the row sums of the entrywise bound of s_congruence)"""
    return _probed(_congruence_terms(P, x, tr), W)


def s_ftf_rows(R, x, S):
    return _sampled(_ftf_terms(R, x), S)


def s_ftf_probe(R, x, W):
    return _probed(_ftf_terms(R, x), W)


def s_prod_rows(x, y, S):
    return _sampled(_prod_terms(x, y), S)


def s_prod_probe(x, y, W):
    return _probed(_prod_terms(x, y), W)


def s_rzr_rows(R, z, lam, b, S):
    """(rows S of R' Z R - diag(lam), their bound 2 b), lam the device's Lambda in R's column order"""
    Rl = np.asarray(R, dtype=np.float64).astype(LD)
    T = _rows_of([[Rl.T, mat(z, LD), Rl]], S)
    T[np.arange(len(S)), S] -= np.asarray(lam, dtype=LD)[S]
    return T, np.full(T.shape, 2 * b)


def s_rzr_probe(R, z, lam, b, W):
    Rl = np.asarray(R, dtype=np.float64).astype(LD)
    r = Rl.shape[0]
    return _applied([[Rl.T, mat(z, LD), Rl]], W) - np.asarray(lam, dtype=LD)[:, None] * W, np.full(r, 2 * b * r)


def s_risri_rows(Ri, s, lam, b, S):
    """(rows S of R^-1 S R^-T - diag(lam), rows S of s_rinv_bound(lam, b))"""
    Ril = np.asarray(Ri, dtype=np.float64).astype(LD)
    T = _rows_of([[Ril, mat(s, LD), Ril.T]], S)
    T[np.arange(len(S)), S] -= np.asarray(lam, dtype=LD)[S]
    return T, s_rinv_bound(lam, b)[S, :]


def s_risri_probe(Ri, s, lam, b, W):
    Ril = np.asarray(Ri, dtype=np.float64).astype(LD)
    q = np.sqrt(np.asarray(lam, dtype=np.float64))
    bound = b * (q * np.sum(1.0 / q) + np.sum(q) / q)                                       # row sums of s_rinv_bound
    return _applied([[Ril, mat(s, LD), Ril.T]], W) - np.asarray(lam, dtype=LD)[:, None] * W, bound


def s_nt_fp64(z, s):
    """(Lambda sorted ascending, its bound 2 b, Lz, Ls, b) above order 300, where ``svals_ld`` takes minutes: Lz and Ls in
    extended precision (for b and the two NT identities, which pin Lambda: R' Z R = Lambda and R^-1 S R^-T = Lambda make
    Lambda^2 similar to Z S), the singular values by LAPACK from the factors rounded to fp64.  The rounding of the
    factors, the fp64 product Lz' Ls and LAPACK's SVD are norm-wise backward stable with the same constants as the
    device's Choleskys, GEMM and Jacobi, so the reference is itself within b = c r u |Lz|_F |Ls|_F of the exact singular
    values: device and reference differ by at most 2 b, one b for the device's error and one for the reference's."""
    Lz, Ls = chol_ld(mat(z, LD)), chol_ld(mat(s, LD))
    r = Lz.shape[0]
    b = 8 * r * U * fro(Lz) * fro(Ls)
    sv = np.linalg.svd(Lz.astype(np.float64).T @ Ls.astype(np.float64), compute_uv=False)
    return np.sort(sv), 2 * b, Lz, Ls, b


def s_nt_rotated(z, s):
    """(Lambda sorted ascending, its bound, Lz, Ls, b) as ``s_nt``, several times faster at orders 200 .. 300: the
    extended-precision Jacobi starts from G W, W the right singular vectors of G from LAPACK with one Newton-Schulz step
    W = V (3 I - V'V) / 2 in extended precision.  The columns of G W are orthogonal to u cond(G), so two or three sweeps
    are left of a dozen.  The singular values are those of G W and not of G: with eps = |W'W - I|_inf,
    |sigma_i(G W) - sigma_i(G)| <= eps sigma_i(G), and 2 eps (eps about 1e-17, evaluated here; the factor 2 for the
    rounding of W'W itself) times the largest singular value is added to b."""
    Lz, Ls = chol_ld(mat(z, LD)), chol_ld(mat(s, LD))
    r = Lz.shape[0]
    G = _mm(Lz.T, Ls)
    V = np.linalg.svd(G.astype(np.float64))[2].T.astype(LD)
    I = np.eye(r, dtype=LD)
    W = _mm(V, 1.5 * I - 0.5 * _mm(V.T, V))
    eps = float(np.abs(_mm(W.T, W) - I).sum(axis=1).max())
    sv = svals_ld(_mm(G, W)).astype(np.float64)
    b = 8 * r * U * fro(Lz) * fro(Ls)
    return sv, b + 2 * eps * float(sv.max()), Lz, Ls, b


def lambda_min_certified(M, b):
    """(the certificate |lambda_min(M)| <= b of ``lambda_min_within``: two extended-precision Choleskys,
    |lambda_min| / b from LAPACK on M rounded to fp64: for the ratio bookkeeping only, it carries LAPACK's own error)"""
    ok = lambda_min_within(M, 0.0, b)
    return ok, float(abs(np.linalg.eigvalsh(np.asarray(M, dtype=np.float64)).min()) / b)
