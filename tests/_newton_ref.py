"""Stage-by-stage references for the layer that joins the primitives into a Newton step: solve3x3_once, solve3x3_chunk,
cip_solve2x2_dev and cip_solve4x4_dev (conicip.jl_amd/csrc/solve.hip) and the fused k_s4_pre_r / k_s4_post_r (csrc/vecops.hip there).  No GPU here;
tests/test_newton_ref.py checks this module, tests/test_gpu_newton.py applies it to the device.

Why stages.  At the last interior-point iterations F spans ten decades and the Schur route is not backward stable: one
end-to-end bound says nothing.  Each piece of glue is therefore judged at the computed output of the piece in front of it
(u = 2^-53, extended precision = numpy.longdouble, |.|^ = the same formula evaluated on magnitudes, a running error bound):

  Schur route, solve3x3(x, y, z) -> (a, b, c), with the factor L^ D^ L^' read back from the handle
    rhs+sweeps   rhs* = [x + A' t*; y; 0], t* = F^-1 F^-T z exact (the formulas of the cone kernels on the packed scaling,
                 as tests/_kkt_ref.py); |rhs* - L^ D^ L^' [a; b; 0]| over all Npad rows within _ldlt_ref.SolveBound.check with
                 more = C2 (|A|' e_t + (len(A') + 1) u (|x| + |A|' t^)),  e_t = 2 cw u t^ + |F^-1|^ |F^-T|^ e_z
                 t^ = |F^-1|^ |F^-T|^ |z|; cw the operation count behind one entry of one cone application, row by row the
                 count of the row's own cone (R 2, Q k + 4, S 2 r + 4: _kkt_ref), len(A') the longest row of A'; e_z a bound
                 on the error of the z handed in (solve4x4).
    padding      where the whole padded solution is at hand (the fp64 model) its rows N .. Npad-1 are exact zeros.  The
                 device does not expose them: the padding block of K is an identity that no other row touches, so a finite
                 stale value there cannot reach (a, b) and a non-finite one turns every entry into NaN (0 * NaN in the
                 backward sweep), which rhs+sweeps rejects.
    backsub      c against c* = t* - F^-1 F^-T (A a) at the computed a, entrywise within
                 C2 (e_t + (2 cw + len(A) + 1) u (t^ + |F^-1|^ |F^-T|^ (|A| |a|)))
    solve2x2     the first stage with t = 0 (more = 0: the right-hand side is copied).
  Full 3x3 route: the glue is signed copies into the (v, y, w) order, [-z; x; y; 0] against the factor within SolveBound
    (more = e_z only).
  solve4x4(lambda, r) -> dz = (dy, dw, dv, ds)
    q* = r.s / lambda (the cone division, exact; the device's q within e_q: the bounds of tests/_cone_ref.py),
    t1* = F' q*, e_t1 = |F'|^ e_q + cw u |F'|^ |q*|;  the 3x3 stages run with z = r.v + t1* and e_z = e_t1 + u (|r.v| + |t1*|)
    ds           against t1* - F'F dv at the computed dv within C2 (e_t1 + (2 cw + 1) u (|F'|^ |q*| + |F'|^ |F|^ |dv|)).
  C2 = 2 covers an arrangement of the scalar steps with up to twice the roundings counted (as C of _cone_ref.py); the
  second-order terms are below (u kappa)^2 with kappa <= 1e10.

End-to-end record (end_to_end): the four block-row residuals of the true system at dz, each row scaled by its magnitude sum.
The same figures of the oracle's fp64 solve (oracle_4x4: pivot(kktsolver_2x2) on the Schur route, kktsolver_qr on the full
one) are the yardstick: device <= margin x max(oracle, 16 u) on every figure (below 16 u a scaled residual is rounding noise
that moves with the BLAS at hand).  (pivot applies F^-T twice, exact only for R and Q cones: with S cones on the Schur route
the oracle's third figure is of order one and the comparison is slack there; the stage checks carry those cases.)  The margin
is no constant: case_margin measures it, case by case and on the CPU, as max(4, 2 x the worst ratio the fp64 model of the
shipped chain (Model: assembly as _kkt_ref, _ldlt_ref.model_factor / model_solve, numpy glue) shows over the oracle on the
case's right-hand sides (rhs_table: random and graded, three draws each; the device runs the first draw of each).  Model and
oracle run the same algebra and differ in summation order and in the factorisation: the margin pays for exactly that, and a
case where they agree (R + Q, S: ratios of 1 to 4) does not inherit the 1e10 of the all-R cases with m > n, whose equality rows
G dy = r.w come out at 2e-5 from the static-order LDL' and at 1e-15 from the oracle's LU with partial pivoting.
"""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import _cone_ref as CR
import _kkt_ref as KR
import _ldlt_ref as LR
from oracle.block import Block, Diagonal, SymWoodbury, VecCongurance
from oracle.conicip import make_cone_ops
from oracle.kktsolvers import kktsolver_2x2, kktsolver_qr, pivot

LD = np.longdouble
U = 2.0 ** -53
C2 = 2.0
OP_F, OP_FT, OP_FINV, OP_FINVT = 0, 1, 2, 3
E2E_FLOOR = 16 * U       # end-to-end figures of the oracle below this are rounding noise: the denominator's floor


def _ld(v):
    """an mpmath value as a long double (two fp64 pieces)"""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


# ---------------------------------------------------------------------------------------------------------- cone operators
class Cones:
    """the block operator F of a packed scaling (R: d; Q: beta, w; S: R then R^-1, column-major), applied per cone in any
    dtype, with the magnitude form of every application"""

    def __init__(self, cone_dims, packed):
        self.dims = [(t, int(k)) for t, k in cone_dims]
        self.m = sum(k for _, k in self.dims)
        self.par = []
        cw = []                                       # per row: the operation count behind one entry of one application
        packed = np.asarray(packed, dtype=np.float64)
        o = 0
        for t, k in self.dims:
            if t == "R":
                self.par.append((packed[o:o + k],))
                o += k
                cw += [2] * k
            elif t == "Q":
                self.par.append((packed[o], packed[o + 1:o + 1 + k]))
                o += k + 1
                cw += [k + 4] * k
            else:
                r = CR.order(k)
                self.par.append((packed[o:o + r * r].reshape(r, r, order="F"), packed[o + r * r:o + 2 * r * r].reshape(r, r, order="F")))
                o += 2 * r * r
                cw += [2 * r + 4] * k
        assert o == packed.size
        self.cw = np.array(cw, dtype=np.float64)

    @classmethod
    def from_blocks(cls, cone_dims, F):
        out = []
        for (t, k), blk in zip(cone_dims, F.Blocks):
            if t == "R":
                out.append(np.asarray(blk.diag, dtype=np.float64).reshape(k))
            elif t == "Q":
                beta, w = KR.q_params(blk, k)
                out.append(np.concatenate([[beta], w]))
            else:
                R = np.asarray(blk.R, dtype=np.float64)
                out.append(np.concatenate([R.reshape(-1, order="F"), np.linalg.inv(R).reshape(-1, order="F")]))
        return cls(cone_dims, np.concatenate(out) if out else np.zeros(0))

    def blocks(self):
        """the oracle's Block of the same scaling"""
        out = []
        for (t, k), par in zip(self.dims, self.par):
            if t == "R":
                out.append(Diagonal(par[0]))
            elif t == "Q":
                J = np.full(k, par[0])
                J[0] = -par[0]
                out.append(SymWoodbury(J, par[1], 1.0))
            else:
                out.append(VecCongurance(par[0]))
        return Block(out)

    def _each(self, x, fn):
        x = np.asarray(x)
        out = np.empty_like(x)
        o = 0
        for (t, k), par in zip(self.dims, self.par):
            out[o:o + k] = fn(t, par, x[o:o + k])
            o += k
        return out

    def apply(self, mode, x, dtype=LD):
        inv = mode in (OP_FINV, OP_FINVT)

        def one(t, par, xc):
            if t == "R":
                d = par[0].astype(dtype)
                return xc / d if inv else xc * d
            if t == "Q":
                beta, w = dtype(par[0]), par[1].astype(dtype)
                if not inv:
                    tt = w @ xc
                    out = beta * xc + w * tt
                    out[0] = -beta * xc[0] + w[0] * tt
                    return out
                tt = (w[0] * xc[0] - w[1:] @ xc[1:]) / beta
                out = (xc - w * tt) / beta
                out[0] = (w[0] * tt - xc[0]) / beta
                return out
            P = (par[1] if inv else par[0]).astype(dtype)
            if mode in (OP_FT, OP_FINVT):
                P = P.T
            return CR.vecm(P.T @ CR.mat(xc, dtype) @ P)             # F: R' X R, F': R X R', F^-1: Ri' X Ri, F^-T: Ri X Ri'

        return self._each(np.asarray(x).astype(dtype), one)

    def mag(self, mode, xa):
        inv = mode in (OP_FINV, OP_FINVT)

        def one(t, par, xc):
            if t == "R":
                return xc / par[0] if inv else xc * par[0]
            if t == "Q":
                beta, w = par[0], np.abs(par[1])
                return (xc + w * ((w @ xc) / beta)) / beta if inv else beta * xc + w * (w @ xc)
            P = np.abs(par[1] if inv else par[0])
            if mode in (OP_FT, OP_FINVT):
                P = P.T
            return CR.vecm(P.T @ CR.mat(xc) @ P)

        return self._each(np.abs(np.asarray(xa, dtype=np.float64)), one)

    def ftf_inv(self, z, dtype=LD):
        return self.apply(OP_FINV, self.apply(OP_FINVT, z, dtype), dtype)

    def ftf_inv_mag(self, za):
        return self.mag(OP_FINV, self.mag(OP_FINVT, za))

    def ftf(self, x, dtype=LD):
        return self.apply(OP_FT, self.apply(OP_F, x, dtype), dtype)

    def ftf_mag(self, xa):
        return self.mag(OP_FT, self.mag(OP_F, xa))

    def div(self, x, lam):
        """(q, e_q): the cone division x / lambda in extended precision and the bound of its fp64 evaluation (R: one
        rounding; Q: the running error of dsoc!, _cone_ref.q_div; S: lambda = vecm(diag(Lambda)), _cone_ref.s_div_diag)"""
        q, e = np.zeros(self.m, dtype=LD), np.zeros(self.m)
        o = 0
        for t, k in self.dims:
            xc, lc = np.asarray(x[o:o + k], dtype=np.float64), np.asarray(lam[o:o + k], dtype=np.float64)
            if t == "R":
                q[o:o + k] = xc.astype(LD) / lc.astype(LD)
                e[o:o + k] = U * np.abs(xc / lc)
            elif t == "Q":
                evs = CR.q_div(xc, lc)
                q[o:o + k] = [_ld(t_.v) for t_ in evs]
                e[o:o + k] = CR.bounds(evs)
            else:
                Lm = np.diag(CR.mat(lc, LD))
                q[o:o + k] = CR.vecm(CR.mat(xc, LD) / (Lm[:, None] + Lm[None, :]))
                e[o:o + k] = CR.C * 5 * U * np.abs(q[o:o + k].astype(np.float64))
            o += k
        return q, e

    def div64(self, x, lam):
        """the same division in fp64 (the model)"""
        _, _, cone_div, _ = make_cone_ops(self.dims)
        out = cone_div(np.asarray(x, dtype=np.float64), np.asarray(lam, dtype=np.float64)) if self.m else np.zeros(0)
        o = 0
        for t, k in self.dims:
            if t == "S":
                Lm = np.diag(CR.mat(lam[o:o + k]))
                out[o:o + k] = CR.vecm(CR.mat(x[o:o + k]) / (Lm[:, None] + Lm[None, :]))
            o += k
        return out


# ---------------------------------------------------------------------------------------------------------------- problems
Problem = namedtuple("Problem", "name route csr Q A Ad G cone_dims n p m N Npad v s mu")


def iterates(cone_dims, mu, rng, gaps=(1e-2, 1e-6, 1e-10), spans=(1e4, 1e8)):
    """a late-iteration pair (v, s): R entries v log-uniform over 1e-5 .. 1e5 with s = mu / v jittered by 30 %, Q points with
    the relative gaps in turn, S points with the eigenvalue spans in turn (s scaled by mu)"""
    vs, ss = [], []
    iq = isd = 0
    for t, k in cone_dims:
        if t == "R":
            v = 10.0 ** rng.uniform(-5.0, 5.0, k)
            vs.append(v)
            ss.append(mu / v * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, k)))
        elif t == "Q":
            vs.append(CR.q_point(k, gaps[iq % len(gaps)], rng))
            ss.append(mu * CR.q_point(k, gaps[(iq + 1) % len(gaps)], rng))
            iq += 1
        else:
            r = CR.order(k)
            vs.append(CR.s_point(r, spans[isd % len(spans)], rng))
            ss.append(mu * CR.s_point(r, spans[isd % len(spans)], rng))
            isd += 1
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    return cat(vs), cat(ss)


def make_problem(name, c=None):
    """the problem of a row of CASES (or of the given row): Q = M'M / n + 0.05 I, so that no case needs regularisation"""
    c = CASES[name] if c is None else c
    n, p, cone_dims, route, csr, mu = c["n"], c["p"], c["cones"], c["route"], c["csr"], c["mu"]
    rng = np.random.default_rng(sum(map(ord, name.replace("_csr", "").replace("_dense", "").replace("_full", "").replace("_schur", ""))))
    m = sum(k for _, k in cone_dims)
    M = rng.standard_normal((n, n))
    Q = M.T @ M / n + 0.05 * np.eye(n)
    Ad = rng.standard_normal((m, n)) / np.sqrt(n)
    G = rng.standard_normal((p, n))
    v, s = iterates(cone_dims, mu, rng, spans=c.get("spans", (1e4, 1e8)))
    if csr:
        keep = rng.random((m, n)) < 0.15
        keep[np.arange(m), rng.integers(0, n, m)] = True
        Ad = Ad * keep
    A = sp.csr_matrix(Ad) if csr else Ad
    N = n + p + (m if route == "full3x3" else 0)
    return Problem(name, route, csr, Q, A if m else None, Ad, G if p else None, cone_dims, n, p, m, N, -(-N // LR.NB) * LR.NB, v, s, mu)


def rhs4(P, kind, rng):
    """a solve4x4 right-hand side: 'normal', or 'graded' as the loop's own (r.y, r.w, r.v ~ 1e-8, r.s ~ mu)"""
    r = rng.standard_normal(P.n + P.p + 2 * P.m)
    if kind == "graded":
        r[:P.n + P.p + P.m] *= 1e-8
        r[P.n + P.p + P.m:] *= P.mu
    return r


_RQ = [("R", 37), ("Q", 1)] + [("Q", 8)] * 5 + [("R", 20), ("Q", 64), ("Q", 70), ("R", 11)]        # m = 243
# name -> problem.  Orders start from the launch arithmetic: k_s4_pre_r runs ceil(max(m, Npad) / 256) workgroups of 256 and
# k_s4_post_r ceil(max(m, n, p) / 256) (vecops.hip); Npad = the order rounded up to 128 (api.hip); the all-R Schur handles take
# the fused path, everything else the generic one; solve3x3_chunk takes 64 columns at a time.
CASES = {
    # m = 330 > Npad = 256: two workgroups, the second one past Npad; sections start at 200, 207, 537
    "allR_330_dense": dict(n=200, p=7, cones=[("R", 130), ("R", 200)], route="schur", csr=False, mu=1e-10),
    "allR_330_csr": dict(n=200, p=7, cones=[("R", 130), ("R", 200)], route="schur", csr=True, mu=1e-6),
    # m = 150 < Npad = 384: the tail of the launch writes the right-hand side only; sections start at 300, 307, 457
    "allR_150_dense": dict(n=300, p=7, cones=[("R", 50), ("R", 100)], route="schur", csr=False, mu=1e-2),
    # (m < n: A'(F'F)^-1 A has rank 150 and Q = O(0.05) must survive beside it -- at mu = 1e-6 the weights reach 1e16 and the
    # remaining pivots lose their sign, which a handle answers by regularising; these two rows stay at mu = 1e-2)
    "allR_150_csr": dict(n=300, p=7, cones=[("R", 50), ("R", 100)], route="schur", csr=True, mu=1e-2),
    "RQ_schur_dense": dict(n=90, p=5, cones=_RQ, route="schur", csr=False, mu=1e-6),
    "RQ_schur_csr": dict(n=90, p=5, cones=_RQ, route="schur", csr=True, mu=1e-10),
    "RQ_full_dense": dict(n=90, p=5, cones=_RQ, route="full3x3", csr=False, mu=1e-10),
    "RQ_full_csr": dict(n=90, p=5, cones=_RQ, route="full3x3", csr=True, mu=1e-2),
    "S7_schur": dict(n=30, p=3, cones=[("R", 5), ("S", 28), ("R", 3)], route="schur", csr=False, mu=1e-6, spans=(1e8,)),
    "S7_full": dict(n=30, p=3, cones=[("R", 5), ("S", 28), ("R", 3)], route="full3x3", csr=True, mu=1e-2, spans=(1e4,)),
    "S49_schur": dict(n=40, p=2, cones=[("S", 1225)], route="schur", csr=False, mu=1e-6, spans=(1e8,)),
    "S49_full": dict(n=40, p=2, cones=[("S", 1225)], route="full3x3", csr=False, mu=1e-2, spans=(1e4,)),
    # one order-133 cone (the side-by-side max-step range of sdp.hip starts here): matrix-free, no dense F'F, no oracle
    "S133_schur": dict(n=40, p=2, cones=[("S", 8911)], route="schur", csr=False, mu=1e-6, spans=(1e4,), oracle=False),
    "m0_schur": dict(n=50, p=6, cones=[], route="schur", csr=False, mu=1e-6),
    "m0_full": dict(n=50, p=6, cones=[], route="full3x3", csr=False, mu=1e-6),
    "p0_allR": dict(n=60, p=0, cones=[("R", 80)], route="schur", csr=True, mu=1e-10),
    "p0_RQ_full": dict(n=40, p=0, cones=[("R", 9), ("Q", 8), ("Q", 3)], route="full3x3", csr=False, mu=1e-2),
    # n + p = 128 = Npad: no padding rows at all
    "N128_RQ": dict(n=120, p=8, cones=[("R", 70), ("Q", 8), ("Q", 65), ("R", 7)], route="schur", csr=False, mu=1e-10),
}
MANY = {"allR_150_csr": (3, 64, 65), "RQ_schur_dense": (3, 64, 65)}          # solve3x3_many_dev, C aliasing Z; 2x2 at 65
MANY_CHUNK = 64


def paths(name):
    """the code paths a case reaches, restated from solve.hip / vecops.hip"""
    c = CASES[name]
    m = sum(k for _, k in c["cones"])
    N = c["n"] + c["p"] + (m if c["route"] == "full3x3" else 0)
    Npad = -(-N // LR.NB) * LR.NB
    out = {"csr" if c["csr"] and m else "dense", c["route"]}
    if m and all(t == "R" for t, _ in c["cones"]) and c["route"] == "schur":
        out.add("fused")
        out.add("fused m>Npad" if m > Npad else "fused m<Npad")
        if -(-max(m, Npad) // 256) > 1:
            out.add("fused two workgroups")
    else:
        out.add("generic")
    if Npad == N:
        out.add("no padding")
    for k in MANY.get(name, ()):
        out.add("chunk %s" % ("edge 64" if k == MANY_CHUNK else "edge 65" if k == MANY_CHUNK + 1 else "short"))
    return out


# ------------------------------------------------------------------------------------------------------------ stage checks
def _entry(err, bound, got):
    err, bound = np.abs(np.asarray(err)).astype(np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    fin = bool(np.all(np.isfinite(np.asarray(got, dtype=np.float64))))
    return dict(ok=bool(np.all(err <= bound)) and fin, ratio=float(ratio.max()) if ratio.size else 0.0, bound=bound)


def _lens(Ad):
    nz = Ad != 0
    return (int(nz.sum(axis=0).max()) if Ad.size else 0), (int(nz.sum(axis=1).max()) if Ad.size else 0)       # rows of A', of A


def check_3x3(P, cones, sb, c_s, x, y, z, a, b, c, e_z=None, pad=None):
    """the stages of one solve3x3 (z None: solve2x2) -> {stage: dict(ok, ratio, ..)}; sb = SolveBound of the factor the solve
    ran on; z may be extended precision with the error bound e_z; pad: the solution's padding rows where they are at hand"""
    n, p, N, Np = P.n, P.p, P.N, P.Npad
    m = P.m if z is not None else 0
    out = {}
    Aq, Aa = P.Ad.astype(LD), np.abs(P.Ad)
    len_At, len_A = _lens(P.Ad)
    rhs, more, sol = np.zeros(Np, dtype=LD), np.zeros(Np), np.zeros(Np)
    xq, yq = np.asarray(x).astype(LD), np.asarray(y).astype(LD)
    ez = np.zeros(m) if e_z is None else np.asarray(e_z, dtype=np.float64)
    if pad is not None:
        sol[N:] = pad
        out["padding"] = dict(ok=bool(np.all(np.asarray(pad) == 0.0)), ratio=float(np.abs(pad).max()) if len(pad) else 0.0)
    if P.route == "schur":
        sol[:n], sol[n:N] = a, b
        rhs[:n], rhs[n:N] = xq, yq
        if m:
            t = cones.ftf_inv(z)
            th = cones.ftf_inv_mag(np.abs(np.asarray(z, dtype=np.float64)))
            e_t = 2 * cones.cw * U * th + cones.ftf_inv_mag(ez)
            rhs[:n] += Aq.T @ t
            more[:n] = C2 * (Aa.T @ e_t + (len_At + 1) * U * (np.abs(np.asarray(x, dtype=np.float64)) + Aa.T @ th))
        out["rhs+sweeps"] = sb.check(rhs, sol, c_s, more=more)
        if m:
            aq = np.asarray(a).astype(LD)
            cstar = t - cones.ftf_inv(Aq @ aq)
            mag = th + cones.ftf_inv_mag(Aa @ np.abs(np.asarray(a, dtype=np.float64)))
            out["backsub"] = _entry(np.asarray(c).astype(LD) - cstar, C2 * (e_t + (2 * cones.cw + len_A + 1) * U * mag), c)
    else:
        sol[:m], sol[m:m + n], sol[m + n:N] = (c if m else np.zeros(0)), a, b
        if m:
            rhs[:m] = -np.asarray(z).astype(LD)
            more[:m] = ez
        rhs[m:m + n], rhs[m + n:N] = xq, yq
        out["rhs+sweeps"] = sb.check(rhs, sol, c_s, more=more)
    return out


def check_4x4(P, cones, sb, c_s, lam, r, dz, pad=None):
    """the stages of one solve4x4 at the computed dz"""
    n, p, m = P.n, P.p, P.m
    ry, rw, rv, rs = r[:n], r[n:n + p], r[n + p:n + p + m], r[n + p + m:]
    dy, dw, dv, ds = dz[:n], dz[n:n + p], dz[n + p:n + p + m], dz[n + p + m:]
    if m == 0:
        return check_3x3(P, cones, sb, c_s, ry, rw, None, dy, dw, None, pad=pad)
    q, e_q = cones.div(rs, lam)
    t1 = cones.apply(OP_FT, q)
    t1h = cones.mag(OP_FT, np.abs(q.astype(np.float64)))
    e_t1 = cones.mag(OP_FT, e_q) + cones.cw * U * t1h
    z = rv.astype(LD) + t1
    e_z = e_t1 + U * (np.abs(rv) + np.abs(t1.astype(np.float64)))
    out = check_3x3(P, cones, sb, c_s, ry, rw, z, dy, dw, dv, e_z=e_z, pad=pad)
    dstar = t1 - cones.ftf(dv)
    out["ds"] = _entry(ds.astype(LD) - dstar, C2 * (e_t1 + (2 * cones.cw + 1) * U * (t1h + cones.ftf_mag(np.abs(dv)))), ds)
    return out


def end_to_end(P, cones, lam, r, dz):
    """the four block-row residuals of the true system at dz, each row scaled by its magnitude sum: the largest per block
    (0 for an empty block) -- Q dy + G'dw - A'dv - r.y;  G dy - r.w;  A dy - ds - r.v;  F'F dv + ds - t1"""
    n, p, m = P.n, P.p, P.m
    G = P.G if p else np.zeros((0, n))
    ry, rw, rv, rs = (np.asarray(t).astype(LD) for t in (r[:n], r[n:n + p], r[n + p:n + p + m], r[n + p + m:]))
    dy, dw, dv, ds = (np.asarray(t).astype(LD) for t in (dz[:n], dz[n:n + p], dz[n + p:n + p + m], dz[n + p + m:]))
    Aq, Gq, Qq = P.Ad.astype(LD), G.astype(LD), P.Q.astype(LD)
    ab = lambda t: np.abs(t).astype(np.float64)
    res = [Qq @ dy + Gq.T @ dw - Aq.T @ dv - ry, Gq @ dy - rw]
    mags = [np.abs(P.Q) @ ab(dy) + np.abs(G).T @ ab(dw) + np.abs(P.Ad).T @ ab(dv) + ab(ry), np.abs(G) @ ab(dy) + ab(rw)]
    if m:
        q, _ = cones.div(r[n + p + m:], lam)
        t1 = cones.apply(OP_FT, q)
        res += [Aq @ dy - ds - rv, cones.ftf(dv) + ds - t1]
        mags += [np.abs(P.Ad) @ ab(dy) + ab(ds) + ab(rv), cones.ftf_mag(ab(dv)) + ab(ds) + cones.mag(OP_FT, ab(q))]
    out = np.zeros(4)
    for i, (rr, mm) in enumerate(zip(res, mags)):
        if rr.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                out[i] = float(np.max(np.where(mm > 0, ab(rr) / np.where(mm > 0, mm, 1.0), np.where(ab(rr) > 0, np.inf, 0.0))))
    return out


def oracle_4x4(P, cones, lam, r):
    """solve4x4 (src/ConicIP.jl:684-692) on the oracle's fp64 solver of the route, with the same scaling and lambda"""
    n, p, m = P.n, P.p, P.m
    F = cones.blocks()
    FinvT = F.inv_adjoint()
    G = P.G if p else np.zeros((0, n))
    solver = pivot(kktsolver_2x2) if P.route == "schur" else kktsolver_qr
    s3 = solver(P.Q, P.Ad, G, P.cone_dims)(F, FinvT)
    _, _, cone_div, _ = make_cone_ops(P.cone_dims)
    t1 = F.tmul(cone_div(r[n + p + m:], np.asarray(lam, dtype=np.float64))) if m else np.zeros(0)
    dy, dw, dv = s3(r[:n], r[n:n + p], r[n + p:n + p + m] + t1)
    ds = t1 - F.tmul(F.mul(dv)) if m else np.zeros(0)
    return np.concatenate([dy, dw, dv, ds])


def e2e_ratio(figs, orc):
    """the worst of the four figures over the oracle's, the denominator floored at 16 u"""
    return float(np.max(np.asarray(figs) / np.maximum(np.asarray(orc), E2E_FLOOR)))


def margin_of(worst):
    """the rule: the larger of 4 and twice the worst ratio the model shows over the oracle"""
    return max(4.0, 2.0 * float(worst))


def rhs_table(P, draws=3):
    """[(kind, draw, r)]: the right-hand sides of a case, 'normal' and 'graded', `draws` of each (draw 0 is what the device runs)"""
    key = lambda kind, d: [len(P.name), P.n, kind == "graded"] + ([d] if d else [])
    return [(kind, d, rhs4(P, kind, np.random.default_rng(key(kind, d)))) for kind in ("normal", "graded") for d in range(draws)]


def case_margin(P, model=None, cones=None, lam=None):
    """(margin, worst, rows): the end-to-end margin of one case, measured on the CPU from the fp64 model against the oracle on
    rhs_table(P); rows = [(kind, draw, model figures, oracle figures)]"""
    if model is None:
        cones, lam = model_inputs(P)
        model = Model(P, cones)
    rows = []
    for kind, d, r in rhs_table(P):
        mo = end_to_end(P, cones, lam, r, model.solve4x4(lam, r))
        orc = end_to_end(P, cones, lam, r, oracle_4x4(P, cones, lam, r))
        rows.append((kind, d, mo, orc))
    worst = max(e2e_ratio(mo, orc) for _, _, mo, orc in rows)
    return margin_of(worst), worst, rows


# ------------------------------------------------------------------------------------------------- the fp64 model of the chain
class Model:
    """the shipped chain in plain fp64 numpy: K as tests/_kkt_ref.py assembles it, the blocked LDL' and the block-inverse
    sweeps of tests/_ldlt_ref.py, the glue of solve3x3_once / cip_solve4x4_dev in numpy.  `defect` plants one error in the
    glue (DEFECTS) -- on this model only, for tests/test_newton_ref.py."""

    def __init__(self, P, cones):
        self.P, self.cones = P, cones
        G = P.G if P.p else np.zeros((0, P.n))
        K = KR.reference(P.Q, P.Ad, G, P.cone_dims, cones.blocks(), P.route, P.Npad, csr=P.csr)[0]
        K = np.tril(K) + np.tril(K, -1).T
        self.fac, self.rho, Xm, info = LR.model_factor(K)
        assert info == 0, "the model met a bad pivot at column %d" % info
        want = -np.ones(P.Npad)
        want[slice(0, P.n) if P.route == "schur" else slice(P.m, P.m + P.n)] = 1.0
        want[P.N:] = 1.0
        self.wrong_signs = int(np.sum(np.sign(np.diag(self.fac)) != want))         # a handle would regularise on any
        self.Bs = LR.dispatch(P.Npad, 3, 0, 1024, 0)[1]
        self.X = LR.model_block_inverses(self.fac, Xm, self.Bs)
        self.pad = None

    def _sweeps(self, rhs, defect):
        P = self.P
        if defect == "pad_one" and P.Npad > P.N:
            rhs[P.N] = 1.0
        sol = LR.model_solve(self.fac, self.rho, self.X, rhs)
        self.pad = sol[P.N:].copy()
        return sol

    def _ftf_inv(self, z, defect):
        t = self.cones.ftf_inv(z, np.float64)
        if defect == "f_for_ff":
            j = self._r_row()
            t[j] = z[j] / self.cones.apply(OP_F, np.ones(self.P.m), np.float64)[j]
        return t

    def _r_row(self):
        o = 0
        for t, k in self.P.cone_dims:
            if t == "R":
                return o + k // 2
            o += k
        raise AssertionError("no R cone")

    def solve3x3(self, x, y, z, defect=None):
        P, n, p = self.P, self.P.n, self.P.p
        m = P.m if z is not None else 0
        A = P.Ad
        rhs = np.zeros(P.Npad)
        sh = 1 if defect == "shift_yw" else 0
        if P.route == "schur":
            rhs[:n] = x
            t = self._ftf_inv(z, defect) if m else None
            if m:
                At = A.T.copy()
                if defect == "csr_last_At":
                    i = self.at_row
                    At[i, np.nonzero(At[i])[0][-1]] = 0.0
                rhs[:n] = At @ t + x
            rhs[n + sh:n + sh + p] = y
            sol = self._sweeps(rhs, defect)
            a, b = sol[:n].copy(), sol[n:n + p].copy()
            if not m:
                return a, b, None
            Ab = A.copy()
            if defect == "csr_last_A":
                i = int(np.argmax((Ab != 0).sum(axis=1)))
                Ab[i, np.nonzero(Ab[i])[0][-1]] = 0.0
            return a, b, t - self.cones.ftf_inv(Ab @ a, np.float64)
        if m:
            rhs[:m] = -z
        rhs[m:m + n] = x
        rhs[m + n + sh:m + n + sh + p] = y
        sol = self._sweeps(rhs, defect)
        return sol[m:m + n].copy(), sol[m + n:m + n + p].copy(), sol[:m].copy()

    def solve4x4(self, lam, r, defect=None):
        P, n, p, m, cones = self.P, self.P.n, self.P.p, self.P.m, self.cones
        ry, rw, rv, rs = r[:n], r[n:n + p], r[n + p:n + p + m], r[n + p + m:]
        if m == 0:
            a, b, _ = self.solve3x3(ry, rw, None, defect)
            return np.concatenate([a, b])
        q = cones.div64(rs, lam)
        t1 = cones.apply(OP_F if defect == "F_for_FT" else OP_FT, q, np.float64)
        z = rv + t1
        dy, dw, dv = self.solve3x3(ry, rw, z, defect)
        ds = t1 - cones.ftf(z if defect == "ds_before" else dv, np.float64)
        if defect == "dv_entry":
            dv = dv.copy()
            dv[self.dv_at] *= 1.0 + 1e-10
        return np.concatenate([dy, dw, dv, ds])


OWNERS = {"t": ("rhs+sweeps", "backsub")}          # a stage name standing for several checks: one of them must fail
# defect -> the stage that owns it (must fail)
DEFECTS = {
    "dv_entry": "backsub",           # one entry of dv off by 1e-10 relative (Model.dv_at: set by the test from the clean bounds)
    "F_for_FT": "ds",                # t1 = F q for F' q (differs on S cones only: R and Q blocks are symmetric)
    "f_for_ff": "t",                 # (F'F)^-1 z applied as z / f on one R row of t: t feeds the right-hand side and c = t - ..,
                                     # so either of the two stages that judge t owns it (the row may be below the sum's bound)
    "csr_last_A": "backsub",         # the last stored entry of one row of A dropped
    "csr_last_At": "rhs+sweeps",     # ... of one row of A' (Model.at_row: the row where that entry weighs most against the bound)
    "pad_one": "padding",            # a padding row of the right-hand side left at 1
    "ds_before": "ds",               # ds from the dv buffer before the back-substitution (it holds r.v + t1 then)
    "shift_yw": "rhs+sweeps",        # the y and w sections shifted by one
}


def model_inputs(P):
    """(cones, lambda) of the model: the oracle's Nesterov-Todd scaling of (v, s), lambda = F v (an S cone's made exactly
    diagonal, as the device hands it out)"""
    _, nt_scaling, _, _ = make_cone_ops(P.cone_dims)
    F = nt_scaling(P.v, P.s)
    cones = Cones.from_blocks(P.cone_dims, F)
    lam = F.mul(P.v) if P.m else np.zeros(0)
    o = 0
    for t, k in P.cone_dims:
        if t == "S":
            lam[o:o + k] = CR.vecm(np.diag(np.diag(CR.mat(lam[o:o + k]))))
        o += k
    return cones, lam
