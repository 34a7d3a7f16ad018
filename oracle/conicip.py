"""ORACLE (test infrastructure, NOT product code).

Line-by-line numpy restatement of the reference's interior-point driver
``conicIP`` (src/ConicIP.jl:468-939): Mehrotra predictor-corrector with
Nesterov-Todd scaling, the 4x4 -> 3x3 reduction (``solve4x4gen`` :669-694),
iterative refinement (:907-921) and the infeasibility certificates (:790-852).
Quirks of the reference are kept: ``sol.y/w/v`` alias the
iterate, a factorisation also happens in the terminating iteration, ``rPr``
ignores the equality residual, ``norm(v4x1)`` is a sum of block 2-norms.
"""
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from . import cones
from .block import Block, Diagonal, SymWoodbury, VecCongurance, identity_block
from .kktsolvers import kktsolver_qr


class V4:
    """v4x1 (src/ConicIP.jl:57-66)."""

    def __init__(self, y, w, v, s):
        self.y, self.w, self.v, self.s = y, w, v, s

    def __add__(a, b):
        return V4(a.y + b.y, a.w + b.w, a.v + b.v, a.s + b.s)

    def __sub__(a, b):
        return V4(a.y - b.y, a.w - b.w, a.v - b.v, a.s - b.s)

    def norm(a):
        return sum(np.linalg.norm(t) if len(t) else 0.0 for t in (a.y, a.w, a.v, a.s))


@dataclass
class Solution:
    """src/ConicIP.jl:384-398."""
    y: np.ndarray
    w: np.ndarray
    v: np.ndarray
    status: str = "None"
    Iter: int = 0
    Mu: float = 0.0
    prFeas: float = np.inf
    duFeas: float = np.inf
    muFeas: float = np.inf
    pobj: float = np.inf
    dobj: float = -np.inf
    # oracle-only bookkeeping (not in the reference struct)
    n_factor: int = 0
    n_solve: int = 0
    trace: list = field(default_factory=list)


def _normsafe(x):
    return 0.0 if len(x) == 0 else float(np.linalg.norm(x))


def _cum_ranges(sizes):
    """cum_range (src/ConicIP.jl:158-159), 0-based slices."""
    out, c = [], 0
    for k in sizes:
        out.append(slice(c, c + k))
        c += k
    return out


def cone_identity(cone_dims):
    """e (src/ConicIP.jl:559-565) and conedim (:547-552)."""
    m = sum(k for _, k in cone_dims)
    e = np.zeros(m)
    conedim = 0
    for (t, k), I in zip(cone_dims, _cum_ranges([k for _, k in cone_dims])):
        if t == "R":
            e[I] = 1.0
            conedim += k
        elif t == "Q":
            e[I.start] = 1.0
            conedim += 1
        elif t == "S":
            r = cones.ord_(np.zeros(k))
            e[I] = cones.vecm(np.eye(r))
            conedim += r
        else:
            raise ValueError("unknown cone type %r" % (t,))
    return e, conedim


def make_cone_ops(cone_dims):
    """The cone-dispatch closures of src/ConicIP.jl:571-665."""
    types = [t for t, _ in cone_dims]
    ranges = _cum_ranges([k for _, k in cone_dims])

    def maxstep(x, d):                                        # :571-587
        mn = np.inf
        for t, I in zip(types, ranges):
            xI = x[I]
            dI = None if d is None else d[I]
            if t == "R":
                a = cones.maxstep_rp(xI, dI)
            elif t == "Q":
                a = cones.maxstep_soc(xI, dI)
            else:
                a = cones.maxstep_sdc(xI, dI)
            mn = min(a, mn)
        return mn

    def nt_scaling(x, y):                                     # :589-605
        blocks = []
        for t, I in zip(types, ranges):
            xI, yI = x[I], y[I]
            if t == "R":
                blocks.append(Diagonal(np.sqrt(yI / xI)))     # :598
            elif t == "Q":
                beta, w = cones.nestod_soc(xI, yI)            # :599
                k = len(xI)
                J = np.full(k, beta)
                J[0] = -beta
                blocks.append(SymWoodbury(J, w, 1.0))
            else:
                blocks.append(VecCongurance(cones.nestod_sdc(xI, yI)))   # :600
        return Block(blocks)

    def cone_div(x, y):                                       # :607-635
        o = np.zeros(len(x))
        for t, I in zip(types, ranges):
            if t == "R":
                o[I] = cones.drp(x[I], y[I])
            elif t == "Q":
                o[I] = cones.dsoc(x[I], y[I])
            else:
                o[I] = cones.dsdc(x[I], y[I])
        return o

    def cone_prod(x, y):                                      # :637-665
        o = np.zeros(len(x))
        for t, I in zip(types, ranges):
            if t == "R":
                o[I] = cones.xrp(x[I], y[I])
            elif t == "Q":
                o[I] = cones.xsoc(x[I], y[I])
            else:
                o[I] = cones.xsdc(x[I], y[I])
        return o

    return maxstep, nt_scaling, cone_div, cone_prod


def _nrm(x2):
    """the norm out of its square as the loop's scalar logic takes it: NaN for a negative (or NaN) square"""
    return float(np.sqrt(x2)) if x2 >= 0 else np.nan


def _jldiv(a, b):
    """Julia's float division: x / 0 is +-Inf, 0 / 0 is NaN, no exception"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return float(np.float64(a) / np.float64(b))


@dataclass
class Verdict:
    """what one pass through src/ConicIP.jl:756-873 decides"""
    status: str                  # "None": keep iterating
    scale: float                 # Infeasible: (w, v) / scale, y = NaN ; Unbounded: y / scale, (w, v) = NaN ; else NaN
    mu: float
    rDu: float
    rPr: float
    rCp: float
    pobj: float
    dobj: float
    improved: bool               # this iterate is the best so far (:768): the caller records Iter, mu, rDu, rPr, rCp
    optBest: float               # the running best after this iteration
    p_infeas: float = np.nan
    d_infeas: float = np.nan


def evaluate_iteration(dots, normc, normb, normd, conedim, m, p, optTol, infeasTol, Iter, optBest):
    """src/ConicIP.jl:756-873 on scalars alone: residuals, best-iterate test, objective values and the stopping verdicts in the
    reference's order -- :Optimal is noted (:786), the primal certificate is tested (:815), then the dual one (:847), then a
    noted :Optimal is acted upon (:867), then :Error (:870).  `dots`: the 16 dot products in the order of IterDots
    (csrc/cip_driver_scalars.h); a norm is the square root of its square, NaN where the square is negative or NaN.
    sol.y aliases the iterate (:726), so an :Infeasible verdict NaN-fills z.y and every quantity of the dual test after it is
    NaN: the verdict stands, and the function returns there."""
    (mubar, cTy, r0y2, r0v2, r0s2, yQy, wr0w, vr0v, dTw, bTv, pinf2, yy, vv, ays2, gy2, qy2) = (float(x) for x in dots)
    with np.errstate(all="ignore"):
        mu = _jldiv(mubar, conedim) if conedim > 0 else np.nan    # :756-757 (Julia: 0.0/0 = NaN, no exception)
        rDu = _nrm(r0y2) / (1 + normc)                            # :764
        rPr = (_nrm(r0v2) if m > 0 else 0.0) / (1 + normb)        # :765 (normsafe)
        rCp = (_nrm(r0s2) if m > 0 else 0.0) / (1 + abs(cTy))     # :766
        worst = _jlmax(_jlmax(rDu, rPr), rCp)
        improved = bool(worst < optBest)                          # :768-773
        if improved:
            optBest = worst
        pobj = 0.5 * yQy - cTy                                    # :775
        dobj = pobj + wr0w + vr0v - mubar                         # :776
        vd = Verdict("None", np.nan, mu, rDu, rPr, rCp, pobj, dobj, improved, optBest)

        status = "Optimal" if worst < optTol else "None"          # :786
        if not (p == 0 and m == 0):                               # :790
            dTy_bTv = dTw - bTv                                   # :808
            if dTy_bTv < 0:
                p_unscaled = _nrm(pinf2)                          # :810
                p_cvx = _jldiv(p_unscaled, _nrm(yy) + (_nrm(vv) if m > 0 else 0.0))      # :811
                p_ecos = _jldiv(p_unscaled, _jlmax(1.0, normc) * abs(dTy_bTv))                # :812
                vd.p_infeas = _jlmax(p_cvx, p_ecos)
            if vd.p_infeas < infeasTol:                           # :815-818
                vd.status, vd.scale = "Infeasible", -dTy_bTv
                return vd
            d1 = -np.inf if m == 0 else _nrm(ays2)                # :839
            d2 = -np.inf if p == 0 else _nrm(gy2)                 # :840
            d3 = _nrm(qy2)                                        # :841
            if cTy > 0:
                d_cvx = _jldiv(_jlmax(_jlmax(_jldiv(d1, _jlmax(1.0, normb)), _jldiv(d2, _jlmax(1.0, normd))),
                                      _jldiv(d3, _jlmax(1.0, normc))), abs(cTy))              # :843
                d_ecos = _jldiv(_jlmax(_jlmax(d1, d2), d3), _nrm(yy))                    # :844
                vd.d_infeas = abs(_jlmax(d_cvx, d_ecos))
            if vd.d_infeas < infeasTol:                           # :847-850
                vd.status, vd.scale = "Unbounded", abs(cTy)
                return vd
        if status != "None":                                      # :867
            vd.status = status
        elif not np.all(np.isfinite([mu, rDu, rPr, rCp])):        # :870-873
            vd.status = "Error"
    return vd


def apply_certificate(status, scale, y, w, v):
    """what a verdict does to the returned iterate (:816, :848); every other status returns it as it is"""
    with np.errstate(all="ignore"):
        if status == "Infeasible":
            return np.full(len(y), np.nan), w / scale, v / scale
        if status == "Unbounded":
            return y / scale, np.full(len(w), np.nan), np.full(len(v), np.nan)
    return y, w, v


def conicIP(Q, c, A, b, cone_dims, G=None, d=None, *,
            kktsolver=kktsolver_qr,
            optTol=1e-6, DTB=0.01, verbose=False,
            maxRefinementSteps=3, maxIters=100, cache_nestodd=False,
            infeasTol=None, refinementThreshold=None):
    """src/ConicIP.jl:468-939."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = len(c)
    if G is None:
        G = sp.csr_matrix((0, n))
    if d is None:
        d = np.zeros(0)
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    if infeasTol is None:
        infeasTol = optTol                                    # :506
    if refinementThreshold is None:
        refinementThreshold = optTol / 1e7                    # :509

    m = A.shape[0]
    p = G.shape[0]
    AT = A.T
    GT = G.T

    normc = float(np.linalg.norm(c))
    normd = -np.inf if len(d) == 0 else float(np.linalg.norm(d))
    normb = _normsafe(b)

    # sanity checks :537-542
    if Q.shape[0] != Q.shape[1]:
        raise ValueError("Q is not square")
    if len(b) != m:
        raise ValueError("Inconsistency in inequalities")
    if Q.shape[0] != n or A.shape[1] != n:
        raise ValueError("Inconsistency in inequalities/objective")
    if len(d) != p:
        raise ValueError("Inconsistency in equalities")
    if G.shape[1] != n:
        raise ValueError("Inconsistency in equalities/objective")
    if sum(k for _, k in cone_dims) != m:
        raise ValueError("cone_dims do not cover the rows of A")

    block_sizes = [k for _, k in cone_dims]
    e, conedim = cone_identity(cone_dims)
    maxstep, nt_scaling, cone_div, cone_prod = make_cone_ops(cone_dims)

    solve3x3gen = kktsolver(Q, A, G, cone_dims)               # :667
    counts = {"factor": 0, "solve": 0}

    def solve4x4gen(lam, F, FinvT):                           # :669-694
        solve3x3 = solve3x3gen(F, FinvT)                      # :682
        counts["factor"] += 1

        def solve4x4(r):
            counts["solve"] += 1
            q = cone_div(r.s, lam)                            # :686
            t1 = F.tmul(q)                                    # :687
            dy, dw, dv = solve3x3(r.y, r.w, r.v + t1)         # :688
            t1 = t1 - F.tmul(F.mul(dv))                       # :689
            return V4(np.array(dy, dtype=np.float64), np.array(dw, dtype=np.float64),
                      np.array(dv, dtype=np.float64), t1)

        return solve4x4

    # initial point :704-713
    I = identity_block(block_sizes)
    r0 = V4(c, d, b, np.zeros(m))
    z = solve4x4gen(e, I, I)(r0)
    a_v = maxstep(z.v, None)
    a_s = maxstep(z.s, None)
    z.v = z.v - a_v * e
    z.s = z.s - a_s * e

    sol = Solution(z.y, z.w, z.v)                             # :726 (aliases z)
    optBest = np.inf
    for Iter in range(1, maxIters + 1):                       # :730
        F = nt_scaling(z.v, z.s)                              # :732
        FinvT = F.inv_adjoint()                               # :733
        lam = F.mul(z.v)                                      # :735
        solve = solve4x4gen(lam, F, FinvT)                    # :737

        lamlam = cone_prod(lam, lam)                          # :746
        Qy = Q @ z.y
        rleft = V4(Qy + GT @ z.w - AT @ z.v, G @ z.y, A @ z.y - z.s, lamlam)   # :747-750
        r0 = V4(rleft.y - c, rleft.w - d, rleft.v - b, rleft.s)               # :753

        # the scalars of :756-873: 16 dot products (the order of csrc/cip_driver_scalars.h: IterDots); every norm the block
        # takes is the square root of one of them (numpy's 2-norm of a vector is sqrt(dot(x, x)), bit for bit)
        pinf = GT @ z.w - AT @ z.v                            # :810
        sq = lambda x: float(np.dot(x, x))
        dots = (float(np.dot(z.v, z.s)), float(np.dot(c, z.y)), sq(r0.y), sq(r0.v), sq(r0.s), float(np.dot(z.y, Qy)),
                float(np.dot(z.w, r0.w)), float(np.dot(z.v, r0.v)), float(np.dot(d, z.w)), float(np.dot(b, z.v)), sq(pinf),
                sq(z.y), sq(z.v), sq(rleft.v), sq(rleft.w),                 # A y - s (:839), G y (:840)
                sq(Qy) if np.all(np.isfinite(z.y)) else np.nan)                  # :841
        vd = evaluate_iteration(dots, normc, normb, normd, conedim, m, p, optTol, infeasTol, Iter, optBest)
        optBest = vd.optBest
        if vd.improved:                                       # :768-773
            sol.Iter, sol.Mu = Iter, vd.mu
            sol.duFeas, sol.prFeas, sol.muFeas = vd.rDu, vd.rPr, vd.rCp
        sol.pobj, sol.dobj = vd.pobj, vd.dobj
        sol.trace.append(dict(Iter=Iter, mu=vd.mu, rDu=vd.rDu, rPr=vd.rPr, rCp=vd.rCp, pobj=vd.pobj, dobj=vd.dobj))
        mu, mubar = vd.mu, dots[0]

        if vd.status != "None":                               # :815-818, :847-850, :867, :870-873
            sol.status = vd.status
            sol.n_factor, sol.n_solve = counts["factor"], counts["solve"]
            sol.y, sol.w, sol.v = apply_certificate(vd.status, vd.scale, z.y, z.w, z.v)
            return sol

        # predictor :879-887
        d_aff = solve(r0)
        a_aff_v = min(maxstep(z.v, d_aff.v), 1)
        a_aff_s = min(maxstep(z.s, d_aff.s), 1)
        a_aff = min(a_aff_v, a_aff_s)
        rho = cones.fts(z.v, a_aff, d_aff.v, z.s, a_aff, d_aff.s) / mubar
        sigma = max(0, min(1, rho)) ** 3

        # corrector :893-901
        FiTdfs = FinvT.mul(d_aff.s)
        Fdfs = F.mul(d_aff.v)
        lc = cone_prod(FiTdfs, Fdfs)
        lc = -(lc - sigma * mu * e)
        r = V4(r0.y, r0.w, r0.v, rleft.s - lc)

        # newton step + refinement :907-921
        dz = solve(r)
        sol.trace[-1]["rnorm"] = []                           # oracle-only: every refinement residual this iteration tests
        for rStep in range(1, maxRefinementSteps + 1):
            pb1 = cone_prod(lam, F.mul(dz.v))
            pb2 = cone_prod(lam, FinvT.mul(dz.s))
            rkkt = V4(Q @ dz.y + GT @ dz.w - AT @ dz.v, G @ dz.y, A @ dz.y - dz.s, pb1 + pb2)
            rIr = r - rkkt
            rnorm = rIr.norm() / (n + 2 * m)
            sol.trace[-1]["rnorm"].append(float(rnorm))
            if rnorm < refinementThreshold:
                break
            dzr = solve(rIr)
            dz = dz + dzr

        # step :927-932
        a_v = min(maxstep(z.v, dz.v / (1 - DTB)), 1)
        a_s = min(maxstep(z.s, dz.s / (1 - DTB)), 1)
        alpha = min(a_v, a_s)
        z.y = z.y - alpha * dz.y
        z.w = z.w - alpha * dz.w
        z.v = z.v - alpha * dz.v
        z.s = z.s - alpha * dz.s
        sol.trace[-1]["alpha"] = alpha
        sol.trace[-1]["sigma"] = sigma

    sol.status = "Abandoned"                                  # :936
    sol.n_factor, sol.n_solve = counts["factor"], counts["solve"]
    sol.y, sol.w, sol.v = z.y, z.w, z.v
    return sol


def _jlmax(a, b):
    """Julia's max propagates NaN."""
    if np.isnan(a) or np.isnan(b):
        return np.nan
    return max(a, b)
