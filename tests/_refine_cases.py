"""The case table of the refinement tests (tests/test_refine_cases.py without a GPU, tests/test_gpu_refinement.py with one).

The Newton step's iterative refinement (src/ConicIP.jl:907-921; oracle/conicip.py; csrc/driver.hip; cipkkt/driver.py) compares a
rounding-level quantity, `rnorm`, with a threshold T.  With the default T = optTol / 1e7 whether a problem refines is an accident
of its data, so every case here carries an explicit T and a data scale (c, b and d multiplied by it: `rnorm` scales with the
data, T does not) that put every `rnorm` of the whole run far from T.

Margin rule.  A (case, maxRefinementSteps) pair is admissible only if no `rnorm` the ORACLE records in the run with that T in
effect lies in [T / 100, 100 T].  It is a condition on the inputs, checked on the oracle alone (tests/test_refine_cases.py); the
device's residuals differ from the oracle's by rounding of another factorisation, and two decades keep the decisions -- and with
them the solve counts -- reproducible.  T = 0.0 (forced: every step refines to the full depth) and T = 1e300 (never) are exempt.

How the table was found: for each shape, seeds and scales 1e-4 .. 1e12 were run forced at depth 3, every gap of five decades or
more in the sorted residuals gave a candidate T, and a candidate stayed if the margin held at depths 1, 2 and 3.  The all-R
shapes refine to rounding in one or two steps at every scale, so no threshold between "all" and "none" is admissible for them:
their high-scale cases have T = None and run forced and never only.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

import problems as P
from oracle.conicip import conicIP as oracle_conicIP

OPT = 1e-7
DEPTHS = (0, 1, 2, 3)
FORCED, NEVER = 0.0, 1e300
MARGIN = 100.0

# tests/test_gpu_vecops.py: LOOP -- n + p + 2 m fills four workgroups of the loop's fused kernels, sections start at 300 / 307 / 607
_ALL_R = dict(n=300, nq=0, kq=0, p=7)
_WITH_Q = dict(n=300, nq=3, kq=6, p=7)
_SMALL_Q = dict(n=40, nq=3, kq=6, p=4)
_SMALL_Q_P0 = dict(n=40, nq=3, kq=6, p=0)
_SMALL_R = dict(n=40, nq=0, kq=0, p=4)

# name -> family, builder arguments, data scale, T (None: no admissible threshold, forced / never only), route.
# `depths`: what the oracle's run with T and maxRefinementSteps = 3 does (tests/test_refine_cases.py asserts it): "none" -- no
# refinement in any iteration, "full" -- 3 in every iteration that steps, "partial" -- some iteration strictly between 0 and 3.
CASES = {
    "all_r_dense_1e-4": dict(family="mixed", kw=dict(_ALL_R, dense_A=True), scale=1e-4, T=1e-12, route="schur", depths="none"),
    "all_r_dense_1e6": dict(family="mixed", kw=dict(_ALL_R, dense_A=True), scale=1e6, T=None, route="schur", depths=None),
    "all_r_csr_1e-4": dict(family="mixed", kw=dict(_ALL_R, dense_A=False), scale=1e-4, T=1e-12, route="schur", depths="none"),
    "all_r_csr_1e6": dict(family="mixed", kw=dict(_ALL_R, dense_A=False), scale=1e6, T=None, route="full3x3", depths=None),
    "q_cones_1e-4": dict(family="mixed", kw=dict(_WITH_Q, dense_A=True), scale=1e-4, T=1e-12, route="schur", depths="none"),
    "q_cones_1e9_schur": dict(family="mixed", kw=dict(_WITH_Q, dense_A=True), scale=1e9, T=1e-12, route="schur", depths="full"),
    "q_cones_1e9_full3x3": dict(family="mixed", kw=dict(_WITH_Q, dense_A=True), scale=1e9, T=1e-12, route="full3x3", depths="full"),
    "small_q_1e12_partial": dict(family="mixed", kw=dict(_SMALL_Q, seed=100), scale=1e12, T=1e14, route="full3x3", depths="partial"),
    "small_q_p0_1e-4": dict(family="mixed", kw=dict(_SMALL_Q_P0, seed=100), scale=1e-4, T=1e-12, route="schur", depths="none"),
    "small_q_p0_1e9": dict(family="mixed", kw=dict(_SMALL_Q_P0, seed=100), scale=1e9, T=1e-12, route="schur", depths="full"),
    "psd_1": dict(family="psd", kw={}, scale=1.0, T=1e-12, route="schur", depths="none"),
    "psd_1e6": dict(family="psd", kw={}, scale=1e6, T=None, route="schur", depths=None),
}


def box(seed, scale, cmul=1.0, n=10):
    """-5 scale <= y <= 5 scale behind a CSR A = [I; -I], the feasible family of
    tests/test_gpu_lockstep.py::test_statuses_differ_inside_one_group; cmul = 50 pushes the optimum onto the bounds"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n)
    H = np.outer(h, h) + 0.1 * np.eye(n)
    A = sp.vstack([sp.identity(n), -sp.identity(n)]).tocsr()
    return H, rng.standard_normal(n) * (cmul * scale), A, -5.0 * scale * np.ones(2 * n), [("R", 2 * n)], None, None


def build(family, kw, scale):
    """(Q, c, A, b, cone_dims, G, d) with c, b and d multiplied by `scale`"""
    if family == "mixed":
        Q, c, A, b, K, G, d = P.random_mixed(**kw)[:7]
    elif family == "psd":
        Q, c, A, b, K, G, d = P.psd_projection()[:7]
    elif family == "infeasible_box":
        Q, c, A, b, K, G, d = P.infeasible_box(**kw)[:7]
    elif family == "box":
        return box(scale=scale, **kw)
    else:
        raise KeyError(family)
    if sp.issparse(Q):
        Q = Q.toarray()
    return Q, c * scale, A, b * scale, K, G, (None if d is None else d * scale)


def case_problem(name):
    cs = CASES[name]
    return build(cs["family"], cs["kw"], cs["scale"])


def thresholds(name):
    """the refinementThreshold values of the sweep for one case"""
    T = CASES[name]["T"]
    return (FORCED, NEVER) + (() if T is None else (T,))


_MEMBER = lambda family, scale, **kw: dict(family=family, kw=kw, scale=scale)
# Lock-step groups: 6 to 8 problems of one shape under ONE explicit T, members that refine in every step next to members that
# never do.  The members are chosen so that the longest-running refining member and the longest-running other one take their
# last step in the same iteration: in every iteration in which the group steps, the refining set is a non-empty strict subset of
# the stepping set (tests/test_refine_cases.py asserts it on the oracle), and some member stops before the rest.
GROUPS = {
    # n = 40, p = 4, dense A, R cones only: the loop's cone terms are fused into its vector kernels
    # (depth 1 only: at depth 3 these problems refine down to rounding, see `member_steady`)
    "all_r_dense_k1": dict(T=1e-12, k=1, route="schur", members=[
        _MEMBER("mixed", 1e-4, **_SMALL_R, seed=100), _MEMBER("mixed", 1e9, **_SMALL_R, seed=102),
        _MEMBER("mixed", 1e9, **_SMALL_R, seed=103), _MEMBER("mixed", 1e-4, **_SMALL_R, seed=101),
        _MEMBER("mixed", 1e9, **_SMALL_R, seed=104), _MEMBER("mixed", 1e-4, **_SMALL_R, seed=102)]),
    # n = 10, m = 20, p = 0, CSR A, R cones only; one member is infeasible (y >= 1e9 and y <= -1e9) and refines until it is certified
    "all_r_csr_k3": dict(T=1e-12, k=3, route="schur", members=[
        _MEMBER("box", 1e-4, seed=3, cmul=50.0), _MEMBER("box", 1e9, seed=4), _MEMBER("infeasible_box", 1e9, n=10, seed=0),
        _MEMBER("box", 1e-3, seed=3, cmul=50.0), _MEMBER("box", 1e9, seed=3), _MEMBER("box", 1e-4, seed=4, cmul=50.0),
        _MEMBER("box", 1e9, seed=7)]),
    "all_r_csr_k1": dict(T=1e-12, k=1, route="schur", members=[
        _MEMBER("box", 1e-4, seed=3, cmul=50.0), _MEMBER("box", 1e9, seed=4), _MEMBER("infeasible_box", 1e9, n=10, seed=0),
        _MEMBER("box", 1e-3, seed=3, cmul=50.0), _MEMBER("box", 1e9, seed=7), _MEMBER("box", 1e-4, seed=4, cmul=50.0)]),
    # n = 40, p = 4, three Q cones.  Scales 1 and 1e12 under T = 1e-7: with 1e-4 and 1e9 under 1e-12 the members that do not refine
    # need 12 to 15 iterations and the refining ones 8 to 11, so the refining set would be empty in the group's last iterations
    "q_cones_k3": dict(T=1e-7, k=3, route="schur", members=[
        _MEMBER("mixed", 1.0, **_SMALL_Q, seed=101), _MEMBER("mixed", 1e12, **_SMALL_Q, seed=103),
        _MEMBER("mixed", 1e12, **_SMALL_Q, seed=100), _MEMBER("mixed", 1.0, **_SMALL_Q, seed=104),
        _MEMBER("mixed", 1e12, **_SMALL_Q, seed=111), _MEMBER("mixed", 1.0, **_SMALL_Q, seed=103)]),
    # (Schur route as well.  On the literal 3x3 route a member that never refines is not comparable with the oracle: without
    # refinement that route's solves leave residuals a thousand times the Schur route's -- seed 103 at scale 1 reaches 3.9e-8 where
    # the oracle has 6e-12 -- and the member needs 13 iterations instead of 11 under any threshold that keeps it from refining.
    # DESIGN_LOG.md has the figures; the one-problem cases above run that route at every depth.)
    "q_cones_k1": dict(T=1e-7, k=1, route="schur", members=[
        _MEMBER("mixed", 1.0, **_SMALL_Q, seed=101), _MEMBER("mixed", 1e12, **_SMALL_Q, seed=103),
        _MEMBER("mixed", 1e12, **_SMALL_Q, seed=100), _MEMBER("mixed", 1.0, **_SMALL_Q, seed=104),
        _MEMBER("mixed", 1e12, **_SMALL_Q, seed=111), _MEMBER("mixed", 1.0, **_SMALL_Q, seed=103)]),
    # forced, depth 0: T = 0.0 asks for refinement everywhere and maxRefinementSteps = 0 never enters the block
    # (scales 1e-4 and 1e6: an unrefined run at 1e9 or above is not steady, see `member_steady`)
    "q_cones_forced_k0": dict(T=FORCED, k=0, route="schur", members=[
        _MEMBER("mixed", 1e-4, **_SMALL_Q, seed=101), _MEMBER("mixed", 1e6, **_SMALL_Q, seed=103),
        _MEMBER("mixed", 1e6, **_SMALL_Q, seed=100), _MEMBER("mixed", 1e-4, **_SMALL_Q, seed=104),
        _MEMBER("mixed", 1e6, **_SMALL_Q, seed=104), _MEMBER("mixed", 1e-4, **_SMALL_Q, seed=103)]),
}


def group_problems(name):
    return [build(mb["family"], mb["kw"], mb["scale"]) for mb in GROUPS[name]["members"]]


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _freeze(x):
    return tuple(sorted((k, _freeze(v)) for k, v in x.items())) if isinstance(x, dict) else x


@functools.lru_cache(maxsize=None)
def _oracle(family, kw, scale, T, k, max_iters, solver="qr"):
    from oracle.kktsolvers import kktsolver_2x2, kktsolver_qr, pivot
    return oracle_conicIP(*build(family, dict(kw), scale), optTol=OPT, refinementThreshold=T, maxRefinementSteps=k, maxIters=max_iters,
                          kktsolver=kktsolver_qr if solver == "qr" else pivot(kktsolver_2x2))


def oracle_run(name, T, k, max_iters=100):
    """the oracle on a case of CASES; computed once per (case, T, k) and shared -- callers do not modify it"""
    return oracle_member(case_member(name), T, k, max_iters)


def oracle_member(mb, T, k, max_iters=100, solver="qr"):
    if k == 0:
        T = FORCED                  # depth 0 never looks at the threshold: one run serves all of them
    elif T == NEVER:
        k = 1                       # the first residual ends the loop at every depth
    return _oracle(mb["family"], _freeze(mb["kw"]), mb["scale"], T, k, max_iters, solver)


def has_second_solver(mb):
    """the oracle's 2x2 elimination (oracle/kktsolvers.py: pivot(kktsolver_2x2)) does not take S cones"""
    return mb["family"] != "psd"


STEADY = 1e-4


def member_steady(mb, T, k):
    """Steadiness rule, the second condition on the inputs (oracle alone): the counts of a run are compared with the oracle's only
    where the oracle's own counts do not depend on how the Newton system was solved.
      1. The oracle has two KKT solvers, a QR-based one and a 2x2 elimination, that differ in rounding only.  Both must give the
         same status, Iter, n_factor and n_solve (and both must respect the margin rule: tests/test_refine_cases.py).  R-cone
         problems at data scale 1e9 refine down to rounding by depth 3, so under T = 1e-12 their last residuals land next to T
         under one solver or the other, and their counts differ between the two: such runs are not used.
      2. mu agrees with the oracle's forced depth-3 run of the same problem row by row within 1e-4.  Where a run leaves a large
         residual unrefined -- depth 0, or a threshold above the residuals, at data scales of 1e9 and more -- the error of the solve
         steers the trajectory: the oracle's own iteration count then depends on the depth (11 or 13 rows against 9 or 11).  The
         runs of this table fall into two groups, at most 1e-5 and at least 9e-3 (or another number of rows)."""
    run, base = oracle_member(mb, T, k), oracle_member(mb, FORCED, 3)
    if len(run.trace) != len(base.trace):
        return False
    if not all(abs(a["mu"] - b["mu"]) <= STEADY * abs(b["mu"]) for a, b in zip(run.trace, base.trace)):
        return False
    if has_second_solver(mb):
        other = oracle_member(mb, T, k, solver="2x2")
        if (run.status, run.Iter, run.n_factor, run.n_solve) != (other.status, other.Iter, other.n_factor, other.n_solve):
            return False
    return True


def member_margin(mb, T, k):
    """the margin of a run under every solver the oracle has for it"""
    return min(margin(rnorms(oracle_member(mb, T, k, solver=sv)), T) for sv in (("qr", "2x2") if has_second_solver(mb) else ("qr",)))


def case_member(name):
    cs = CASES[name]
    return dict(family=cs["family"], kw=cs["kw"], scale=cs["scale"])


def steady(name, T, k):
    return member_steady(case_member(name), T, k)


def solves_per_iteration(sol, T):
    """refinement solves of every trace row of an oracle run: a residual that is not below T is followed by a solve"""
    return [sum(1 for r in row.get("rnorm", ()) if not r < T) for row in sol.trace]


def rnorms(sol):
    return [r for row in sol.trace for r in row.get("rnorm", ())]


def margin(values, T):
    """the smallest factor between T and a recorded residual (inf for the exempt thresholds and for no residuals at all).
    An exactly zero residual is infinitely far below T"""
    if T in (FORCED, NEVER):
        return math.inf
    return min((math.inf if r == 0.0 else max(r / T, T / r) for r in values), default=math.inf)


def closed_form(rows, k, stopped=True):
    """n_solve of a run that refines to depth k in every step: the initial point, then predictor + Newton step + k refinement
    solves per stepping row.  The terminating row of a run that stopped factors but does not solve; an abandoned run steps in
    every row"""
    return 1 + (rows - 1 if stopped else rows) * (2 + k)
