"""The case table of the stopping tests (tests/test_stop_cases.py without a GPU, tests/test_gpu_stopping.py with one).

The interior-point loop (src/ConicIP.jl:730-936; oracle/conicip.py; csrc/driver.hip; cipkkt/driver.py) ends :Optimal, :Infeasible,
:Unbounded, :Abandoned or :Error.  Every case here is a tiny problem (n <= 12: the point is the branch, not the size) whose end
state, number of iterations and best-iterate index are written in the table and asserted on the ORACLE in
tests/test_stop_cases.py, before a GPU is involved.  :Error needs non-finite data and is tested on scalars alone
(tests/test_stop_verdict.py).

Tolerance rule.  The iterates of an infeasible or unbounded problem diverge by design, so the 1e-6 of the :Optimal comparisons
does not transfer.  The oracle has two KKT solvers that are equal in exact arithmetic, a QR-based one and the 2x2 elimination
pivot(kktsolver_2x2) (no S cone: the S-cone case takes the sparse 3x3 solver as its second one), and its sums depend on the
kernels the host's BLAS picks for the CPU.  `measured` is the largest relative difference (`deviation` below) between ANY two of
the ten runs of a case -- two solvers under five OpenBLAS kernel sets (OPENBLAS_CORETYPE = Prescott, Nehalem, Sandybridge,
Haswell, SkylakeX; Zen runs Haswell's) -- as `python tests/_stop_spread.py` prints it, copied here as printed.  One figure per
group of quantities: the blocks of the returned iterate; pobj and dobj; Mu and the three feasibilities.  dobj of a diverging
iterate is worth six to seven digits where the certificate is worth thirteen and Mu fourteen, so one figure for all would
loosen every check to dobj's.  The spread of a case is MARGIN = 4 x measured (a kernel set that is not among the five; over the
five the figures of one solver pair move by up to 10 x), and the tolerance 10 x max(spread, 1e-12), per group.
tests/test_stop_cases.py measures the host's own two-solver spread again and asserts it is below the spread.

What carries no check: a feasibility is measured against the largest of the three (what the loop tests is their maximum), so
one that is itself below tolerance x largest could be anything below that; `unchecked` names those per case (asserted on the
oracle).  pobj is measured against max(|pobj|, |dobj|): on a diverging iterate it is the small difference of two large terms,
and where |pobj| is below tolerance x |dobj| it is named in `unchecked` too.  tests/test_gpu_stopping.py compares all of them bit
for bit between the two drivers, and tests/test_stop_verdict.py within 2 ulp on scalars."""
import functools
import math

import numpy as np
import scipy.sparse as sp

import problems as P
from oracle import cones as OC
from oracle.conicip import conicIP as oracle_conicIP

FIELDS = ("Mu", "prFeas", "duFeas", "muFeas", "pobj", "dobj")
FLOOR = 1e-12
MARGIN = 4.0
GROUPS = dict(iterate=("y", "w", "v"), objective=("pobj", "dobj"), state=("Mu", "prFeas", "duFeas", "muFeas"))


# ---------------------------------------------------------------------------------------------------------------- the problems
def infeasible_soc():
    """y in the Q cone of dimension 4 (A = I, b = 0) and y0 = -1"""
    n = 4
    G = np.zeros((1, n))
    G[0, 0] = 1.0
    return np.eye(n), np.array([1.0, 2.0, -1.0, 0.5]), sp.identity(n, format="csr"), np.zeros(n), [("Q", n)], G, np.array([-1.0])


def infeasible_psd():
    """mat(y) positive semidefinite of order 3 (A = I, b = 0) and tr mat(y) = -1"""
    n = 6
    G = OC.vecm(np.eye(3)).reshape(1, n)
    return np.eye(n), np.arange(1.0, n + 1) / n, sp.identity(n, format="csr"), np.zeros(n), [("S", n)], G, np.array([-1.0])


def infeasible_mixed():
    """R + Q, p = 0: y0 >= 1 and y0 <= -1 inside a problem that is feasible without either of the two rows
    (y1 .. y3 >= 0, (y4 + 2, y5, y6, y7) in the Q cone of dimension 4)"""
    n = 8
    R = np.zeros((5, n))
    R[0, 0], R[1, 0] = 1.0, -1.0
    R[2, 1] = R[3, 2] = R[4, 3] = 1.0
    A = np.vstack([R, np.eye(n)[4:]])
    b = np.concatenate([[1.0, 1.0, 0.0, 0.0, 0.0], [-2.0, 0.0, 0.0, 0.0]])
    rng = np.random.default_rng(5)
    M = rng.standard_normal((n, n))
    return M.T @ M / n + 0.1 * np.eye(n), rng.standard_normal(n), A, b, [("R", 5), ("Q", 4)], None, None


def unbounded_singular_q(n=6):
    """Q = diag(1, 0, .., 0), y >= 0, c with weight in the null space of Q: along the ray Qy -> 0 is what decides"""
    Q = np.zeros((n, n))
    Q[0, 0] = 1.0
    return Q, np.arange(1.0, n + 1), sp.identity(n, format="csr"), np.zeros(n), [("R", n)], None, None


def unbounded_eq(n=6):
    """an LP over y >= 0 whose equality y0 = y1 cuts the recession cone: the ray has to satisfy Gy = 0"""
    G = np.zeros((1, n))
    G[0, 0], G[0, 1] = 1.0, -1.0
    return np.zeros((n, n)), np.arange(1.0, n + 1), sp.identity(n, format="csr"), np.zeros(n), [("R", n)], G, np.array([0.0])


def unbounded_soc():
    """an LP over the Q cone of dimension 4 with c in its interior"""
    n = 4
    return np.zeros((n, n)), np.array([2.0, 1.0, -0.5, 0.5]), sp.identity(n, format="csr"), np.zeros(n), [("Q", n)], None, None


def lockstep_boxes(n=10, count=3):
    """-5 <= y <= 5 behind a CSR A = [I; -I], drawn one after the other from one generator: the feasible members of
    tests/test_gpu_lockstep.py::test_statuses_differ_inside_one_group"""
    rng = np.random.default_rng(3)
    out = []
    for _ in range(count):
        h = rng.standard_normal(n)
        H = np.outer(h, h) + 0.1 * np.eye(n)
        A = sp.vstack([sp.identity(n), -sp.identity(n)]).tocsr()
        out.append((H, rng.standard_normal(n), A, -5 * np.ones(2 * n), [("R", 2 * n)], None, None))
    return out


def _unbounded_box(n=10):
    """the shape of the box problems (n = 10, m = 20, p = 0, CSR A) without an upper bound: y >= 0 and y >= -1, Q = 0"""
    A = sp.vstack([sp.identity(n), sp.identity(n)]).tocsr()
    return np.zeros((n, n)), np.arange(1.0, n + 1), A, np.concatenate([np.zeros(n), -np.ones(n)]), [("R", 2 * n)], None, None


BUILDERS = dict(infeasible_box=lambda **kw: P.infeasible_box(**kw)[:7], infeasible_eq=lambda **kw: P.infeasible_eq(**kw)[:7],
                infeasible_soc=infeasible_soc, infeasible_psd=infeasible_psd, infeasible_mixed=infeasible_mixed,
                unbounded=lambda **kw: P.unbounded(**kw)[:7], unbounded_singular_q=unbounded_singular_q, unbounded_eq=unbounded_eq,
                unbounded_soc=unbounded_soc, simplex=lambda **kw: P.simplex(**kw)[:7], box=lambda i: lockstep_boxes()[i], unbounded_box=_unbounded_box)

# Every case refines every Newton step to the full depth (refinementThreshold = 0.0).  With the derived default, optTol / 1e7 =
# 1e-13, whether a step refines is an accident of rounding on these problems -- the oracle's residuals pass the threshold at
# factors of 1.04 to 7, and its two solvers already disagree on n_solve for the S-cone case -- so n_solve could not be compared.
# tests/test_gpu_refinement.py is where the threshold itself is tested, with margins.
BASE = dict(optTol=1e-6, refinementThreshold=0.0)
LOOSE = dict(infeasTol=1e-3, optTol=1e-9)                                  # tolerances apart
# name -> builder, its arguments, options beyond BASE, and what the oracle does with it (tests/test_stop_cases.py asserts
# it): end state, trace rows (the stopping iteration), Iter (the best iterate's index).  `routes`: Q = 0 stays on the Schur route,
# as tests/test_gpu_driver.py::test_unbounded_status does.  `second`: the oracle's second solver.  `measured` (iterate, objective, state) and `unchecked`: see the module text.
CASES = {
    "infeasible_box": dict(builder="infeasible_box", kw=dict(n=10, seed=0), opts={}, status="Infeasible", rows=6, Iter=2,
                           routes=("schur", "full3x3"), second="2x2", measured=(2.9e-13, 8.3e-08, 2.8e-14), unchecked=('duFeas', 'pobj')),
    "infeasible_eq": dict(builder="infeasible_eq", kw=dict(n=10, seed=0), opts={}, status="Infeasible", rows=4, Iter=3,
                          routes=("schur", "full3x3"), second="2x2", measured=(2.2e-16, 2e-14, 4.5e-15), unchecked=()),
    "infeasible_soc": dict(builder="infeasible_soc", kw={}, opts={}, status="Infeasible", rows=7, Iter=2,
                           routes=("schur", "full3x3"), second="2x2", measured=(7e-14, 2.3e-07, 1.6e-15), unchecked=('pobj',)),
    "infeasible_psd": dict(builder="infeasible_psd", kw={}, opts={}, status="Infeasible", rows=7, Iter=3,
                           routes=("schur", "full3x3"), second="sparse", measured=(8.9e-15, 1e-06, 3.3e-14), unchecked=('pobj',)),
    "infeasible_mixed": dict(builder="infeasible_mixed", kw={}, opts={}, status="Infeasible", rows=6, Iter=2,
                             routes=("schur", "full3x3"), second="2x2", measured=(5.2e-18, 1.6e-08, 2.8e-15), unchecked=('pobj',)),
    "unbounded": dict(builder="unbounded", kw=dict(n=10), opts={}, status="Unbounded", rows=1, Iter=1,
                      routes=("schur",), second="2x2", measured=(0.0, 0.0, 1.6e-17), unchecked=('prFeas',)),
    "unbounded_singular_q": dict(builder="unbounded_singular_q", kw={}, opts={}, status="Unbounded", rows=4, Iter=4,
                                 routes=("schur", "full3x3"), second="2x2", measured=(1.7e-16, 1.9e-16, 1.9e-23), unchecked=('prFeas',)),
    "unbounded_eq": dict(builder="unbounded_eq", kw={}, opts={}, status="Unbounded", rows=1, Iter=1,
                         routes=("schur",), second="2x2", measured=(3.3e-17, 0.0, 3.4e-17), unchecked=('prFeas',)),
    "unbounded_soc": dict(builder="unbounded_soc", kw={}, opts={}, status="Unbounded", rows=1, Iter=1,
                          routes=("schur",), second="2x2", measured=(0.0, 0.0, 0.0), unchecked=('prFeas',)),
    "abandoned_1": dict(builder="simplex", kw=dict(n=10), opts=dict(maxIters=1), status="Abandoned", rows=1, Iter=1,
                        routes=("schur", "full3x3"), second="2x2", measured=(1.7e-15, 1.3e-15, 1.3e-15), unchecked=()),
    "abandoned_3": dict(builder="simplex", kw=dict(n=10), opts=dict(maxIters=3), status="Abandoned", rows=3, Iter=3,
                        routes=("schur", "full3x3"), second="2x2", measured=(1.9e-15, 3.6e-16, 1e-14), unchecked=('prFeas', 'duFeas')),
    "infeasible_box_loose": dict(builder="infeasible_box", kw=dict(n=10, seed=0), opts=LOOSE, status="Infeasible", rows=4, Iter=2,
                                 routes=("schur", "full3x3"), second="2x2", measured=(2.8e-14, 2e-12, 2.8e-14), unchecked=('duFeas',)),
    "unbounded_box_loose": dict(builder="unbounded_box", kw={}, opts=LOOSE, status="Unbounded", rows=4, Iter=4,
                                routes=("schur",), second="2x2", measured=(1.4e-16, 5.1e-14, 9.4e-15), unchecked=()),
}
# Iterations the loose infeasTol saves: against infeasTol = optTol = 1e-9, and against the default tolerances (the case of the
# same problem).  The dual certificate converges quadratically: no unbounded LP or QP that was tried (this one, b scaled by 1e3 ..
# 1e6, singular Q scaled by 1 .. 100) saves more than ONE iteration against the default, where the issue says several.
EARLIER = {"infeasible_box_loose": (3, 2, "infeasible_box"), "unbounded_box_loose": (2, 1, "unbounded_box")}

# One lock-step group (n = 10, m = 20, p = 0, CSR A, R cones) that holds every end state a group can reach, behind the six
# members of tests/test_gpu_lockstep.py::test_statuses_differ_inside_one_group.  The options are the group's: maxIters = 9 lets
# every other member finish (5 to 9 iterations) and abandons the narrowly infeasible box (y >= 1e-6 and y <= -1e-6 is certified
# in iteration 11), whose best iterate is that of iteration 6.  (Abandoned at 10, one iteration before its certificate, the
# oracle's own runs of that member differ by 2e-3 in y.)
GROUP_OPTS = dict(maxIters=9, **BASE)
GROUP_EXTRA = {
    "optimal_box": dict(builder="box", kw=dict(i=0), status="Optimal", rows=7, Iter=7, measured=(1.4e-14, 2.4e-15, 6.7e-08), unchecked=('prFeas', 'duFeas')),
    "unbounded_box": dict(builder="unbounded_box", kw={}, status="Unbounded", rows=5, Iter=5, measured=(1.4e-16, 4.2e-13, 3.2e-11), unchecked=()),
    "narrow_infeasible_box": dict(builder="narrow_infeasible_box", kw={}, status="Abandoned", rows=9, Iter=6, measured=(8.4e-06, 1.5e-09, 1.3e-10), unchecked=('duFeas', 'pobj')),
}
# position in the group of tests/test_gpu_lockstep.py::test_statuses_differ_inside_one_group -> the case it is compared as
GROUP_MEMBERS = {0: "infeasible_box", 3: "optimal_box", 6: "unbounded_box", 7: "narrow_infeasible_box"}


def group_tail():
    """the members this table adds behind the six of that test, as problems of cipkkt.batch"""
    keys = ("Q", "c", "A", "b", "cone_dims", "G", "d")
    return [dict(zip(keys, case_problem(name)), kwargs=dict(GROUP_OPTS)) for name in ("unbounded_box", "narrow_infeasible_box")]


def _narrow_infeasible_box(n=10, eps=1e-6):
    Q, c, A, b, K, G, d = P.infeasible_box(n, 0)[:7]
    return Q, c, A, eps * b, K, G, d


BUILDERS["narrow_infeasible_box"] = _narrow_infeasible_box


def case_problem(name):
    cs = case(name)
    return BUILDERS[cs["builder"]](**cs["kw"])


def case_options(name):
    return dict(BASE, **(CASES[name]["opts"] if name in CASES else GROUP_OPTS))


def case(name):
    return CASES.get(name) or GROUP_EXTRA[name]


def allowed_spread(name):
    """{group: MARGIN x measured}"""
    return {g: MARGIN * x for g, x in zip(GROUPS, case(name)["measured"])}


def tolerance(name):
    """{group: 10 x max(spread, 1e-12)}"""
    return {g: 10.0 * max(x, FLOOR) for g, x in allowed_spread(name).items()}


# ---------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def _oracle(name, solver, opts):
    from oracle import kktsolvers as KS
    sv = dict(qr=KS.kktsolver_qr, sparse=KS.kktsolver_sparse)[solver] if solver != "2x2" else KS.pivot(KS.kktsolver_2x2)
    with np.errstate(all="ignore"):
        return oracle_conicIP(*case_problem(name), kktsolver=sv, **dict(opts))


def oracle_run(name, solver="qr", **more):
    """the oracle on a case; computed once and shared -- callers do not modify it"""
    return _oracle(name, solver, tuple(sorted(dict(case_options(name), **more).items())))


def deviation(got, ref):
    """{quantity: relative difference} over everything the GPU tests compare with the oracle.  A block of the returned iterate is
    either NaN in full on both sides or finite on both, and is then measured against its own norm; the three feasibilities
    against the largest of them (what the loop tests is their maximum: one of them at rounding level carries no digits); Mu
    against itself; pobj and dobj against the larger of the two (on a diverging iterate pobj is the small difference of two
    large terms)."""
    out = {}
    for f in ("y", "w", "v"):
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(ref, f))
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if b.size == 0:
            continue
        if np.isnan(b).any():
            assert np.isnan(b).all(), f
            out[f] = 0.0 if np.isnan(a).all() else math.inf
        else:
            assert np.isfinite(b).all(), f
            out[f] = float(np.linalg.norm(a - b) / np.linalg.norm(b)) if np.isfinite(a).all() else math.inf
    feas = max(ref.prFeas, ref.duFeas, ref.muFeas)
    for f in ("prFeas", "duFeas", "muFeas"):
        out[f] = abs(getattr(got, f) - getattr(ref, f)) / feas
    out["Mu"] = abs(got.Mu - ref.Mu) / abs(ref.Mu)
    obj = max(abs(ref.pobj), abs(ref.dobj))
    for f in ("pobj", "dobj"):
        out[f] = abs(getattr(got, f) - getattr(ref, f)) / obj
    return {k: (math.inf if v != v else v) for k, v in out.items()}


def by_group(dev):
    return {g: max((dev[q] for q in qs if q in dev), default=0.0) for g, qs in GROUPS.items()}


def spread(name):
    """{group: the host's own spread on a case}: the oracle's two solvers, equal in exact arithmetic"""
    a, b = oracle_run(name), oracle_run(name, case(name).get("second", "2x2"))
    assert counts(a) == counts(b), (name, counts(a), counts(b))
    return by_group(deviation(b, a))


def unchecked(name):
    """the scalars of a case that are below tolerance x the scale they are measured against: they carry no check"""
    ref, tol = oracle_run(name), tolerance(name)
    feas, obj = max(ref.prFeas, ref.duFeas, ref.muFeas), max(abs(ref.pobj), abs(ref.dobj))
    out = [f for f in ("prFeas", "duFeas", "muFeas") if abs(getattr(ref, f)) <= tol["state"] * feas]
    return tuple(out + [f for f in ("pobj", "dobj") if abs(getattr(ref, f)) <= tol["objective"] * obj])


def counts(sol):
    return (sol.status, sol.Iter, len(sol.trace), sol.n_factor, sol.n_solve)


def assert_matches_oracle(got, name, what="", trace=True):
    """a. of tests/test_gpu_stopping.py (trace = False: the batch paths keep no trace rows)"""
    ref, tol = oracle_run(name), tolerance(name)
    pick = lambda t: tuple(t[i] for i in (range(5) if trace else (0, 1, 3, 4)))
    assert pick(counts(got)) == pick(counts(ref)), (name, what, counts(got), counts(ref))
    dev = deviation(got, ref)
    print("DEVIATION %s %s: %s (tolerances %s)" % (name, what, {k: "%.2e" % v for k, v in dev.items()}, {g: "%.2g" % t for g, t in tol.items()}))
    for g, v in by_group(dev).items():
        assert v <= tol[g], (name, what, g, dev, tol[g])


# ---------------------------------------------------------------------------------------------------------------- certificates
def _blocks(cone_dims):
    at = 0
    for t, k in cone_dims:
        yield t, slice(at, at + k)
        at += k


def strictly_inside(v, cone_dims):
    """R entries > 0, v0 > |v1|, mat(v) with smallest eigenvalue > 0"""
    for t, I in _blocks(cone_dims):
        x = v[I]
        if t == "R":
            ok = bool(np.all(x > 0))
        elif t == "Q":
            ok = bool(x[0] > np.linalg.norm(x[1:]))
        else:
            ok = bool(np.linalg.eigvalsh(OC.mat(x)).min() > 0)
        if not ok:
            return False
    return True


def cone_distance(x, cone_dims):
    """the distance of x from the cone: the negative part for R, the projection for Q, the negative eigenvalues for S"""
    d2 = 0.0
    for t, I in _blocks(cone_dims):
        z = x[I]
        if t == "R":
            d2 += float(np.sum(np.minimum(z, 0.0) ** 2))
        elif t == "Q":
            t0, r = z[0], float(np.linalg.norm(z[1:]))
            if r <= t0:
                pass
            elif r <= -t0:
                d2 += float(z @ z)
            else:
                d2 += (r - t0) ** 2 / 2.0
        else:
            lam = np.linalg.eigvalsh(OC.mat(z))
            d2 += float(np.sum(np.minimum(lam, 0.0) ** 2))
    return math.sqrt(d2)


def assert_certificate(sol, name, what=""):
    """b. of tests/test_gpu_stopping.py: what a certificate must satisfy, whoever computed it.  The bounds are the stopping test's
    own (src/ConicIP.jl:812, :843) after the scaling of :816 / :848; gamma = k 2^-53 is the running error of a dot of length k."""
    Q, c, A, b, K, G, d = case_problem(name)
    n, m = len(c), len(b)
    p = 0 if G is None else G.shape[0]
    G = np.zeros((0, n)) if G is None else np.asarray(G)
    d = np.zeros(0) if d is None else d
    A = A.toarray() if sp.issparse(A) else np.asarray(A)
    Q = Q.toarray() if sp.issparse(Q) else np.asarray(Q)
    opts = case_options(name)
    tol = opts.get("infeasTol", opts["optTol"])
    slack = 1 + 1e-12
    nrm1 = lambda x: max(1.0, float(np.linalg.norm(x))) if len(x) else 1.0
    if sol.status == "Infeasible":
        assert np.isnan(sol.y).all() and len(sol.y) == n, (name, what)
        assert np.isfinite(sol.v).all() and np.isfinite(sol.w).all(), (name, what)
        assert strictly_inside(sol.v, K), (name, what, sol.v)
        gamma = (m + p) * 2.0 ** -53
        lhs = abs(float(d @ sol.w) - float(b @ sol.v) + 1.0)
        assert lhs <= 4 * gamma * (float(np.abs(d) @ np.abs(sol.w)) + float(np.abs(b) @ np.abs(sol.v))), (name, what, lhs)
        res = float(np.linalg.norm(G.T @ sol.w - A.T @ sol.v))
        assert res < tol * nrm1(c) * slack, (name, what, res)
    elif sol.status == "Unbounded":
        assert np.isnan(sol.v).all() and np.isnan(sol.w).all() and len(sol.v) == m and len(sol.w) == p, (name, what)
        assert np.isfinite(sol.y).all(), (name, what)
        lhs = abs(float(c @ sol.y) - 1.0)
        assert lhs <= 4 * n * 2.0 ** -53 * float(np.abs(c) @ np.abs(sol.y)), (name, what, lhs)
        assert float(np.linalg.norm(Q @ sol.y)) < tol * nrm1(c) * slack, (name, what)
        if p > 0:
            assert float(np.linalg.norm(G @ sol.y)) < tol * nrm1(d) * slack, (name, what)
        assert cone_distance(A @ sol.y, K) < tol * nrm1(b) * slack, (name, what)
    else:
        raise AssertionError("no certificate: %s %s %s" % (name, what, sol.status))
