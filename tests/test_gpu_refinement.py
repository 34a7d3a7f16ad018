"""The Newton step's iterative refinement inside the interior-point loop (csrc/driver.hip: "Newton step + refinement" down to
"step"; cipkkt/driver.py is its per-operation twin), driven on purpose at every depth.

The cases, their thresholds T and the margin that makes the solve counts reproducible are in tests/_refine_cases.py;
tests/test_refine_cases.py checks them on the oracle without a GPU.  Here:
  a. the native loop against the oracle over maxRefinementSteps x refinementThreshold: status, Iter, n_factor, n_solve, trace rows,
     the closed form of forced runs, and the refinement solves of every single iteration (by differencing n_solve over maxIters)
  b. the native loop against the Python driver -- no speculation, no masks, no fused kernel -- bit for bit
  c. that the refinement takes effect numerically: mu per iteration against the oracle at a scaling where depth 0 and depth 3 part
  d. lock-step groups in which a strict subset refines, bit for bit against the one-problem runs and in counts against the oracle
  e. regularised members that stay in their group under forced refinement
  f. refinementThreshold = 0.0 and infeasTol = 0.0 through every batch path"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _refine_cases as RC
import problems as P

pytestmark = pytest.mark.gpu

FIELDS = ("Mu", "prFeas", "duFeas", "muFeas", "pobj", "dobj")
SWEEP = [(name, T) for name in RC.CASES for T in RC.thresholds(name)]
_ids = lambda v: v if isinstance(v, str) else {RC.FORCED: "forced", RC.NEVER: "never"}.get(v, "T%g" % v)


def _device(name, T, k, driver="native", **kw):
    import cipkkt
    Q, c, A, b, K, G, d = RC.case_problem(name)
    return cipkkt.conicIP(Q, c, A, b, K, G, d, kktsolver=RC.CASES[name]["route"], optTol=RC.OPT, refinementThreshold=T,
                          maxRefinementSteps=k, driver=driver, **kw)


def _same_counts(got, ref, what):
    assert got.status == ref.status, (what, got.status, ref.status)
    assert (got.Iter, got.n_factor, got.n_solve, len(got.trace)) == (ref.Iter, ref.n_factor, ref.n_solve, len(ref.trace)), (
        what, (got.Iter, got.n_factor, got.n_solve, len(got.trace)), (ref.Iter, ref.n_factor, ref.n_solve, len(ref.trace)))


# ---------------------------------------------------------------------------------------------------------------- a. depth sweep
@pytest.mark.parametrize("name,T", SWEEP, ids=_ids)
def test_depth_sweep_against_the_oracle(name, T):
    for k in RC.DEPTHS:
        got, ref = _device(name, T, k), RC.oracle_run(name, T, k)
        if RC.steady(name, T, k):
            _same_counts(got, ref, (name, T, k))
        else:                                  # (tests/_refine_cases.py: member_steady) the run's own counts only
            assert got.status == "Optimal" and (k == 0 or T == RC.NEVER)
        if T == RC.FORCED:
            assert got.n_solve == RC.closed_form(len(got.trace), k), (name, k, got.n_solve, len(got.trace))
        if T == RC.NEVER:
            assert got.n_solve == RC.closed_form(len(got.trace), 0), (name, k, got.n_solve, len(got.trace))


PREFIX = [("q_cones_1e9_schur", RC.FORCED, 2), ("all_r_csr_1e6", RC.FORCED, 3), ("q_cones_1e9_full3x3", 1e-12, 3),
          ("small_q_1e12_partial", 1e14, 3), ("small_q_p0_1e9", 1e-12, 2), ("psd_1e6", RC.FORCED, 3),
          ("all_r_dense_1e-4", RC.NEVER, 3), ("q_cones_1e-4", 1e-12, 1)]


@pytest.mark.parametrize("name,T,k", PREFIX, ids=_ids)
def test_refinement_solves_of_every_iteration(name, T, k):
    """n_solve of the runs with maxIters = 1 .. J - 1 (each abandoned behind its last step; the prefixes of one deterministic
    run), differenced: predictor + Newton step + that iteration's refinement solves -- against the oracle's residual lists"""
    assert T in RC.thresholds(name) and RC.steady(name, T, k)
    ref = RC.oracle_run(name, T, k)
    want = RC.solves_per_iteration(ref, T)
    J = len(ref.trace)
    prev, got = 1, []                                  # the initial point's solve
    for j in range(1, J):
        sol = _device(name, T, k, maxIters=j)
        assert sol.status == "Abandoned" and len(sol.trace) == j, (j, sol.status)
        got.append(sol.n_solve - prev - 2)
        prev = sol.n_solve
    full = _device(name, T, k)
    assert len(full.trace) == J and full.n_solve == prev          # the terminating row factors, and solves nothing
    assert got == want[:-1], (got, want)
    if T == RC.CASES[name]["T"] and RC.CASES[name]["depths"] == "partial" and k == 3:
        assert any(0 < c < k for c in got)


# ---------------------------------------------------------------------------------------------------------------- b. the two drivers
def _ratio_line(name, T, k, py, ref):
    """the device's refinement residuals over the oracle's, pair by pair (recorded in DESIGN_LOG.md)"""
    ratios = [g / o for gl, row in zip(py.refine_rnorms, ref.trace) for g, o in zip(gl, row.get("rnorm", ())) if o > 0.0]
    if ratios:
        print("RNORM_RATIO %s T=%g k=%d: device/oracle min %.3g median %.3g max %.3g over %d residuals" % (
            name, T, k, min(ratios), float(np.median(ratios)), max(ratios), len(ratios)))


@pytest.mark.parametrize("name,T", SWEEP, ids=_ids)
def test_native_loop_equals_the_python_driver_bit_for_bit(name, T):
    for k in RC.DEPTHS:
        nat, py = _device(name, T, k), _device(name, T, k, driver="python")
        _same_counts(nat, py, (name, T, k))
        for tn, tp in zip(nat.trace, py.trace):
            assert set(tn) == set(tp)
            for key in tn:
                assert tn[key] == tp[key], (name, T, k, key, tn["Iter"], tn[key], tp[key])
        for f in ("y", "w", "v"):
            assert np.array_equal(getattr(nat, f), getattr(py, f)), (name, T, k, f)
        for f in FIELDS:
            assert getattr(nat, f) == getattr(py, f), (name, T, k, f)
        # the Python driver's own residual lists: as many as the oracle's, and far from T on the device too
        assert len(py.refine_rnorms) == len(py.trace) - 1
        assert "rnorm" not in py.trace[0] and nat.refine_rnorms == []
        if RC.steady(name, T, k):
            ref = RC.oracle_run(name, T, k)
            assert [len(x) for x in py.refine_rnorms] == [len(row["rnorm"]) for row in ref.trace[:-1]], (name, T, k)
            _ratio_line(name, T, k, py, ref)
        if T != RC.FORCED:
            mg = RC.margin([r for rl in py.refine_rnorms for r in rl], T)
            print("DEVICE_MARGIN %s T=%g k=%d: %.3g" % (name, T, k, mg))
            assert mg >= 10.0, (name, T, k, mg)


# ---------------------------------------------------------------------------------------------------------------- c. the effect
# seed 100 of the n = 40 Q-cone shape at data scale 1e12, forced refinement: the oracle's depth-0 run needs 11 iterations and its
# depth-3 run 9, and their mu part by factors of 3 to 700 from the second iteration on.  MU_TOL is 10 x the largest relative
# deviation of the device's mu from the oracle's depth-3 mu measured on the MI355X (DESIGN_LOG.md), one decade for the run-to-run
# variation of a rounding-driven quantity; it has to stay below a tenth of the oracle's own depth-0 / depth-3 gap.
EFFECT = dict(family="mixed", kw=dict(n=40, nq=3, kq=6, p=4, seed=100), scale=1e12)
MU_TOL = 2.1e-2


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_refinement_takes_effect_on_mu(route):
    import cipkkt
    Q, c, A, b, K, G, d = RC.build(EFFECT["family"], EFFECT["kw"], EFFECT["scale"])
    ref0, ref3 = RC.oracle_member(EFFECT, RC.FORCED, 0), RC.oracle_member(EFFECT, RC.FORCED, 3)
    gap = [abs(a["mu"] - b_["mu"]) / b_["mu"] for a, b_ in zip(ref0.trace, ref3.trace)]
    ks = cipkkt.KKTSystem(Q, A, G, K, route=route)
    try:
        got = cipkkt.conicIP(Q, c, A, b, K, G, d, optTol=RC.OPT, refinementThreshold=RC.FORCED, maxRefinementSteps=3, system=ks)
        health = ks.health()
    finally:
        ks.close()
    assert health["n_regularized"] == 0, health
    _same_counts(got, ref3, route)
    dev = [abs(a["mu"] - b_["mu"]) / b_["mu"] for a, b_ in zip(got.trace, ref3.trace)]
    print("MU_DEVIATION %s: device vs oracle depth 3 %s" % (route, ["%.2e" % x for x in dev]))
    print("MU_GAP oracle depth 0 vs depth 3 %s" % ["%.2e" % x for x in gap])
    assert any(MU_TOL <= g / 10.0 for g in gap), (MU_TOL, gap)             # the tolerance separates refined from unrefined
    assert max(dev) <= MU_TOL, (dev, MU_TOL)


# ---------------------------------------------------------------------------------------------------------------- d. lock-step groups
def _solve(prs, mode, in_flight=4, keep=False):
    """tests/test_gpu_lockstep.py: the one-problem reference runs under the solve block the lock-step call uses"""
    from cipkkt import _lib as L
    from cipkkt.batch import _solve_problems_native
    lib = L.load()
    prev = lib.cip_set_solve_block_max(lib.cip_lockstep_solve_block_for(len(prs))) if mode == "threads" else None
    try:
        return _solve_problems_native(prs, torch.device("cuda:0"), in_flight, mode, keep_regularized=keep)
    finally:
        if prev is not None:
            lib.cip_set_solve_block_max(prev)


def _assert_identical(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.status == y.status, (i, x.status, y.status)
        assert (x.Iter, x.n_factor, x.n_solve) == (y.Iter, y.n_factor, y.n_solve), (i, (x.Iter, x.n_factor, x.n_solve), (y.Iter, y.n_factor, y.n_solve))
        for f in ("y", "w", "v"):
            assert np.array_equal(getattr(x, f), getattr(y, f), equal_nan=True), (i, f)
        for f in FIELDS:
            assert getattr(x, f) == getattr(y, f) or (getattr(x, f) != getattr(x, f) and getattr(y, f) != getattr(y, f)), (i, f)


def _group(name, **more):
    g = RC.GROUPS[name]
    kw = dict(optTol=RC.OPT, refinementThreshold=g["T"], maxRefinementSteps=g["k"], **more)
    if g["route"] != "schur":
        kw["kktsolver"] = g["route"]
    return [dict(Q=Q, c=c, A=A, b=b, cone_dims=K, G=G, d=d, kwargs=dict(kw)) for Q, c, A, b, K, G, d in RC.group_problems(name)]


@pytest.mark.parametrize("name", list(RC.GROUPS))
def test_group_with_a_refining_subset(name):
    g = RC.GROUPS[name]
    prs = _group(name)
    one = _solve(prs, "threads", in_flight=1)
    lock = _solve(prs, "lockstep")
    _assert_identical(lock, one)
    for i, (got, mb) in enumerate(zip(lock, g["members"])):
        ref = RC.oracle_member(mb, g["T"], g["k"])
        assert got.status == ref.status, (i, got.status, ref.status)
        assert (got.Iter, got.n_factor, got.n_solve) == (ref.Iter, ref.n_factor, ref.n_solve), (
            i, (got.Iter, got.n_factor, got.n_solve), (ref.Iter, ref.n_factor, ref.n_solve))
    assert len({s.n_solve for s in lock}) > 1 and len({s.n_factor for s in lock}) > 1
    if g["T"] != RC.FORCED:
        # the device's own residuals keep a factor of 10 from T on the group's route (the Python driver records them)
        import cipkkt
        for i, pr in enumerate(prs):
            py = cipkkt.conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], pr["G"], pr["d"], driver="python",
                                **dict(pr["kwargs"], kktsolver=g["route"]))
            mg = RC.margin([r for rl in py.refine_rnorms for r in rl], g["T"])
            print("DEVICE_MARGIN group %s member %d: %.3g" % (name, i, mg))
            assert mg >= 10.0, (name, i, mg)
            assert (py.status, py.n_factor, py.n_solve) == (lock[i].status, lock[i].n_factor, lock[i].n_solve), i
    if name == "all_r_csr_k3":
        assert [s.status for s in lock].count("Infeasible") == 1 and sp.issparse(prs[0]["A"])


def test_group_refinement_solves_per_problem_and_iteration():
    """the maxIters differencing on a group: every member's refinement solves in every iteration, in lock-step, against the
    oracle's -- the members that refine take 3, the others none, and a member that has stopped takes nothing more"""
    name = "all_r_csr_k3"
    g = RC.GROUPS[name]
    assert all(RC.member_steady(mb, g["T"], g["k"]) for mb in g["members"])
    refs = [RC.oracle_member(mb, g["T"], g["k"]) for mb in g["members"]]
    want = [RC.solves_per_iteration(r, g["T"]) for r in refs]
    rows = [len(r.trace) for r in refs]
    prev = [1] * len(refs)
    for j in range(1, max(rows)):
        sols = _solve(_group(name, maxIters=j), "lockstep")
        for i, s in enumerate(sols):
            stepped = j < rows[i]                      # iteration j of member i is not its terminating one
            assert s.n_solve - prev[i] == ((2 + want[i][j - 1]) if stepped else 0), (j, i, s.n_solve, prev[i], want[i])
            assert s.n_factor == 1 + min(j, rows[i])
            prev[i] = s.n_solve
    assert prev == [r.n_solve for r in refs]
    assert {c for w in want for c in w} == {0, 3}


# ---------------------------------------------------------------------------------------------------------------- e. regularised members
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("variant", ["schur", "schur-qcone"])
def test_regularised_members_under_forced_refinement(variant, k):
    """the LP / QP mix of tests/test_gpu_lockstep_regularized.py with keep_regularized: the loop's refine mask (narrowed as members
    stop) and the regularised problems' mask of cip_solve4x4_dev are both narrower than the active set at once"""
    import test_gpu_lockstep_regularized as REG
    rng = np.random.default_rng(15)
    q = "qcone" in variant
    prs = [REG._lp(16, rng, q_cone=q) if i % 2 else REG._definite_qp(16, rng, q_cone=q) for i in range(6)]
    assert [REG._needs_regularisation(pr) for pr in prs] == [False, True] * 3
    for pr in prs:
        pr["kwargs"] = dict(pr["kwargs"], refinementThreshold=RC.FORCED, maxRefinementSteps=k)
    one = _solve(prs, "threads", in_flight=1)
    assert [s.status for s in one] == ["Optimal"] * 6, [s.status for s in one]
    on = _solve(prs, "lockstep", keep=True)
    st, nreg = REG._stats()
    assert st == (1, 6, 0) and nreg == 3, (st, nreg)
    _assert_identical(on, one)
    assert len({s.n_factor for s in on}) > 1                       # members stop at different iterations: the refine mask narrows
    for s in on:
        assert s.n_solve == RC.closed_form(s.n_factor - 1, k), (s.n_solve, s.n_factor, k)
    assert REG._switch_is_off()


# ---------------------------------------------------------------------------------------------------------------- f. options
def _batch_paths(prs):
    from cipkkt.batch import _solve_many_native, _solve_problems_native
    dev = torch.device("cuda:0")
    yield "many", _solve_many_native(prs, dev, 1)
    for mode in ("lockstep", "threads", "auto"):
        yield mode, _solve_problems_native(prs, dev, 1, mode)


def _pairs(seeds, scale, **kw):
    prs = []
    for seed in seeds:
        Q, c, A, b, K, G, d = RC.build("mixed", dict(n=40, nq=3, kq=6, p=4, seed=seed), scale)
        prs.append(dict(Q=Q, c=c, A=A, b=b, cone_dims=K, G=G, d=d, kwargs=dict(kw)))
    return prs


def test_forced_refinement_reaches_every_batch_path():
    """refinementThreshold = 0.0 means "always refine"; at data scale 1e-4 the default threshold would never refine"""
    import cipkkt
    kw = dict(optTol=RC.OPT, refinementThreshold=0.0, maxRefinementSteps=2)
    prs = _pairs((100, 101), 1e-4, **kw)
    want = [cipkkt.conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], pr["G"], pr["d"], **kw) for pr in prs]
    default = [cipkkt.conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], pr["G"], pr["d"], optTol=RC.OPT, maxRefinementSteps=2)
               for pr in prs]
    for s, dflt in zip(want, default):
        assert s.status == "Optimal" and s.n_solve == RC.closed_form(len(s.trace), 2)
        assert dflt.n_solve == RC.closed_form(len(dflt.trace), 0)            # what a dropped 0.0 would give
    for path, got in _batch_paths(prs):
        for s in got:
            assert s.n_solve == RC.closed_form(s.n_factor - 1, 2), (path, s.n_solve, s.n_factor)
        _assert_identical(got, want)


def test_infeas_tol_zero_reaches_every_batch_path():
    """infeasTol = 0.0 means "never certify": the infeasible box is not ended as Infeasible (maxIters = 8: it is abandoned)"""
    import cipkkt
    kw = dict(optTol=RC.OPT, infeasTol=0.0, maxIters=8)
    prs = []
    for seed in (0, 1):
        Q, c, A, b, K, G, d = P.infeasible_box(10, seed)[:7]
        prs.append(dict(Q=Q, c=c, A=A, b=b, cone_dims=K, G=G, d=d, kwargs=dict(kw)))
    want = [cipkkt.conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], **kw) for pr in prs]
    certified = cipkkt.conicIP(prs[0]["Q"], prs[0]["c"], prs[0]["A"], prs[0]["b"], prs[0]["cone_dims"], optTol=RC.OPT, maxIters=8)
    assert certified.status == "Infeasible"                                  # what a dropped 0.0 would give
    assert [s.status for s in want] == ["Abandoned"] * 2, [s.status for s in want]
    for path, got in _batch_paths(prs):
        assert all(s.status != "Infeasible" for s in got), (path, [s.status for s in got])
        _assert_identical(got, want)
