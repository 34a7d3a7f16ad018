"""The refinement case table (tests/_refine_cases.py) checked on the oracle alone -- no GPU.

What is asserted here is a condition on the INPUTS of tests/test_gpu_refinement.py: every (case, threshold, depth) the GPU tests
run keeps every refinement residual of the oracle a factor of 100 away from the threshold, the table holds runs without any
refinement, runs that refine to the full depth 1, 2 and 3 in every step, and runs with an intermediate depth, every run whose
counts are compared is steady (tests/_refine_cases.py: member_steady), and every lock-step group has, in every iteration in which it steps, a refining set that is a non-empty strict subset of the stepping set.
Also here: the options helper of the native batch paths (cipkkt/batch.py: _native_options)."""
import math

import pytest

import _refine_cases as RC


# ---------------------------------------------------------------------------------------------------------------- the hook
def test_oracle_records_every_refinement_residual():
    """trace[-1]["rnorm"]: one list per stepping row, as long as the depth allows and the threshold asks for; none on the
    terminating row; the run itself is unchanged by the hook (status, counts)"""
    name = "small_q_1e12_partial"
    T = RC.CASES[name]["T"]
    for k in RC.DEPTHS:
        forced, never, part = (RC.oracle_run(name, t, k) for t in (RC.FORCED, RC.NEVER, T))
        for sol in (forced, never, part):
            assert sol.status == "Optimal" and len(sol.trace) == sol.n_factor - 1
            assert "rnorm" not in sol.trace[-1]
            assert all(isinstance(r, float) for row in sol.trace[:-1] for r in row["rnorm"])
        assert [len(row["rnorm"]) for row in forced.trace[:-1]] == [k] * (len(forced.trace) - 1)
        assert [len(row["rnorm"]) for row in never.trace[:-1]] == [min(k, 1)] * (len(never.trace) - 1)
        for sol, t in ((forced, RC.FORCED), (never, RC.NEVER), (part, T)):
            assert sol.n_solve == 1 + sum(2 + c for c in RC.solves_per_iteration(sol, t)[:-1])
            # a residual below the threshold ends the row's list; every residual before it was followed by a solve
            for row in sol.trace[:-1]:
                assert all(not r < t for r in row["rnorm"][:-1])


# ---------------------------------------------------------------------------------------------------------------- the margin rule
@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_respects_the_margin_rule(name):
    cs = RC.CASES[name]
    for T in RC.thresholds(name):
        for k in RC.DEPTHS:
            sol = RC.oracle_run(name, T, k)
            assert sol.status == "Optimal", (name, T, k, sol.status)
            mg = RC.member_margin(RC.case_member(name), T, k)
            print("%s T=%g k=%d: Iter %d n_solve %d solves/iteration %s margin %.3g" % (
                name, T, k, sol.Iter, sol.n_solve, RC.solves_per_iteration(sol, T), mg))
            assert mg >= RC.MARGIN, (name, T, k, mg)
            if not RC.steady(name, T, k):                 # only runs that leave a large residual unrefined may be unsteady
                print("    not steady: no counts are compared with this run")
                assert k == 0 or T == RC.NEVER, (name, T, k)
                assert cs["scale"] >= 1e9
            per = RC.solves_per_iteration(sol, T)
            assert per[-1] == 0 and sol.n_solve == 1 + sum(2 + c for c in per[:-1])
            if T == RC.FORCED:
                assert per[:-1] == [k] * (len(per) - 1)
                assert sol.n_solve == RC.closed_form(len(sol.trace), k)
            if T == RC.NEVER or k == 0:
                assert per == [0] * len(per)
                assert sol.n_solve == RC.closed_form(len(sol.trace), 0)
    if cs["T"] is not None:
        per = RC.solves_per_iteration(RC.oracle_run(name, cs["T"], 3), cs["T"])[:-1]
        kind = "none" if not any(per) else ("full" if all(c == 3 for c in per) else "partial")
        assert kind == cs["depths"], (name, per)
        if kind == "partial":
            assert any(0 < c < 3 for c in per), per


def test_table_holds_every_depth():
    """(a) no refinement anywhere, (b) depth k everywhere for k = 1, 2, 3 -- by threshold, not only forced -- and (c) an
    intermediate depth in some iteration"""
    seen = set()
    for name, cs in RC.CASES.items():
        if cs["T"] is None:
            continue
        for k in (1, 2, 3):
            per = RC.solves_per_iteration(RC.oracle_run(name, cs["T"], k), cs["T"])[:-1]
            if not any(per):
                seen.add("none")
            elif all(c == k for c in per):
                seen.add(("full", k))
            if any(0 < c < k for c in per):
                seen.add("partial")
    assert seen >= {"none", ("full", 1), ("full", 2), ("full", 3), "partial"}, seen


def test_table_covers_the_shapes():
    fams = {name: RC.case_problem(name) for name in RC.CASES}
    import scipy.sparse as sp
    kinds = set()
    for name, (Q, c, A, b, K, G, d) in fams.items():
        types = {t for t, _ in K}
        p = 0 if G is None else G.shape[0]
        kinds.add(("".join(sorted(types)), "csr" if sp.issparse(A) else "dense", p > 0, RC.CASES[name]["route"]))
        assert 21 <= Q.shape[0] <= 300
    assert ("R", "dense", True, "schur") in kinds and any(k[:2] == ("R", "csr") for k in kinds)
    assert ("QR", "dense", True, "schur") in kinds and ("QR", "dense", True, "full3x3") in kinds
    assert ("QR", "dense", False, "schur") in kinds              # p == 0
    assert any(k[0] == "S" for k in kinds)
    # the fused kernels' four workgroups, no section boundary on a multiple of 64 (tests/test_gpu_vecops.py: LOOP)
    Q, c, A, b, K, G, d = fams["q_cones_1e9_schur"]
    n, m, p = Q.shape[0], A.shape[0], G.shape[0]
    assert 768 < n + p + 2 * m <= 1024 and all(s % 64 for s in (n, n + p, n + p + m))


# ---------------------------------------------------------------------------------------------------------------- the groups
@pytest.mark.parametrize("name", list(RC.GROUPS))
def test_group_has_a_refining_strict_subset_in_every_stepping_iteration(name):
    g = RC.GROUPS[name]
    T, k = g["T"], g["k"]
    assert 6 <= len(g["members"]) <= 8
    shapes = {(Q.shape[0], A.shape[0], 0 if G is None else G.shape[0], tuple(K)) for Q, c, A, b, K, G, d in RC.group_problems(name)}
    assert len(shapes) == 1
    sols = [RC.oracle_member(mb, T, k) for mb in g["members"]]
    for mb, sol in zip(g["members"], sols):
        assert sol.status == ("Infeasible" if mb["family"] == "infeasible_box" else "Optimal"), (mb, sol.status)
        mg = RC.member_margin(mb, T, k)
        print("%s %s scale %g: %s rows %d n_solve %d solves/iteration %s margin %.3g" % (
            name, mb["family"], mb["scale"], sol.status, len(sol.trace), sol.n_solve, RC.solves_per_iteration(sol, T), mg))
        assert mg >= RC.MARGIN, (mb, mg)
        assert RC.member_steady(mb, T, k), mb
    rows = [len(s.trace) for s in sols]
    assert min(rows) < max(rows)                                  # some member stops before the rest
    assert len({s.n_solve for s in sols}) > 1
    if k == 0:
        return
    per = [RC.solves_per_iteration(s, T) for s in sols]
    for it in range(max(rows) - 1):                               # the group's last iteration only terminates
        stepping = [i for i, r in enumerate(rows) if it < r - 1]
        refining = [i for i in stepping if per[i][it] > 0]
        assert 0 < len(refining) < len(stepping), (it, stepping, refining)
        assert all(per[i][it] == k for i in refining)


# ---------------------------------------------------------------------------------------------------------------- options
def test_native_options_helper():
    """absent or None -> -1.0 (the library's default: optTol, optTol / 1e7); every given number goes through, 0.0 too"""
    from cipkkt.batch import _native_options
    o = _native_options({})
    assert (o.optTol, o.DTB, o.infeasTol, o.refinementThreshold, o.maxRefinementSteps, o.maxIters, o.verbose) == (1e-6, 0.01, -1.0, -1.0, 3, 100, 0)
    o = _native_options(dict(infeasTol=None, refinementThreshold=None))
    assert (o.infeasTol, o.refinementThreshold) == (-1.0, -1.0)
    o = _native_options(dict(infeasTol=0.0, refinementThreshold=0.0, maxRefinementSteps=2))
    assert (o.infeasTol, o.refinementThreshold, o.maxRefinementSteps) == (0.0, 0.0, 2)
    assert math.copysign(1.0, o.refinementThreshold) == 1.0 and math.copysign(1.0, o.infeasTol) == 1.0
    o = _native_options(dict(infeasTol=1e-3, refinementThreshold=1e-12, optTol=1e-7, DTB=0.05, maxIters=7, maxRefinementSteps=0))
    assert (o.optTol, o.DTB, o.infeasTol, o.refinementThreshold, o.maxRefinementSteps, o.maxIters) == (1e-7, 0.05, 1e-3, 1e-12, 0, 7)
    o = _native_options(dict(refinementThreshold=1e300, kktsolver="full3x3"))
    assert o.refinementThreshold == 1e300
