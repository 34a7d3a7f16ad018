"""The stopping case table (tests/_stop_cases.py) checked on the oracle alone -- no GPU.

What is asserted here is a condition on the INPUTS of tests/test_gpu_stopping.py: every case ends in the state, at the iteration
and with the best-iterate index the table names; the certificates the oracle returns satisfy what a certificate must satisfy
(the same function the GPU tests apply to the device's); the oracle's own spread between its two solvers is still below the
recorded one the tolerances are built from; and the lock-step group holds every end state and stops at different iterations."""
import numpy as np
import pytest

import _stop_cases as SC

ALL = list(SC.CASES) + list(SC.GROUP_EXTRA)


@pytest.mark.parametrize("name", ALL)
def test_case_ends_as_the_table_says(name):
    cs = SC.case(name)
    sol = SC.oracle_run(name)
    Q, c, A, b, K, G, d = SC.case_problem(name)
    assert len(c) <= 12
    print("%s: %s rows %d Iter %d n_factor %d n_solve %d" % (name, sol.status, len(sol.trace), sol.Iter, sol.n_factor, sol.n_solve))
    assert (sol.status, len(sol.trace), sol.Iter) == (cs["status"], cs["rows"], cs["Iter"]), (name, SC.counts(sol))
    assert sol.n_factor == len(sol.trace) + 1
    # every stepping row refines to the full depth; the terminating row of a run that stopped solves nothing
    stepping = len(sol.trace) if sol.status == "Abandoned" else len(sol.trace) - 1
    assert sol.n_solve == 1 + 5 * stepping
    if sol.status in ("Infeasible", "Unbounded"):
        SC.assert_certificate(sol, name, "oracle")
        nan, fin = (("y",), ("w", "v")) if sol.status == "Infeasible" else (("w", "v"), ("y",))
        assert all(np.isnan(getattr(sol, f)).all() for f in nan) and all(np.isfinite(getattr(sol, f)).all() for f in fin)
    else:
        assert all(np.isfinite(getattr(sol, f)).all() for f in ("y", "w", "v"))
    if sol.status == "Abandoned":
        assert len(sol.trace) == SC.case_options(name)["maxIters"] and "alpha" in sol.trace[-1]      # the last row stepped


@pytest.mark.parametrize("name", ALL)
def test_spread_of_the_oracle_is_below_the_recorded_one(name):
    """the host's own two-solver spread against MARGIN x the figure measured over five BLAS kernel sets (tests/_stop_spread.py)"""
    cs, host, allowed, tol = SC.case(name), SC.spread(name), SC.allowed_spread(name), SC.tolerance(name)
    print("%s: host spread %s, measured %r, tolerances %s, unchecked %r" % (
        name, {g: "%.2g" % v for g, v in host.items()}, cs["measured"], {g: "%.2g" % v for g, v in tol.items()}, cs["unchecked"]))
    assert len(cs["measured"]) == len(SC.GROUPS) == 3
    for g in SC.GROUPS:
        assert host[g] <= max(allowed[g], SC.FLOOR), (name, g, host[g], allowed[g])        # (below the floor the figure does not enter the tolerance)
        assert tol[g] == 10 * max(4 * cs["measured"][list(SC.GROUPS).index(g)], 1e-12)
    assert tol["iterate"] <= 1e-10 or name == "narrow_infeasible_box"
    assert tol["state"] <= 1e-10 or name in SC.GROUP_EXTRA
    assert max(tol.values()) <= 1e-4 or name == "narrow_infeasible_box"
    assert SC.unchecked(name) == cs["unchecked"], (name, SC.unchecked(name))
    # Mu, dobj and the largest feasibility are checked in every case; pobj wherever the iterate does not diverge
    assert "dobj" not in cs["unchecked"] and len([f for f in cs["unchecked"] if f.endswith("Feas")]) <= 2
    if cs["status"] != "Infeasible" and name != "narrow_infeasible_box":
        assert "pobj" not in cs["unchecked"]


def test_table_holds_every_branch():
    states = {cs["status"] for cs in SC.CASES.values()}
    assert states == {"Infeasible", "Unbounded", "Abandoned"}
    kinds = set()
    for name, cs in SC.CASES.items():
        Q, c, A, b, K, G, d = SC.case_problem(name)
        kinds.add((cs["status"], "".join(sorted({t for t, _ in K})), G is not None, bool(np.any(Q))))
    for want in (("Infeasible", "R", False, True), ("Infeasible", "R", True, True), ("Infeasible", "Q", True, True),
                 ("Infeasible", "S", True, True), ("Infeasible", "QR", False, True), ("Unbounded", "R", False, False),
                 ("Unbounded", "R", False, True), ("Unbounded", "R", True, False), ("Unbounded", "Q", False, False),
                 ("Abandoned", "R", True, True)):
        assert want in kinds, want
    # the best iterate of an infeasible problem is an early one: Iter is not the stopping iteration
    assert all(cs["Iter"] < cs["rows"] for cs in SC.CASES.values() if cs["status"] == "Infeasible")
    # Q = 0 stays on the Schur route; singular Q != 0 runs on both
    for name, cs in SC.CASES.items():
        assert ("full3x3" in cs["routes"]) == bool(np.any(SC.case_problem(name)[0])), name
    Q = SC.case_problem("unbounded_singular_q")[0]
    assert np.linalg.matrix_rank(Q) == 1 and SC.case_problem("unbounded_singular_q")[1][1:].any()


def test_ray_of_the_equality_case_lies_in_the_equality():
    Q, c, A, b, K, G, d = SC.case_problem("unbounded_eq")
    y = SC.oracle_run("unbounded_eq").y
    assert abs(float((G @ y)[0])) < 1e-6 and y[0] > 0 and abs(y[0] - y[1]) < 1e-6 * abs(y[0])


@pytest.mark.parametrize("name", list(SC.EARLIER))
def test_tolerances_apart_end_the_loop_earlier(name):
    """infeasTol = 1e-3 next to optTol = 1e-9: the certificate is found before the one of infeasTol = optTol, and before the one
    of the default tolerances (for the dual certificate by one iteration only: tests/_stop_cases.py, EARLIER)"""
    o = SC.case_options(name)
    assert (o["infeasTol"], o["optTol"]) == (1e-3, 1e-9)
    against_tight, against_default, same = SC.EARLIER[name]
    loose, tight, dflt = SC.oracle_run(name), SC.oracle_run(name, infeasTol=1e-9), SC.oracle_run(same)
    assert SC.case_problem(name)[1].tolist() == SC.case_problem(same)[1].tolist() and "infeasTol" not in SC.case_options(same)
    assert loose.status == tight.status == dflt.status == SC.CASES[name]["status"]
    assert len(tight.trace) - len(loose.trace) == against_tight >= 2, (len(tight.trace), len(loose.trace))
    assert len(dflt.trace) - len(loose.trace) == against_default >= 1, (len(dflt.trace), len(loose.trace))


def test_group_holds_every_end_state_and_stops_at_different_iterations():
    names = list(SC.GROUP_MEMBERS.values())
    sols = [SC.oracle_run(nm, **SC.GROUP_OPTS) for nm in names]
    assert {s.status for s in sols} == {"Optimal", "Infeasible", "Unbounded", "Abandoned"}
    assert [len(s.trace) for s in sols] == [6, 7, 5, 9]
    assert len({len(s.trace) for s in sols}) == len(sols)                      # no two of them stop in the same iteration
    shapes = set()
    for nm in names:
        Q, c, A, b, K, G, d = SC.case_problem(nm)
        shapes.add((len(c), A.shape, tuple(K), G is None))
    assert shapes == {(10, (20, 10), (("R", 20),), True)}
    # the group's options do not change the one-problem case that is also a member
    assert SC.counts(SC.oracle_run("infeasible_box", **SC.GROUP_OPTS)) == SC.counts(SC.oracle_run("infeasible_box"))
    # the abandoned member's best iterate is not its last one
    ab = SC.oracle_run("narrow_infeasible_box")
    assert ab.status == "Abandoned" and ab.Iter < len(ab.trace) == SC.GROUP_OPTS["maxIters"]
    assert SC.oracle_run("narrow_infeasible_box", maxIters=100).status == "Infeasible"
    # the feasible members are the ones the lock-step test draws
    assert len(SC.lockstep_boxes()) == 3 and SC.case_problem("optimal_box")[1].tolist() == SC.lockstep_boxes()[0][1].tolist()
