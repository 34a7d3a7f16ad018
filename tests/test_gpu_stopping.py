"""The interior-point loop's end states other than :Optimal through the device (csrc/driver.hip: cip_conicip; cipkkt/driver.py, its
per-operation twin): :Infeasible, :Unbounded and :Abandoned on both routes and both drivers.

The cases, the oracle's verdict on each and the tolerances (10 x the oracle's own spread between its two solvers, floor 1e-12)
are in tests/_stop_cases.py; tests/test_stop_cases.py checks them on the oracle without a GPU.  Here, per case:
  a. against the oracle: status, Iter (the best iterate's index, not the last iteration), trace rows, n_factor, n_solve, Mu and the
     feasibilities of the best iterate, pobj, dobj, and the returned y, w, v block by block -- a NaN block NaN in full, a finite
     one relative to its own norm; for :Abandoned that is the last iterate itself
  b. what a certificate must satisfy whoever computed it, with bounds taken from the stopping test
  c. the native loop and the Python driver agree bit for bit, certificates included
The lock-step group that holds every end state is tests/test_gpu_lockstep.py::test_statuses_differ_inside_one_group.
:Error is not reached here: it needs non-finite data (tests/test_stop_verdict.py tests it on scalars)."""
import numpy as np
import pytest

import _stop_cases as SC

pytestmark = pytest.mark.gpu

RUNS = [(name, route) for name, cs in SC.CASES.items() for route in cs["routes"]]


def _device(name, route, driver):
    import cipkkt
    Q, c, A, b, K, G, d = SC.case_problem(name)
    return cipkkt.conicIP(Q, c, A, b, K, G, d, kktsolver=route, driver=driver, **SC.case_options(name))


@pytest.mark.parametrize("name,route", RUNS)
def test_end_state_against_the_oracle(name, route):
    cs = SC.CASES[name]
    nat, py = _device(name, route, "native"), _device(name, route, "python")
    for drv, got in (("native", nat), ("python", py)):
        assert got.status == cs["status"], (name, route, drv, got.status)
        SC.assert_matches_oracle(got, name, "%s %s" % (route, drv))
        if cs["status"] != "Abandoned":
            SC.assert_certificate(got, name, "%s %s" % (route, drv))
        else:
            assert "alpha" in got.trace[-1] and len(got.trace) == SC.case_options(name)["maxIters"]
    # c. one loop, stated twice
    assert SC.counts(nat) == SC.counts(py), (name, route, SC.counts(nat), SC.counts(py))
    for f in ("y", "w", "v"):
        assert np.array_equal(getattr(nat, f), getattr(py, f), equal_nan=True), (name, route, f)
    for f in SC.FIELDS:
        assert getattr(nat, f) == getattr(py, f), (name, route, f, getattr(nat, f), getattr(py, f))
    for tn, tp in zip(nat.trace, py.trace):
        assert tn == tp, (name, route, tn, tp)
