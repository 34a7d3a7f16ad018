"""The switch and the counter of the regularised lock-step groups (include/cipkkt.h: cip_set_lockstep_regularize,
cip_lockstep_regularized) and their Python face, through ctypes on the built library: no device call."""
import ctypes as C
import inspect

from cipkkt import _lib as L


def test_setter_returns_the_previous_value_and_other_values_only_query():
    lib = L.load()
    first = lib.cip_set_lockstep_regularize(-1)
    try:
        assert first == 0                                # the default: such problems leave their group
        assert lib.cip_set_lockstep_regularize(1) == 0
        assert lib.cip_set_lockstep_regularize(1) == 1
        for query in (-1, 2, 7, -100):
            assert lib.cip_set_lockstep_regularize(query) == 1
        assert lib.cip_set_lockstep_regularize(0) == 1
        assert lib.cip_set_lockstep_regularize(-1) == 0
    finally:
        lib.cip_set_lockstep_regularize(first)


def test_counter_refuses_null_and_starts_at_zero():
    lib = L.load()
    assert lib.cip_lockstep_regularized(None) == -1       # CIP_E_INVALID
    k = C.c_int(-1)
    assert lib.cip_lockstep_regularized(C.byref(k)) == 0
    assert k.value == 0                                  # no lock-step call on this thread yet


def test_python_switch_and_keywords():
    from cipkkt import batch
    prev = batch.lockstep_regularize()
    try:
        assert batch.lockstep_regularize(True) == prev
        assert batch.lockstep_regularize() == 1
        assert batch.lockstep_regularize(False) == 1
        assert batch.lockstep_regularize(None) == 0
    finally:
        batch.lockstep_regularize(prev)
    for fn in (batch._solve_problems_native, batch.solve_batch):
        assert inspect.signature(fn).parameters["keep_regularized"].default is False
