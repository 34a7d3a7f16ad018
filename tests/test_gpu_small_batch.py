"""cip_conicip_small on the GPU (csrc/small.hip: one workgroup per problem): every problem's trajectory against the oracle with
the measures and tolerances of tests/test_gpu_driver.py, the shape edges of its tiles and limits, independence of a problem's
bits from count, position, run and pointer kind, different fates in one batch (with the hand-over to cip_conicip_mixed),
launch and read-back counts that do not depend on count, agreement with the lock-step path, and the refusals.

The iterates differ from the other paths' in rounding, so the inputs are ones for which the oracle's iteration count is robust
(tests/_small_cases.py: robust(); the seeds are listed there and nothing is filtered here).  The oracle's answers are computed
once per case and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import _small_cases as S
import problems as P
from oracle.conicip import conicIP as oracle_conicIP
from test_gpu_driver import OPT, TOL, assert_same_trajectory

pytestmark = pytest.mark.gpu
KAT_KW = dict(optTol=OPT, DTB=0.01, maxRefinementSteps=3)


def solve_small(probs, **kw):
    from cipkkt import batch
    return batch.solve_small([S.as_dict(p) for p in probs], **kw)


@functools.lru_cache(maxsize=None)
def kat_oracle(name):
    return oracle_conicIP(*getattr(P, name)()[:7], **KAT_KW)


# ---------------------------------------------------------------- 1. trajectory against the oracle, per problem
@pytest.mark.parametrize("name", ["sphere", "simplex", "combined"])
def test_reference_kats(name):
    prob = getattr(P, name)()
    for got in solve_small([prob, prob], **KAT_KW):
        assert got.status == "Optimal"
        assert np.linalg.norm(got.y - prob[7]) < TOL           # the reference's own assertion
        assert_same_trajectory(got, kat_oracle(name))


@pytest.mark.parametrize("name, status", [("infeasible_box", "Infeasible"), ("infeasible_eq", "Infeasible"), ("unbounded", "Unbounded")])
def test_certificates(name, status):
    prob = getattr(P, name)()
    ref = kat_oracle(name)
    assert ref.status == status
    for got in solve_small([prob, prob], **KAT_KW):
        assert_same_trajectory(got, ref)
        for f in ("y", "w", "v"):                                # the certificate's scaling and its NaN block
            np.testing.assert_allclose(getattr(got, f), getattr(ref, f), rtol=1e-6, atol=1e-9, equal_nan=True)


def test_abandoned():
    prob = P.simplex()
    ref = oracle_conicIP(*prob[:7], optTol=OPT, maxIters=2)
    got, = solve_small([prob], optTol=OPT, maxIters=2)
    assert got.status == ref.status == "Abandoned"
    assert (got.Iter, got.n_factor, got.n_solve) == (ref.Iter, ref.n_factor, ref.n_solve)
    np.testing.assert_allclose(got.y, ref.y, rtol=1e-9, atol=1e-12)


def test_random_mixed_seeds_in_one_batch():
    probs = [P.random_mixed(n=60, nq=4, kq=7, p=5, seed=s) for s in S.MIXED_SEEDS]
    gots = solve_small(probs, optTol=1e-8)
    for got, prob in zip(gots, probs):
        assert got.status == "Optimal"
        assert_same_trajectory(got, oracle_conicIP(*prob[:7], optTol=1e-8))


# ---------------------------------------------------------------- 2. shape edges
@pytest.mark.parametrize("shape, cones", S.EDGE_SHAPES, ids=[str(s) for s, _ in S.EDGE_SHAPES])
def test_shape_edges(shape, cones):
    n, m, p = shape
    assert sum(k for _, k in cones) == m
    probs = [S.cone_problem(n, p, cones, 1000 + s) for s in S.EDGE_SEEDS[shape]]
    assert len(probs) == 5
    gots = solve_small(probs, optTol=S.OPT_EDGE)
    for got, prob in zip(gots, probs):
        assert got.status == "Optimal"
        assert_same_trajectory(got, oracle_conicIP(*prob, optTol=S.OPT_EDGE))


# ---------------------------------------------------------------- 3. count and position
def bits(sol):
    return sol.y.tobytes() + sol.w.tobytes() + sol.v.tobytes() + np.array([sol.pobj, sol.dobj, sol.Mu]).tobytes()


def test_count_and_position():
    """3000 problems of (8, 16, 0) -- more workgroups than can be resident: a problem's bits are those of the same problem solved
    alone, whatever its index; two identical calls agree; host and device pointers agree"""
    from cipkkt import batch
    probs = [S.as_dict(S.cone_problem(8, 0, [("R", 16)], 9000 + i)) for i in range(3000)]
    first = batch.solve_small(probs, optTol=OPT)
    st = batch.small_stats()
    assert st["finished"] == 3000 and st["handed_over"] == 0
    assert all(s.status == "Optimal" for s in first)
    assert len({s.Iter for s in first}) > 1                      # (the live list shrinks along the way)
    picks = [0, 1, 1499, 2998, 2999]
    for i in picks:
        alone, = batch.solve_small([probs[i]], optTol=OPT)
        assert (alone.status, alone.Iter, alone.n_factor, alone.n_solve) == (first[i].status, first[i].Iter, first[i].n_factor, first[i].n_solve)
        assert bits(alone) == bits(first[i]), i
    ref = oracle_conicIP(*S.cone_problem(8, 0, [("R", 16)], 9000 + 1499), optTol=OPT)
    assert first[1499].status == ref.status and np.linalg.norm(first[1499].y - ref.y) / (1 + np.linalg.norm(ref.y)) < 1e-6
    second = batch.solve_small(probs, optTol=OPT)
    assert [bits(s) for s in second] == [bits(s) for s in first]
    sub = [probs[i] for i in picks]
    host, dev = batch.solve_small(sub, optTol=OPT), batch.solve_small(sub, pointers="device", optTol=OPT)
    assert [bits(s) for s in host] == [bits(s) for s in dev] == [bits(first[i]) for i in picks]


# ---------------------------------------------------------------- 4. different fates in one batch
def test_different_fates_in_one_batch():
    from cipkkt import batch
    names, probs = zip(*S.fates())
    refs = [oracle_conicIP(*pr, optTol=OPT) for pr in probs]
    assert len({r.Iter for r, nm in zip(refs, names) if nm.startswith("qp")}) == 3
    assert [r.status for r in refs][3:] == ["Infeasible", "Unbounded", "Optimal"]
    gots = solve_small(probs, optTol=OPT)
    st = batch.small_stats()
    assert st["handed_over"] == 1 and st["finished"] == len(probs) - 1, st
    for nm, got, ref in zip(names, gots, refs):
        assert_same_trajectory(got, ref)
        if ref.status != "Optimal":
            for f in ("y", "w", "v"):
                np.testing.assert_allclose(getattr(got, f), getattr(ref, f), rtol=1e-6, atol=1e-9, equal_nan=True)
    # the problem the kernels could not finish: cip_conicip_mixed's result on it alone, bit for bit -- and that is the oracle's answer
    k = names.index("free_lp")
    alone = batch._solve_problems_native([S.as_dict(probs[k], optTol=OPT)], "cuda:0", 4, "auto")[0]
    assert bits(gots[k]) == bits(alone)
    assert (gots[k].status, gots[k].Iter, gots[k].n_factor, gots[k].n_solve) == (alone.status, alone.Iter, alone.n_factor, alone.n_solve)
    assert gots[k].status == refs[k].status == "Optimal"
    assert np.linalg.norm(gots[k].y - refs[k].y) / (1 + np.linalg.norm(refs[k].y)) < 1e-6


# ---------------------------------------------------------------- 5. launch and read-back counts
def test_launches_and_readbacks_do_not_depend_on_count():
    """at most 2 launches and 1 read-back per iteration plus 2 launches and 1 read-back per call (include/cipkkt.h), for 1 problem
    and for 500 whose slowest takes the same number of iterations"""
    from cipkkt import batch
    slow = S.as_dict(S.cone_problem(6, 1, [("R", 6)], 28, q_scale=0.02))          # 10 iterations
    fast = S.as_dict(S.cone_problem(6, 1, [("R", 6)], 26))                        # 5
    one, = batch.solve_small([slow], optTol=OPT)
    st1 = batch.small_stats()
    many = batch.solve_small([fast] * 499 + [slow], optTol=OPT)
    st500 = batch.small_stats()
    assert max(s.Iter for s in many) == one.Iter == 10 and many[0].Iter == 5
    assert (st1["launches"], st1["readbacks"]) == (st500["launches"], st500["readbacks"])
    assert st1["launches"] <= 2 * one.Iter + 2 and st1["readbacks"] <= one.Iter + 1
    assert st500["finished"] == 500 and st1["finished"] == 1


# ---------------------------------------------------------------- 6. agreement with the other product path
def test_agrees_with_lockstep():
    from cipkkt import batch
    K = [("R", 100), ("Q", 28)]
    probs = [S.as_dict(S.cone_problem(64, 8, K, 5000 + s), optTol=OPT) for s in S.LOCKSTEP_SEEDS]
    assert len(probs) == 64
    small = batch.solve_small(probs)
    lock = batch._solve_problems_native(probs, "cuda:0", 4, "lockstep")
    batch.release_cached_memory()
    for a, b in zip(small, lock):
        assert a.status == b.status == "Optimal" and a.Iter == b.Iter
        for f in ("y", "w", "v"):
            x, y = getattr(a, f), getattr(b, f)
            assert np.linalg.norm(x - y) / (1 + np.linalg.norm(y)) < 1e-6


# ---------------------------------------------------------------- 7. refusals on the device
def _raw_call(structs, n, m, p):
    """cip_conicip_small on ready-made structs with sentinel-filled outputs; returns (rc, outputs untouched)"""
    from cipkkt import _lib as L
    lib = L.load()
    k = len(structs)
    arr = (L.CipProblem * k)(*structs)
    vp = C.c_void_p * k
    ins = [np.ones(max(x, 1)) for x in (n, m, p)]
    outs = [[np.full(max(x, 1), -7.25) for _ in range(k)] for x in (n, p, m)]
    res = (L.CipResult * k)()
    C.memset(res, 0x5a, C.sizeof(res))
    ptrs = lambda xs: vp(*[x.ctypes.data for x in xs])
    rc = lib.cip_conicip_small(k, arr, ptrs([ins[0]] * k), ptrs([ins[1]] * k), ptrs([ins[2]] * k), None, ptrs(outs[0]), ptrs(outs[1]), ptrs(outs[2]), res)
    clean = all(np.all(o == -7.25) for grp in outs for o in grp) and bytes(res) == b"\x5a" * C.sizeof(res)
    return rc, clean


def test_refusals_write_nothing():
    from test_small_batch_args import REFUSED, description
    from cipkkt import _lib as L
    for label, make in REFUSED:
        st, keep = description(make)
        rc, clean = _raw_call([st, st], st.n, st.m, st.p)
        assert rc == L.E_UNSUPPORTED, label
        assert clean, label


# ---------------------------------------------------------------- the Python keyword
def test_solve_batch_small_keyword():
    """solve_batch(small=True): the bins that fit get solve_small's bits, the rest what they get without the keyword"""
    from cipkkt import batch
    a = [S.as_dict(S.cone_problem(6, 1, [("R", 6)], s), optTol=OPT) for s in (26, 13)]
    big = S.as_dict(P.random_mixed(n=200, nq=3, kq=6, p=4, seed=77), optTol=OPT)          # n + p > 128
    probs = [a[0], big, a[1]]
    sols, stats = batch.solve_batch(probs, small=True)
    direct = batch.solve_small(a)
    assert bits(sols[0]) == bits(direct[0]) and bits(sols[2]) == bits(direct[1])
    plain, _ = batch.solve_batch(probs)
    assert bits(sols[1]) == bits(plain[1])
    assert stats["n_problems"] == 3 and stats["n_optimal"] == 3
