"""Problems that need the regularised LDL' inside their lock-step group (`cip_set_lockstep_regularize(1)`, csrc/lockstep.hip:
GroupLoop; csrc/solve.hip: the refined solves under a batch mask; csrc/assemble.hip: the regularisation's tile pass).

The bar is the one of tests/test_gpu_lockstep.py: bit-identity with `cip_conicip` on each problem -- status, Iter, n_factor,
n_solve, (y, w, v), the six scalars -- with the one-problem reference run under the solve block the lock-step call uses.

The inputs make the regularisation certain: a variable whose column of A and whose row of Q are zero has an exactly zero pivot
at its column in the static order (Schur route: S_ii = Q_ii + sum_r A_ri^2 f_r = 0 and nothing has been subtracted from it
yet, the rows above it hold zeros there; literal 3x3: the same entry after the elimination of the -F'F block, every term of it
an exact zero).  `_lp` builds that family -- A covers the first n - 2 variables, G pins the last two -- and `_needs_regularisation`
asserts the property on the host before anything is solved."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import problems as P

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers (as in tests/test_gpu_lockstep.py)
def _solve(prs, mode, in_flight=4, keep=False):
    from cipkkt import _lib as L
    from cipkkt.batch import _solve_problems_native
    lib = L.load()
    prev = lib.cip_set_solve_block_max(lib.cip_lockstep_solve_block_for(len(prs))) if mode == "threads" else None
    try:
        return _solve_problems_native(prs, torch.device("cuda:0"), in_flight, mode, keep_regularized=keep)
    finally:
        if prev is not None:
            lib.cip_set_solve_block_max(prev)


def _as_problem(t, **kw):
    Q, c, A, b, cone_dims, G, d = t[:7]
    return dict(Q=Q.toarray() if sp.issparse(Q) else Q, c=c, A=A, b=b, cone_dims=cone_dims, G=G, d=d, kwargs=dict(kw))


def _assert_identical(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.status == y.status, (i, x.status, y.status)
        assert (x.Iter, x.n_factor, x.n_solve) == (y.Iter, y.n_factor, y.n_solve), i
        for f in ("y", "w", "v"):
            assert np.array_equal(getattr(x, f), getattr(y, f), equal_nan=True), (i, f)
        for f in ("Mu", "prFeas", "duFeas", "muFeas", "pobj", "dobj"):
            assert getattr(x, f) == getattr(y, f) or (getattr(x, f) != getattr(x, f) and getattr(y, f) != getattr(y, f)), (i, f)


def _stats():
    from cipkkt import _lib as L
    lib = L.load()
    st = (C.c_int * 3)()
    L.check(lib.cip_lockstep_stats(st))
    k = C.c_int(-1)
    L.check(lib.cip_lockstep_regularized(C.byref(k)))
    return tuple(st), k.value


def _switch_is_off():
    from cipkkt.batch import lockstep_regularize
    return lockstep_regularize() == 0


# ------------------------------------------------------------------ the inputs
def _lp(n, rng, q_cone=False, csr=False, route="schur", bounded=True):
    """min -c'y (the reference's sign: 1/2 y'Qy - c'y) over y_i >= 0 (i < n - 2), y_{n-2} = 1, y_{n-1} = 2: A = [I_{n-2} 0; e_0'; e_1']
    (n rows), Q = 0.  bounded: c < 0 on the constrained variables, the optimum is y = 0 there; else c > 0 as in the family's first
    use (tests/test_gpu_lockstep.py), an unbounded LP.  q_cone: the last five rows of A form a second-order cone instead (-c is kept
    inside its dual cone: the LP stays bounded)."""
    Q = np.zeros((n, n))
    A = np.zeros((n, n))
    A[:n - 2, :n - 2] = np.eye(n - 2)
    A[n - 2, 0] = 1.0
    A[n - 1, 1] = 1.0
    G = np.zeros((2, n))
    G[0, n - 2] = 1.0
    G[1, n - 1] = 1.0
    c = np.concatenate([rng.random(n - 2) + 0.5, [0.0, 0.0]])
    cone_dims = [("R", n)]
    if q_cone:
        cone_dims = [("R", n - 5), ("Q", 5)]
        c[n - 5] = 4.0                                   # > |(c_{n-4}, c_{n-3}, .., ..)| <= sqrt(4 * 1.5^2) = 3
    if bounded:
        c = -c
    return dict(Q=Q, c=c, A=sp.csr_matrix(A) if csr else A, b=np.zeros(n), cone_dims=cone_dims, G=G, d=np.array([1.0, 2.0]),
                kwargs=dict(kktsolver=route) if route != "schur" else {})


def _definite_qp(n, rng, q_cone=False, route="schur"):
    """of the LPs' shape, with a definite Q: no bad pivot.  y = 1 satisfies G y = d; q_cone: b moves (5, 1, 1, 1, 1) into the cone"""
    M = rng.standard_normal((n, n))
    G = rng.standard_normal((2, n))
    b = np.zeros(n)
    if q_cone:
        b[n - 5] = -4.0
    return dict(Q=M @ M.T / n + 0.1 * np.eye(n), c=rng.standard_normal(n), A=np.eye(n), b=b,
                cone_dims=[("R", n - 5), ("Q", 5)] if q_cone else [("R", n)], G=G, d=G @ np.ones(n),
                kwargs=dict(kktsolver=route) if route != "schur" else {})


def _needs_regularisation(pr):
    """some variable has a zero column in A and a zero row in Q: an exactly zero pivot in the static order"""
    A = pr["A"].toarray() if sp.issparse(pr["A"]) else np.asarray(pr["A"])
    Q = np.asarray(pr["Q"])
    free = [i for i in range(Q.shape[0]) if not A[:, i].any() and not Q[i, :].any() and not Q[:, i].any()]
    return len(free) > 0


def _six_of_the_ejection_test():
    """the six problems of tests/test_gpu_lockstep.py::test_problems_that_need_the_regularised_factorisation_leave_the_group"""
    n = 12
    rng = np.random.default_rng(5)
    return [_lp(n, rng, bounded=False) if k % 2 == 0 else _definite_qp(n, rng) for k in range(6)]


# ------------------------------------------------------------------ 1. a mixed group
def test_mixed_group_keeps_its_lps():
    prs = _six_of_the_ejection_test()
    assert [_needs_regularisation(pr) for pr in prs] == [True, False] * 3
    one = _solve(prs, "threads", in_flight=1)
    off = _solve(prs, "lockstep")
    st_off, k_off = _stats()
    assert st_off[:2] == (1, 6) and st_off[2] >= 1 and k_off == 0, (st_off, k_off)
    on = _solve(prs, "lockstep", keep=True)
    st_on, k_on = _stats()
    assert st_on == (1, 6, 0), st_on
    assert k_on == st_off[2], (k_on, st_off)
    _assert_identical(on, one)
    _assert_identical(on, off)
    assert [s.status for s in on[1::2]] == ["Optimal"] * 3
    assert _switch_is_off()


@pytest.mark.parametrize("variant", ["full3x3", "schur-qcone", "full3x3-qcone"])
def test_mixed_group_through_the_generic_solve(variant):
    """the literal 3x3 route, or a Q cone on the Schur route: no fused solve4x4, so the regularised and the other problems of the
    group go through ONE cip_solve3x3_dev call -- the first solve for all of them from the private copy of the right-hand side, the
    refinement under the mask of the regularised ones"""
    parts = variant.split("-")
    rng = np.random.default_rng(15)
    kw = dict(q_cone="qcone" in parts, route=parts[0])
    prs = [_lp(16, rng, **kw) if k % 2 else _definite_qp(16, rng, **kw) for k in range(6)]
    assert [_needs_regularisation(pr) for pr in prs] == [False, True] * 3
    one = _solve(prs, "threads", in_flight=1)
    assert [s.status for s in one] == ["Optimal"] * 6, [s.status for s in one]
    on = _solve(prs, "lockstep", keep=True)
    assert _stats() == ((1, 6, 0), 3)
    _assert_identical(on, one)


# ------------------------------------------------------------------ 2. every problem of the group regularised
@pytest.mark.parametrize("variant", ["schur-dense", "schur-csr", "full3x3-dense", "full3x3-csr", "schur-dense-qcone", "full3x3-csr-qcone"])
def test_all_regularised(variant):
    parts = variant.split("-")
    rng = np.random.default_rng(11)
    prs = [_lp(24, rng, q_cone="qcone" in parts, csr="csr" in parts, route=parts[0]) for _ in range(16)]
    assert all(_needs_regularisation(pr) for pr in prs)
    one = _solve(prs, "threads", in_flight=4)
    assert [s.status for s in one] == ["Optimal"] * 16, [s.status for s in one]
    on = _solve(prs, "lockstep", keep=True)
    st, k = _stats()
    assert st[1] == 16 and st[2] == 0 and k == 16, (st, k)
    _assert_identical(on, one)


# ------------------------------------------------------------------ 3. groups of one and two, and more than 64 problems
@pytest.mark.parametrize("count", [1, 2])
def test_small_groups(count):
    """a group of ONE problem is no batch for the kernels: the group sets the handle's own regularisation (GroupLoop::factor_under)"""
    rng = np.random.default_rng(21)
    prs = [_lp(16, rng) for _ in range(count)]
    assert all(_needs_regularisation(pr) for pr in prs)
    one = _solve(prs, "threads", in_flight=1)
    on = _solve(prs, "lockstep", keep=True)
    st, k = _stats()
    assert st == (1, count, 0) and k == count, (st, k)
    _assert_identical(on, one)


def test_seventy_problems_two_groups_and_side_by_side():
    from cipkkt import _lib as L
    lib = L.load()
    rng = np.random.default_rng(31)
    prs = [_lp(16, rng) if i % 3 else _definite_qp(16, rng) for i in range(70)]
    nreg = sum(_needs_regularisation(pr) for pr in prs)
    assert nreg == 46
    one = _solve(prs, "threads", in_flight=4)
    prev = lib.cip_set_lockstep_split(1)
    try:
        seq = _solve(prs, "lockstep", keep=True)
        st1, k1 = _stats()
        lib.cip_set_lockstep_split(2)
        par = _solve(prs, "lockstep", keep=True)
        st2, k2 = _stats()
    finally:
        lib.cip_set_lockstep_split(prev)
    assert st1 == (2, 70, 0) and st2 == (2, 70, 0), (st1, st2)
    assert k1 == nreg and k2 == nreg, (k1, k2)
    _assert_identical(seq, one)
    _assert_identical(par, one)


# ------------------------------------------------------------------ 4. a pivot the regularisation cannot help
def test_dead_pivot_ends_one_problem_only():
    """variable n - 1 of problem 2 appears nowhere (zero rows in Q, A and G, c = 0): its row of K is zero, so is its delta, and
    the regularised factor has a zero pivot there -- the problem ends as it does alone, the other three do not notice"""
    n = 12
    rng = np.random.default_rng(41)
    prs = [_lp(n, rng) for _ in range(4)]
    G = np.zeros((2, n))
    G[0, n - 2] = 1.0
    G[1, 0] = 1.0                                        # pins y_0 instead of y_{n-1}
    prs[2]["G"] = G
    assert not prs[2]["A"][:, n - 1].any() and not prs[2]["Q"][n - 1].any() and not G[:, n - 1].any() and prs[2]["c"][n - 1] == 0.0
    one = _solve(prs, "threads", in_flight=1)
    on = _solve(prs, "lockstep", keep=True)
    st, k = _stats()
    assert st == (1, 4, 0) and k == 4, (st, k)
    assert on[2].status == one[2].status
    assert one[2].status != "Optimal" and [one[i].status for i in (0, 1, 3)] == ["Optimal"] * 3, [s.status for s in one]
    _assert_identical(on, one)


# ------------------------------------------------------------------ 5. cip_conicip_mixed and solve_batch
def _two_shapes():
    rng = np.random.default_rng(51)
    prs = [_lp(12, rng) for _ in range(4)] + [_as_problem(P.random_mixed(n=16, nq=1, kq=4, p=2, seed=520 + s)) for s in range(3)]
    return [prs[i] for i in (0, 4, 1, 5, 2, 6, 3)]


def test_mixed_entry_point():
    prs = _two_shapes()
    one = _solve(prs, "threads", in_flight=1)
    mixed = _solve(prs, "auto", keep=True)
    st, k = _stats()
    assert st == (2, 7, 0) and k == 4, (st, k)
    _assert_identical(mixed, one)
    assert _switch_is_off()


def test_solve_batch_keyword():
    from cipkkt import _lib as L
    from cipkkt.batch import lockstep_regularize, solve_batch
    lib = L.load()
    prs = _two_shapes()
    prev = lib.cip_set_solve_block_max(lib.cip_lockstep_solve_block_for(len(prs)))
    try:
        one, _ = solve_batch(prs, native="threads", concurrency=1)
    finally:
        lib.cip_set_solve_block_max(prev)
    assert lockstep_regularize() == 0
    got, stats = solve_batch(prs, native=True, keep_regularized=True)
    st, k = _stats()
    assert st == (2, 7, 0) and k == 4, (st, k)
    assert lockstep_regularize() == 0                    # restored
    _assert_identical([got[i] for i in range(len(prs))], [one[i] for i in range(len(prs))])


# ------------------------------------------------------------------ 6. the regularisation, entry by entry
def _graded_symmetric(n, rng, zero=None):
    """symmetric, entries over six orders of magnitude: some rows have their largest entry left of the diagonal (the stored row
    part), some below it (the column part)"""
    M = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, n))
    M = np.tril(M) + np.tril(M, -1).T
    if zero is not None:
        M[zero, :] = 0.0
        M[:, zero] = 0.0
    return M


@pytest.mark.parametrize("rel", [1e-13, 0.5])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_regularisation_entrywise(route, N, rel):
    """cip_set_regularization(h, rel, 0) -> cip_assemble_only -> cip_get_kkt_matrix against numpy's K_ii +- rel max_j |K_ij| on the
    device's own unregularised K, bit for bit: max is exact and order-independent, then one multiply and one add.  Orders around the
    128 x 128 tile of the pass, a matrix with maxima on both sides of the diagonal and an exactly zero row"""
    import cipkkt
    rng = np.random.default_rng(1000 + N)
    if N == 1:
        n, m, p = 1, 0, 0
    else:
        m, p = 3, 2
        n = N - p - (m if route == "full3x3" else 0)
    zero = n // 2 if n >= 3 else None
    Q = _graded_symmetric(n, rng, zero)
    A = G = None
    if m > 0:
        A = rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-2.0, 2.0, (m, n))
        G = rng.standard_normal((p, n)) * 10.0 ** rng.uniform(-2.0, 2.0, (p, n))
        A[:, zero] = 0.0
        G[:, zero] = 0.0
    ks = cipkkt.KKTSystem(Q, A, G, [("R", m)] if m > 0 else [], route=route)
    try:
        assert ks.N == N
        ks.assemble_only()
        K0 = ks.kkt_matrix()
        p0, p1 = (0, n) if route == "schur" else (m, m + n)
        L = np.abs(np.tril(K0[:N, :N]))
        mx = np.maximum(L.max(axis=1), L.max(axis=0))
        if N > 1:
            left = L.max(axis=1) > L.max(axis=0)
            assert left.any() and (~left).any()          # maxima in the row part and in the column part
            assert mx[p0 + zero] == 0.0
        assert ks.lib.cip_set_regularization(ks.h, rel, 0) == 0
        ks.assemble_only()
        K1 = ks.kkt_matrix()
        i = np.arange(N)
        exp = K0.copy()
        delta = rel * mx
        exp[i, i] = K0[i, i] + np.where((i >= p0) & (i < p1), delta, -delta)
        low = np.tri(ks.Npad, dtype=bool)
        bad = low & (K1.view(np.int64) != exp.view(np.int64))
        assert not bad.any(), np.argwhere(bad)[:5].tolist()
        assert np.array_equal(K1[i, i] != K0[i, i], mx > 0.0)      # |delta| >= rel |K_ii| > an ulp of K_ii wherever the row is not zero
    finally:
        ks.close()


# ------------------------------------------------------------------ 7. a group that is switched in the middle of the loop
def test_group_switched_at_a_later_factorisation():
    """The wrong-sign kind of the test hook cip_debug_chain_giveup (2^28, with a skip count) sets the pivot flag through a batched
    launch: it reaches every problem of the lock-step launch it fires behind.  Four definite QPs therefore join the regularised
    factorisation together at their FOURTH factorisation -- with iterates, scalings and the fused solve4x4 path behind them -- and
    must go on exactly as each does alone under the same hook."""
    from cipkkt import _lib as L
    lib = L.load()
    hook = 1 | (3 << 16) | (1 << 28)                     # one firing, after three factorisations left alone, wrong-sign kind
    rng = np.random.default_rng(71)
    prs = [_definite_qp(12, rng) for _ in range(4)]
    assert not any(_needs_regularisation(pr) for pr in prs)
    plain = _solve(prs, "lockstep", keep=True)
    assert _stats() == ((1, 4, 0), 0)
    assert all(s.status == "Optimal" and s.n_factor > 4 for s in plain), [(s.status, s.n_factor) for s in plain]
    one = []
    try:
        for pr in prs:
            lib.cip_debug_chain_giveup(hook)
            one += _solve([pr], "threads", in_flight=1)
            assert lib.cip_debug_chain_giveup(-1) == 0   # the hook fired
        lib.cip_debug_chain_giveup(hook)
        on = _solve(prs, "lockstep", keep=True)
        assert lib.cip_debug_chain_giveup(-1) == 0
    finally:
        lib.cip_debug_chain_giveup(0)
    assert _stats() == ((1, 4, 0), 4)
    _assert_identical(on, one)
    assert all(s.status == "Optimal" for s in on)
