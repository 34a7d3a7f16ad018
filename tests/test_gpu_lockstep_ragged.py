"""Ragged lock-step groups (`cip_set_lockstep_ragged(1)`, csrc/lockstep.hip: lockstep_group): problems of one shape whose CSR A or
CSR Q differ in their numbers of non-zeros -- or whose CSR Q take different mat-vec forms -- share a group.  Its slabs are laid out
for the group's largest CSR arrays, the host code's questions about CSR content are asked of the whole group, and the Q mat-vec
runs every slice in its own form (csrc/vecops.hip: k_spmv_csr_forms).

The bar is the lock-step contract of tests/test_gpu_lockstep.py: status, Iter, the counts, the six scalars and the bits of y, w, v
equal `cip_conicip` on each problem alone under the solve block the lock-step call uses.  No tolerance.

Inputs: b = -e (the cone identity), d = 0 and, unless a case says otherwise, Q positive definite: y = 0 is strictly feasible and
every problem ends Optimal whatever A is."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle.cones import vecm
from test_gpu_lockstep_regularized import _assert_identical, _lp, _needs_regularisation
from test_gpu_sparse_q import _raw_batch, q_pattern

pytestmark = pytest.mark.gpu


def _solve(prs, mode, in_flight=4, **kw):
    from cipkkt import _lib as L
    from cipkkt.batch import _solve_problems_native
    lib = L.load()
    prev = lib.cip_set_solve_block_max(lib.cip_lockstep_solve_block_for(len(prs))) if mode == "threads" else None
    try:
        return _solve_problems_native(prs, torch.device("cuda:0"), in_flight, mode, **kw)
    finally:
        if prev is not None:
            lib.cip_set_solve_block_max(prev)


def _stats():
    from cipkkt import _lib as L
    lib = L.load()
    st = (C.c_int * 3)()
    L.check(lib.cip_lockstep_stats(st))
    k = C.c_int(-1)
    L.check(lib.cip_lockstep_regularized(C.byref(k)))
    return tuple(st), k.value


def _switch_is_off():
    from cipkkt.batch import lockstep_ragged
    return lockstep_ragged() == 0


def _identity(cone_dims):
    """e: the identity element of the product cone"""
    parts = []
    for t, k in cone_dims:
        if t == "R":
            parts.append(np.ones(k))
        elif t == "Q":
            parts.append(np.concatenate([[1.0], np.zeros(k - 1)]))
        else:
            r = int(round((np.sqrt(8 * k + 1) - 1) / 2))
            parts.append(vecm(np.eye(r)))
    return np.concatenate(parts)


def _spd(n, rng):
    M = rng.standard_normal((n, n))
    return M @ M.T / n + 0.5 * np.eye(n)


def _problem(Q, A, cone_dims, rng, G=None, route="schur", sparse_q=False, c=None):
    n = Q.shape[0]
    pr = dict(Q=Q, c=rng.standard_normal(n) if c is None else c, A=A, b=-_identity(cone_dims), cone_dims=cone_dims, G=G,
              d=None if G is None else np.zeros(G.shape[0]), kwargs=dict(kktsolver=route) if route != "schur" else {})
    if sparse_q:
        pr["sparse_q"] = True
    return pr


def _nnz(M):
    return int(sp.csr_matrix(M).nnz)


def _csr_density(m, n, density, rng):
    """about `density` of the entries, at least one per column (no variable without a constraint)"""
    M = rng.standard_normal((m, n)) * (rng.random((m, n)) < density)
    for j in range(n):
        if not M[:, j].any():
            M[rng.integers(m), j] = 1.0
    A = sp.csr_matrix(M)
    A.eliminate_zeros()
    A.sort_indices()
    return A


# ------------------------------------------------------------------ A. CSR Q of both mat-vec forms in one group
def _q_form_problems(n, route="schur", kinds=("diag", "rand", "full", "zero"), seed=300):
    prs = []
    for i, kind in enumerate(kinds):
        rng = np.random.default_rng(seed + i)
        Q = q_pattern(kind, n, rng)
        c = rng.standard_normal(n)
        if kind == "zero":
            c = -np.abs(c) - 0.5                             # min -c'y over y >= -1: bounded
        if kind == "rand":
            c[n // 3] = -1.0                                 # (the variable of the empty row: the same)
        prs.append(_problem(Q, sp.identity(n, format="csr"), [("R", n)], rng, route=route, sparse_q=True, c=c))
    return prs


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_csr_q_of_both_forms_share_a_group(route):
    """diag: thread per row; rand (an empty row) and full (nnz = n^2): wave per row; zero: nnz = 0, no entry at all"""
    n = 256
    prs = _q_form_problems(n, route)
    rowmax = [int(np.diff(pr["Q"].indptr).max()) for pr in prs]
    assert rowmax[0] <= 8 < rowmax[1] and rowmax[2] == n and rowmax[3] == 0      # both sides of CIP_SPMV_WAVE_MIN
    assert len({pr["Q"].nnz for pr in prs}) == 4
    one = _solve(prs, "threads", in_flight=1)
    lock = _solve(prs, "lockstep", ragged=True)
    assert _stats() == ((1, 4, 0), 0)
    _assert_identical(lock, one)
    assert [s.status for s in one[:3]] == ["Optimal"] * 3, [s.status for s in one]
    assert _switch_is_off()


# ------------------------------------------------------------------ B. CSR A beside a dense Q at an order that takes the lazy copy
def _lazy_order_problems():
    """n = m = 640 = 5 x 128, p = 0, R cones, dense Q: where a one-entry-per-row CSR A lets the assembly copy Q lazily.  A = I; an A
    of the same nnz with a two-entry row and an empty row; an A with 1-4 entries per row"""
    n = 640
    rng = np.random.default_rng(640)
    A0 = sp.identity(n, format="csr")
    M1 = sp.identity(n, format="lil")
    M1[5, 5] = 0.0                                           # row 5 empty ..
    M1[9, 5] = 0.75                                          # .. row 9 holds (9, 5) and (9, 9)
    A1 = sp.csr_matrix(M1)
    A1.eliminate_zeros()
    A1.sort_indices()
    M2 = sp.identity(n, format="lil")
    for r in range(n):
        for j in rng.choice(n, size=int(rng.integers(0, 4)), replace=False):
            if j != r:
                M2[r, j] = rng.standard_normal()
    A2 = sp.csr_matrix(M2)
    A2.sort_indices()
    assert A1.nnz == A0.nnz and np.diff(A1.indptr).max() == 2 and np.diff(A1.indptr).min() == 0
    assert A2.nnz != A0.nnz and 1 <= np.diff(A2.indptr).min() and np.diff(A2.indptr).max() <= 4
    return [_problem(_spd(n, rng), A, [("R", n)], rng) for A in (A0, A1, A2)]


_LAZY = {}


def _lazy_case():
    """the three problems and their one-problem runs, computed once (under the solve block of a call of 3; a call of 2 uses the same)"""
    if not _LAZY:
        from cipkkt import _lib as L
        lib = L.load()
        assert lib.cip_lockstep_solve_block_for(2) == lib.cip_lockstep_solve_block_for(3)
        prs = _lazy_order_problems()
        _LAZY["prs"], _LAZY["one"] = prs, _solve(prs, "threads", in_flight=1)
        assert [s.status for s in _LAZY["one"]] == ["Optimal"] * 3
    return _LAZY["prs"], _LAZY["one"]


def test_csr_a_of_differing_nnz_at_a_lazy_copy_order():
    prs, one = _lazy_case()
    lock = _solve(prs, "lockstep", ragged=True)
    assert _stats() == ((1, 3, 0), 0)
    _assert_identical(lock, one)


def test_equal_nnz_other_pattern_with_the_switch_off():
    """A = I first and, behind it, an A of the same nnz that is NOT one entry per row: same shape with the switch off.  The group's
    host code runs on problem 0's handle; the lazy copy (a diagonal Schur term) may run only when every problem of the group allows it"""
    prs, one = _lazy_case()
    assert _switch_is_off()
    lock = _solve(prs[:2], "lockstep")
    assert _stats() == ((1, 2, 0), 0)
    _assert_identical(lock, one[:2])


# ------------------------------------------------------------------ C. mixed cones: k_schur_qcols, AtS, k_scatter_negA
@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_mixed_cones_with_csr_a_of_three_densities(route):
    n, p = 100, 5
    cone_dims = [("R", 40), ("Q", 8), ("Q", 8), ("Q", 8), ("S", 6)]
    m = sum(k for _, k in cone_dims)
    prs = []
    for i, density in enumerate((0.1, 0.2, 0.3)):
        rng = np.random.default_rng(900 + i)
        prs.append(_problem(_spd(n, rng), _csr_density(m, n, density, rng), cone_dims, rng, G=rng.standard_normal((p, n)), route=route))
    assert len({pr["A"].nnz for pr in prs}) == 3
    one = _solve(prs, "threads", in_flight=1)
    assert [s.status for s in one] == ["Optimal"] * 3, [s.status for s in one]
    lock = _solve(prs, "lockstep", ragged=True)
    assert _stats() == ((1, 3, 0), 0)
    _assert_identical(lock, one)


# ------------------------------------------------------------------ D. ragged and regularised together
def test_ragged_group_keeps_its_regularised_problems():
    """the LP family of tests/test_gpu_lockstep_regularized.py with a CSR A; problem k carries k + 1 more entries in the two last rows
    (redundant constraints y_0 + sum y_j >= 0 on variables that are >= 0 already)"""
    n = 24
    rng = np.random.default_rng(13)
    prs = []
    for k in range(3):
        pr = _lp(n, rng, csr=True)
        A = pr["A"].tolil()
        for j in range(k + 1):
            A[n - 2 + (j % 2), 2 + j] = 1.0
        pr["A"] = sp.csr_matrix(A)
        pr["A"].sort_indices()
        prs.append(pr)
    assert len({pr["A"].nnz for pr in prs}) == 3 and all(_needs_regularisation(pr) for pr in prs)
    one = _solve(prs, "threads", in_flight=1)
    assert [s.status for s in one] == ["Optimal"] * 3, [s.status for s in one]
    lock = _solve(prs, "lockstep", keep_regularized=True, ragged=True)
    assert _stats() == ((1, 3, 0), 3)
    _assert_identical(lock, one)


# ------------------------------------------------------------------ E. two groups side by side
def test_sixteen_problems_run_as_two_ragged_groups():
    from cipkkt import _lib as L
    lib = L.load()
    n = 128
    kinds = ("diag", "rand", "full", "rand")                 # each group of 8 holds both mat-vec forms
    prs = []
    for i in range(16):
        rng = np.random.default_rng(1600 + i)
        Q = q_pattern(kinds[i % 4], n, rng)
        c = rng.standard_normal(n)
        c[n // 3] = -1.0
        prs.append(_problem(Q, sp.identity(n, format="csr"), [("R", n)], rng, sparse_q=True, c=c))
    assert len({pr["Q"].nnz for pr in prs}) >= 9
    one = _solve(prs, "threads", in_flight=4)
    assert [s.status for s in one] == ["Optimal"] * 16, [s.status for s in one]
    prev = lib.cip_set_lockstep_split(2)
    try:
        lock = _solve(prs, "lockstep", ragged=True)
    finally:
        lib.cip_set_lockstep_split(prev)
    assert _stats() == ((2, 16, 0), 0)
    _assert_identical(lock, one)


# ------------------------------------------------------------------ F. the mixed entry point, and the default
def test_mixed_entry_point_bins_by_the_switch_and_the_default_refuses():
    from cipkkt import _lib as L
    from cipkkt.batch import lockstep_ragged
    lib = L.load()
    prs = _q_form_problems(256)
    assert _switch_is_off()
    rc, ys_off, vs_off, res_off = _raw_batch("cip_conicip_mixed", prs, -7.5)
    assert rc == 0, lib.cip_last_error()
    assert _stats()[0] == (0, 0, 0)                          # four numbers of non-zeros, four bins of one: the thread pool
    prev = lockstep_ragged(True)
    try:
        rc, ys_on, vs_on, res_on = _raw_batch("cip_conicip_mixed", prs, -7.5)
        assert rc == 0, lib.cip_last_error()
        assert _stats()[0] == (1, 4, 0)
    finally:
        lockstep_ragged(prev)
    for i in range(4):
        assert res_on[i].status == res_off[i].status, i
        if L.STATUS_NAMES[res_on[i].status] == "Optimal":
            # (the figure of tests/test_gpu_sparse_q.py for lock-step against the thread pool, whose handles use another solve block)
            np.testing.assert_allclose(ys_on[i], ys_off[i], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(vs_on[i], vs_off[i], rtol=1e-9, atol=1e-12)
    assert [L.STATUS_NAMES[res_on[i].status] for i in range(3)] == ["Optimal"] * 3
    # switched back: the lock-step entry point refuses again, nothing written
    assert _switch_is_off()
    rc, ys, vs, res = _raw_batch("cip_conicip_lockstep", prs, -7.5)
    assert rc == L.E_UNSUPPORTED, (rc, lib.cip_last_error())
    assert all((y == -7.5).all() for y in ys) and all((v == -7.5).all() for v in vs)
