"""The diagonal kernel of the blocked LDL' (csrc/diag.hip) at the orders where it is most of the factorisation: 128 (one panel:
the diagonal kernel alone, no TRSM strips), 256 and 384 (two and three panels), on matrices that reach its corners --
  * an SPD matrix whose diagonal is graded from 1e-150 to 1e150 (every pivot through the reciprocal path at the ends of the range),
  * quasi-definite matrices whose sign change falls inside a block of four pivots (columns 13 | 14) and on a micro-panel
    boundary (columns 15 | 16 and 63 | 64),
  * an exact zero pivot and a wrong-sign pivot at column 17 (0-based), which the factorisation must report at that column: through
    cip_ldlt_factor_dev (flag word 0: the first bad pivot) and through a handle, which knows the signs -- without regularisation
    it reports flag word 0 (first bad pivot of any kind), with a static regularisation in force flag word 2 (first zero /
    non-finite pivot; a wrong-sign one is then accepted).
The factor and a solve are judged entrywise by tests/_ldlt_ref.py under that module's own bounds (C_F, C_S), and the fused panel
chain and the three-launch chain, which share the diagonal kernel's body, must agree bit for bit."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _ldlt_ref as R

pytestmark = pytest.mark.gpu

F64 = dict(dtype=torch.float64, device="cuda")
ORDERS = (128, 256, 384)
BAD = 17                                  # 0-based column of the planted pivot: second column of the second micro-panel


@pytest.fixture(scope="module")
def lib():
    import cipkkt
    return cipkkt._lib.load()


@contextlib.contextmanager
def chain_knob(lib, chain):
    prev = (lib.cip_set_ldlt_fused_chain(chain), lib.cip_set_solve_block_max(1024), lib.cip_set_solve_fused(0))
    try:
        yield
    finally:
        lib.cip_set_ldlt_fused_chain(prev[0])
        lib.cip_set_solve_block_max(prev[1])
        lib.cip_set_solve_fused(prev[2])


def _spd(n, rng):
    M = rng.standard_normal((n, n))
    return M @ M.T / n + np.eye(n)


@functools.lru_cache(maxsize=None)
def graded(N):
    """D^(1/2) (I + 1e-3 R) D^(1/2), R symmetric with entries in [-1, 1] and a zero diagonal, D = 1e-150 .. 1e150: SPD (a
    diagonal scaling of a matrix within 0.4 of the identity), every entry sqrt(d_i d_j) times a number of order one"""
    rng = np.random.default_rng([1, N])
    d = 10.0 ** np.linspace(-150.0, 150.0, N)
    Rm = np.tril(rng.uniform(-1.0, 1.0, (N, N)), -1)
    K = 1e-3 * np.sqrt(np.outer(d, d)) * (Rm + Rm.T)
    K[np.arange(N), np.arange(N)] = d
    K.setflags(write=False)
    return R.Case("graded(%d)" % N, K, N, (0, N)), np.sqrt(d)


@functools.lru_cache(maxsize=None)
def quasi(N, p1):
    """[[A, B'], [B, -C]], A (p1 x p1) and C SPD: pivots 0 .. p1-1 positive, the rest negative, in this order"""
    rng = np.random.default_rng([2, N, p1])
    K = np.zeros((N, N))
    K[:p1, :p1] = _spd(p1, rng)
    K[p1:, p1:] = -_spd(N - p1, rng)
    B = rng.standard_normal((N - p1, p1)) / np.sqrt(N)
    K[p1:, :p1] = B
    K[:p1, p1:] = B.T
    K.setflags(write=False)
    return R.Case("quasi(%d,%d)" % (N, p1), K, N, (0, p1)), np.ones(N)


def _factor(lib, K, expect_info=0):
    """(factor as the device stores it, info, workspace, device buffer) of cip_ldlt_factor_dev"""
    from cipkkt import _lib as L
    N = K.shape[0]
    nb = C.c_size_t()
    L.check(lib.cip_ldlt_workspace_bytes(N, C.byref(nb)))
    ws = torch.zeros(nb.value // 8 + 8, **F64)
    buf = torch.as_tensor(np.array(K), **F64).t().contiguous()
    info = C.c_int(-1)
    L.check(lib.cip_ldlt_factor_dev(None, buf.data_ptr(), N, N, ws.data_ptr(), C.byref(info)))
    torch.cuda.synchronize()
    assert info.value == expect_info, "reported column %d, expected %d" % (info.value, expect_info)
    return buf.t().cpu().numpy(), ws, buf


def _solve(lib, buf, ws, b):
    from cipkkt import _lib as L
    N = buf.shape[0]
    x = torch.as_tensor(b, **F64).clone()
    L.check(lib.cip_ldlt_solve_dev(None, buf.data_ptr(), N, N, ws.data_ptr(), x.data_ptr()))
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _factor_and_solve_both_chains(lib, case, scale):
    K, N = np.asarray(case.K), case.K.shape[0]
    _, Bs, _ = R.dispatch(N, 3, 0, 1024, 0)
    b = np.random.default_rng(N).standard_normal(N) * scale
    got = {}
    for chain in (3, 0):
        with chain_knob(lib, chain):
            F, ws, buf = _factor(lib, K)
            got[chain] = (F, _solve(lib, buf, ws, b))
    F, x = got[3]
    fc = R.factor_check(K, F)
    print("FACTOR | %s | %d | |E| <= %.3g x bound at %s, %.1f u B, micro |L11||inv L11| <= %.3g"
          % (case.name, N, fc["ratio"], fc["at"], fc["textbook"], fc["micro"]))
    assert np.isfinite(np.tril(F)).all(), case.name
    assert fc["ok"], (case.name, fc)
    assert np.array_equal(np.sign(np.diag(F)), R.expected_signs(case)), case.name
    sc = R.SolveBound(F, Bs).check(b, x, R.C_S["gemv"])
    print("SOLVE | %s | %d | Bs %d | %.3g x bound, %.3g x plain substitution bound" % (case.name, N, Bs, sc["ratio"], sc["plain"]))
    assert sc["ok"], (case.name, {k: v for k, v in sc.items() if k not in ("r", "bound")})
    # the two chains share diag_body: same bits (lower triangle: the part above the diagonal blocks' diagonal is undefined)
    assert np.array_equal(np.tril(got[0][0]), np.tril(F)), case.name + ": the three-launch chain's factor differs"
    assert np.array_equal(got[0][1], x), case.name + ": the three-launch chain's solve differs"


@pytest.mark.parametrize("N", ORDERS)
def test_graded_spd_factor_and_solve(lib, N):
    case, scale = graded(N)
    _factor_and_solve_both_chains(lib, case, scale)


@pytest.mark.parametrize("p1", [14, 16, 64])
@pytest.mark.parametrize("N", ORDERS)
def test_quasi_definite_sign_change_at_block_and_micro_panel_boundaries(lib, N, p1):
    case, scale = quasi(N, p1)
    _factor_and_solve_both_chains(lib, case, scale)


def _block_diagonal_with(N, value):
    """[[S1, 0], [0, S2]], S1 of order BAD, S2[0, 0] = value: pivot BAD is exactly `value` (nothing of S1 reaches S2)"""
    rng = np.random.default_rng([3, N])
    K = np.zeros((N, N))
    K[:BAD, :BAD] = _spd(BAD, rng)
    K[BAD:, BAD:] = _spd(N - BAD, rng)
    K[BAD, BAD] = value
    return K


@pytest.mark.parametrize("N", ORDERS)
def test_zero_pivot_is_reported_at_its_column_by_both_chains(lib, N):
    K = _block_diagonal_with(N, 0.0)
    factors = []
    for chain in (3, 0):
        with chain_knob(lib, chain):
            F, _, _ = _factor(lib, K, expect_info=BAD + 1)
            factors.append(F)
    # the micro-panel in front of the bad pivot's (columns 0 .. 15) is final and finite: the factor of S1's leading block; in the
    # bad pivot's own micro-panel the in-place rank-4 updates carry the NaN into finished columns too (diag.hip: 0 * NaN), which
    # is why the column is reported from the reciprocals.  The two chains agree on all of it.
    assert np.isfinite(np.tril(factors[0])[:, :16]).all()
    assert np.array_equal(np.tril(factors[0]), np.tril(factors[1]), equal_nan=True)


def _handle_with_pivot(N, value, rel):
    """a Schur-route handle (it knows which pivots must be positive) whose matrix Q + A'A, A = I, is block diagonal as above with
    pivot BAD = value; row BAD is otherwise zero, so a static regularisation (relative to the row's largest entry) leaves an
    exact zero exactly zero.  Automatic regularisation off, static regularisation `rel`."""
    import cipkkt
    Q = _block_diagonal_with(N, 1.0) - np.eye(N)
    Q[BAD, :] = 0.0
    Q[:, BAD] = 0.0
    Q[BAD, BAD] = value - 1.0
    ks = cipkkt.KKTSystem(Q, sp.identity(N, format="csr"), None, [("R", N)], route="schur")
    from cipkkt import _lib as L
    L.check(ks.lib.cip_set_regularization(ks.h, rel, 0))
    ks.set_scaling_identity()
    return ks


@pytest.mark.parametrize("chain", [3, 0])
@pytest.mark.parametrize("N", ORDERS)
def test_handle_names_the_zero_and_the_wrong_sign_pivot(lib, N, chain):
    from cipkkt._lib import CipError
    with chain_knob(lib, chain):
        # the matrix is what the construction says (the assembly adds A'A = I exactly)
        ks = _handle_with_pivot(N, 0.0, 0.0)
        ks.assemble_only()
        torch.cuda.synchronize()
        K = ks.kkt_matrix()
        # (the lower triangle: the assembly writes nothing above the diagonal outside the diagonal blocks)
        assert K[BAD, BAD] == 0.0 and not K[BAD, :BAD].any() and not K[BAD + 1:N, BAD].any() and K[BAD + 1, BAD + 1] > 0.0
        ks.close()
        for value, rel, flag in ((0.0, 0.0, "first bad pivot"), (0.0, 1e-13, "first zero pivot, regularised"),
                                 (-3.0, 0.0, "first bad pivot: wrong sign")):
            ks = _handle_with_pivot(N, value, rel)
            with pytest.raises(CipError, match=r"pivot at column %d\b" % (BAD + 1)) as e:
                ks.factor(check=True)
            assert ("regularised" in str(e.value)) == (rel > 0.0), (flag, str(e.value))
            ks.close()
        # a wrong-sign pivot is no zero pivot: under a static regularisation the factorisation stands, the pivot as planted
        ks = _handle_with_pivot(N, -3.0, 1e-13)
        ks.factor(check=True)
        assert -3.0 <= ks.kkt_matrix()[BAD, BAD] <= -3.0 + 1e-12          # (+ rel x the row's largest entry)
        ks.close()
