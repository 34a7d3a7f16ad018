"""tests/_vec_ref.py on its own (no GPU): the exact dot and the exact fused multiply-add against rational arithmetic, the extended
type, known answers for the bounds, and the row table of the GPU tests against the model of k_gemv_t's aligned path -- every
class of lane the kernel has is reached by some row count."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _vec_ref as R


def _fraction_dot(x, y):
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y)), Fraction(0))


def _cancelling_pair(n, seed):
    """graded magnitudes; y orthogonal to x up to rounding"""
    rng = np.random.default_rng(seed)
    x = R.graded(rng, n, 6.0)
    y = R.graded(rng, n, 6.0)
    return x, (R.orthogonalised(x, y) if n > 1 else y)


@pytest.mark.parametrize("n", [1, 7, 300])
def test_exact_dot_is_the_correctly_rounded_rational_dot(n):
    x, y = _cancelling_pair(n, n)
    exact = _fraction_dot(x, y)
    got = R.exact_dot(x, y)
    assert got == float(exact)                       # Fraction -> float rounds correctly (to nearest even)
    scale = float(np.abs(x * y).sum())
    if n > 1:
        assert abs(got) < 1e-13 * scale, "the pair does not cancel: %g of %g" % (got, scale)
        # ... which is where a plain fp64 dot is wrong in most of its digits: the exact one is not
        assert abs(Fraction(got) - exact) <= Fraction(R.U) * abs(exact)
    # the four partial products are exact
    P = R.partial_products(x, y)
    for i in range(n):
        assert sum(Fraction(float(P[k, i])) for k in range(4)) == Fraction(float(x[i])) * Fraction(float(y[i]))


def test_split_halves_are_short():
    rng = np.random.default_rng(0)
    a = R.graded(rng, 1000, 8.0)
    hi, lo = R.split(a)
    assert np.array_equal(hi + lo, a)
    for h in np.concatenate([hi, lo]):
        m, _ = math.frexp(float(h))
        assert (m * 2.0 ** 26) == int(m * 2.0 ** 26), h            # at most 26 significant bits


def test_exact_matvec_and_csr_are_columns_of_exact_dots():
    rng = np.random.default_rng(5)
    M = R.graded(rng, (37, 9))
    x = rng.standard_normal(37)
    got = R.exact_matvec_t(M, x)
    for j in range(9):
        assert got[j] == float(_fraction_dot(M[:, j], x))
    assert R.exact_matvec_t(np.zeros((0, 3)), np.zeros(0)).tolist() == [0.0, 0.0, 0.0]
    indptr, indices = np.array([0, 3, 3, 4]), np.array([0, 8, 4, 2])
    data = R.graded(rng, 4)
    v = rng.standard_normal(9)
    got = R.exact_csr_matvec(indptr, indices, data, v)
    assert got[0] == float(_fraction_dot(data[:3], v[[0, 8, 4]])) and got[1] == 0.0 and got[2] == data[3] * v[2]


def test_exact_fma_against_fractions():
    rng = np.random.default_rng(11)
    x = R.graded(rng, 200, 6.0)
    a = 1.0 / 3.0
    t = -a * x * (1.0 + rng.standard_normal(200) * 2.0 ** -30)    # a x + t cancels 30 bits: a twice-rounded result differs
    t[:20] = R.graded(rng, 20, 6.0)
    got = R.exact_fma(a, x, t)
    twice = a * x + t
    for i in range(200):
        assert got[i] == float(Fraction(a) * Fraction(float(x[i])) + Fraction(float(t[i]))), i
    assert (got != twice).sum() > 50, "the inputs do not tell a fused multiply-add from a product and a sum"
    assert R.exact_fma(2.0, np.array([3.0]), np.array([0.0]))[0] == 6.0
    # the extended value: 2^-64 of the result, cancellation or not
    ext = R.ld_fma(a, x, t)
    for i in range(200):
        hi = float(ext[i])
        exact = Fraction(a) * Fraction(float(x[i])) + Fraction(float(t[i]))
        assert abs(Fraction(hi) + Fraction(float(ext[i] - R.LD(hi))) - exact) <= Fraction(2.0 ** -64 * (1 + 2.0 ** -50)) * abs(exact), i
    b = rng.standard_normal(200)
    np.testing.assert_array_equal(R.exact_fma(b, x, t), [R.exact_fma(b[i], x[i:i + 1], t[i:i + 1])[0] for i in range(200)])


def test_extended_type_and_ld_matvec():
    assert np.finfo(R.LD).eps < 2 ** -60
    assert R.ld_ok()
    rng = np.random.default_rng(2)
    M, x, y0 = R.graded(rng, (40, 30)), rng.standard_normal(30), rng.standard_normal(40)
    for trans, xx, yy in ((False, x, y0), (True, y0, x)):
        want = R.ld_matvec(0.5, M, xx, -2.0, yy, trans=trans)
        Mo = M.T if trans else M
        for j in range(len(yy)):
            exact = Fraction(0.5) * _fraction_dot(Mo[j], xx) - 2 * Fraction(float(yy[j]))
            scale = 0.5 * float(np.abs(Mo[j] * xx).sum()) + 2 * abs(yy[j])
            hi = float(want[j])
            got = Fraction(hi) + Fraction(float(want[j] - R.LD(hi)))                # the extended value, exactly
            assert abs(got - exact) <= Fraction((len(xx) + 2) * 2.0 ** -64 * scale), (trans, j)
    assert np.array_equal(R.ld_matvec(1.0, M, x, 0.0, np.full(40, np.nan)), M.astype(R.LD) @ x.astype(R.LD))


def test_bound_known_answers():
    assert R.dot_depth(0) == 16 and R.dot_depth(1) == 17 and R.dot_depth(8192) == 17 and R.dot_depth(8193) == 18
    assert R.dot_depth(100003) == 13 + 16
    x = np.array([1.0, -2.0, 4.0])
    assert R.dot_bound(x, x) == 17 * R.U / (1 - 17 * R.U) * 21.0
    b = R.matvec_bound(np.array([0, 5]), -0.5, np.array([2.0, 4.0]), 3.0, np.array([1.0, -1.0]))
    assert b.tolist() == [2 * 2 * R.U * (1.0 + 3.0), 2 * 7 * R.U * (2.0 + 3.0)]
    assert R.matvec_bound(3, 2.0, np.array([1.0]), 0.0, np.array([np.nan])).tolist() == [2 * 5 * R.U * 2.0]
    # a correctly computed fp64 dot, in any order, is inside the bound; one with a term dropped is not
    a, c = _cancelling_pair(300, 4)
    want = R.exact_dot(a, c)
    pairwise = lambda v: float(v[0]) if len(v) == 1 else pairwise(v[:len(v) // 2]) + pairwise(v[len(v) // 2:])
    assert abs(pairwise(a * c) - want) <= R.dot_bound(a, c)               # a tree of depth 9 < 17
    assert abs(pairwise((a * c)[::-1]) - want) <= R.dot_bound(a, c)
    j = int(np.argsort(np.abs(a * c))[150])                               # the median term dropped
    assert abs(pairwise(np.delete(a * c, j)) - want) > R.dot_bound(a, c)


def test_gemv_model_known_answers():
    t = R.gemv_trips(1)
    assert t["tail"].tolist() == [1] + [0] * 63 and all(t[k].sum() == 0 for k in R.TRIPS)
    t = R.gemv_trips(128)
    assert t[128].tolist() == [1] * 64 and t["tail"].sum() == 0 and t[512].sum() == 0
    t = R.gemv_trips(2690)                                                # 2 x 1024, 512, then 130 = 128 + lane 0's second 128
    assert t[1024].tolist() == [2] * 64 and t[512].tolist() == [1] * 64 and t[128].tolist() == [2] + [1] * 63 and t["tail"].sum() == 0
    # every row is read exactly once, whatever the count
    for rows in list(R.GEMV_ROWS) + [4097, 5000]:
        t = R.gemv_trips(rows)
        assert int(2 * (8 * t[1024] + 4 * t[512] + t[128]).sum() + t["tail"].sum()) == rows, rows
        assert t["tail"].sum() == rows % 2


def test_row_table_reaches_every_class_of_lane():
    """each trip taken by all lanes, by some lanes and not by others, the 1024-row trip twice, and the odd tail directly behind each
    kind of trip (and with no trip in front of it)"""
    T = {rows: R.gemv_trips(rows) for rows in R.GEMV_ROWS}
    for kind in R.TRIPS:
        assert any((t[kind] > 0).all() for t in T.values()), "no row count where every lane takes the %d-row trip" % kind
        assert any((t[kind] > 0).any() and (t[kind] == 0).any() for t in T.values()), "%d-row trip: never partial" % kind
        assert any(t["last"][l] == kind for t in T.values() for l in range(64) if t["tail"][l]), "no odd tail behind a %d-row trip" % kind
    assert any((t[1024] >= 2).any() for t in T.values())
    assert any(t["last"][l] is None for t in T.values() for l in range(64) if t["tail"][l])
    # the last count at which a trip is not taken and the first at which it is, for lane 0 and for lane 63
    for reach in (1, 385, 897):
        for lane in (0, 63):
            edge = 2 * lane + reach
            assert edge in R.GEMV_ROWS and edge + 1 in R.GEMV_ROWS, (reach, lane)
    assert max(R.GEMV_ROWS) == 2690
