"""Self-test of tests/_cone_ref.py (CPU): the mpmath references reproduce known answers, and the fp64 oracle -- an
independent implementation with its own summation order (QF(z) = 2 z0^2 - z.z, numpy's pairwise sums, LAPACK) --
meets every bound on the same hard iterates the device is tested at, so the bounds are not tuned to the kernels."""
import mpmath as mp
import numpy as np
import pytest

import _cone_ref as CR
from oracle import cones as oc
from oracle.conicip import make_cone_ops

GAPS = [1e-2, 1e-6, 1e-10]


def _within(got, ref_evs):
    err = np.abs(np.asarray(got, dtype=np.float64) - CR.values(ref_evs))
    assert np.all(err <= CR.bounds(ref_evs)), (err / CR.bounds(ref_evs)).max()


def test_known_answers():
    z = np.array([3.0, 1.0, -2.0, 0.5])
    beta, w, lam = CR.q_nt(z, z)                                   # z = s: the NT scaling is the identity
    assert abs(beta.v - 1) < mp.mpf(10) ** -40
    assert abs(w[0].v - mp.sqrt(2)) < mp.mpf(10) ** -40 and all(abs(t.v) < mp.mpf(10) ** -40 for t in w[1:])
    assert all(abs(a.v - b) < mp.mpf(10) ** -40 for a, b in zip(lam, z))
    e = np.eye(1, 5)[0]
    st, _ = CR.step_of(CR.q_maxstep(e, e, 1.0))                    # e - alpha e leaves Q at alpha = 1
    assert abs(st - 1) < mp.mpf(10) ** -40
    assert CR.r_maxstep(np.ones(7), np.ones(7), 1.0) == 1.0
    assert CR.q_maxstep_none(e).v == -1
    prod = CR.q_prod(z, e)
    assert CR.values(prod).tolist() == z.tolist()
    sv, _, _, _ = CR.s_nt(CR.vecm(np.eye(4)), CR.vecm(np.eye(4)))
    assert np.array_equal(sv, np.ones(4))
    assert CR.lambda_min_within(CR.mat(CR.vecm(np.diag([2.0, 3.0, 5.0])), CR.LD), 2.0, 1e-12)
    assert not CR.lambda_min_within(CR.mat(CR.vecm(np.diag([2.0, 3.0, 5.0])), CR.LD), 2.1, 1e-3)


@pytest.mark.parametrize("k", [1, 2, 8, 65, 300])
@pytest.mark.parametrize("gz", GAPS)
@pytest.mark.parametrize("gs", GAPS)
def test_oracle_meets_the_q_bounds(k, gz, gs):
    rng = np.random.default_rng(k * 7 + int(-np.log10(gz)) * 3 + int(-np.log10(gs)))
    z, s = CR.q_point(k, gz, rng), CR.q_point(k, gs, rng)
    beta, w, lam = CR.q_nt(z, s)
    ob, ow = oc.nestod_soc(z, s)
    assert abs(ob - float(beta.v)) <= beta.bound()
    _within(ow, w)
    _, nt_scaling, _, _ = make_cone_ops([("Q", k)])
    F = nt_scaling(z, s)
    _within(F.mul(z), lam)
    x = rng.standard_normal(k) * 10.0 ** rng.uniform(-4, 4, k)
    _within(F.mul(x), CR.q_apply(ob, ow, x, False))
    # F^-1 = J F J / beta^2 (QF(w) = 2 beta), the form k_apply evaluates; the oracle's Woodbury inverse of the block
    # agrees with it only to the rounding of that identity, so numpy evaluates the closed form here
    J = np.ones(k)
    J[1:] = -1.0
    _within(J * F.mul(J * x) / ob ** 2, CR.q_apply(ob, ow, x, True))
    _within(oc.xsoc(x, z), CR.q_prod(x, z))
    _within(oc.dsoc(x, z), CR.q_div(x, z))
    for kind in ("one", "far", "never"):
        d = CR.q_direction(z, kind, rng)
        for scale in (1.0, 1.0 / 0.99):
            alpha = CR.q_maxstep(z, d, scale)
            got = oc.maxstep_soc(z, d * scale)
            for label, err, bnd in CR.q_step_errors(alpha, got):
                assert err <= bnd, (kind, label, float(err / bnd))
            st = CR.step_of(alpha)
            if st is not None and st[0] != mp.inf:
                dist, slope = CR.q_distance(z, d, scale, got)
                assert abs(dist) <= slope * st[1]
    if k > 1:
        xo = z.copy()
        xo[0] = -np.linalg.norm(z[1:]) * 0.5
        a = CR.q_maxstep_none(xo)
        assert abs(mp.mpf(oc.maxstep_soc(xo, None)) - (-1 - a.v)) <= a.bound() + 2 * CR.U * abs(1 + float(a.v))


def test_r_reference_is_the_oracle_bit_for_bit():
    rng = np.random.default_rng(3)
    x = 10.0 ** rng.uniform(-12, 12, 5000)
    for _ in range(4):
        d = rng.standard_normal(5000) * 10.0 ** rng.uniform(-6, 6, 5000)
        assert CR.r_maxstep(x, d, 1.0) == oc.maxstep_rp(x, d)
    assert CR.r_maxstep(x, -np.abs(d), 1.0) == oc.maxstep_rp(x, -np.abs(d)) == np.inf
    xn = x.copy()
    xn[17] = np.nan
    d[17] = 1.0
    assert np.isnan(CR.r_maxstep(xn, d, 1.0)) and np.isnan(oc.maxstep_rp(xn, d))
    d[17] = -1.0
    assert CR.r_maxstep(xn, d, 1.0) == oc.maxstep_rp(xn, d)
    assert np.isnan(CR.r_maxstep(xn, None, 1.0)) and np.isnan(oc.maxstep_rp(xn, None))
    assert CR.r_maxstep(x, None, 1.0) == oc.maxstep_rp(x, None) == 0.0


def _cholesky_step(x, d):
    """1 / lambda_max(L^-1 D L^-T), X = L L', in fp64 LAPACK: the formula the device evaluates, implemented apart"""
    import scipy.linalg as sl
    L = np.linalg.cholesky(oc.mat(x))
    T = sl.solve_triangular(L, sl.solve_triangular(L, oc.mat(d), lower=True).T, lower=True)
    mx = np.linalg.eigvalsh(0.5 * (T + T.T)).max()
    return np.inf if mx < 0 else 1.0 / mx


@pytest.mark.parametrize("r", [2, 7, 17, 48])
@pytest.mark.parametrize("span", [1e4, 1e8])
def test_oracle_meets_the_s_bounds(r, span):
    rng = np.random.default_rng(r + int(np.log10(span)))
    z, s = CR.s_point(r, span, rng), CR.s_point(r, span, rng)
    sv, b, _, _ = CR.s_nt(z, s)
    R = oc.nestod_sdc(z, s)
    Lam = np.diag(R.T @ oc.mat(z) @ R)
    assert np.all(np.abs(np.sort(Lam) - sv) <= b)
    Ri = np.linalg.inv(R)
    Rl, Ril = R.astype(CR.LD), Ri.astype(CR.LD)
    D = np.diag(Lam).astype(CR.LD)
    assert np.abs((Rl.T @ CR.mat(z, CR.LD) @ Rl - D).astype(np.float64)).max() <= 2 * b
    assert np.all(np.abs((Ril @ CR.mat(s, CR.LD) @ Ril.T - D).astype(np.float64)) <= CR.s_rinv_bound(Lam, b))
    x = rng.standard_normal(len(z))
    ref, bnd = CR.s_ftf(R, x)
    assert np.all(np.abs(oc.vecm(R @ (R.T @ oc.mat(x) @ R) @ R.T) - ref) <= bnd)
    for P, tr in ((R, False), (R, True)):
        ref, bnd = CR.s_congruence(P, x, tr)
        got = oc.vecm((P @ oc.mat(x) @ P.T) if tr else (P.T @ oc.mat(x) @ P))
        assert np.all(np.abs(got - ref) <= bnd)
    ref, bnd = CR.s_prod(x, z)
    assert np.all(np.abs(oc.xsdc(x, z) - ref) <= bnd)
    ref, bnd = CR.s_div_diag(x, sv)
    assert np.all(np.abs(oc.dsdc(x, oc.vecm(np.diag(sv))) - ref) <= bnd)
    res, bnd = CR.s_div_residual(x, z, oc.dsdc(x, z))
    assert res <= bnd
    d = rng.standard_normal(len(z))
    for scale in (1.0, 1.0 / 0.99):
        st = _cholesky_step(z, d * scale)
        M = CR.mat(z, CR.LD) - CR.LD(st) * CR.LD(scale) * CR.mat(d, CR.LD)
        assert CR.lambda_min_within(M, 0.0, CR.s_maxstep_bound(z, d, scale, st)), "Cholesky route"
        if span <= 1e4:
            # the oracle's own route goes through X^-1/2 (an eigendecomposition of X): a different formula, whose
            # error grows with cond(X) beyond the norm-wise bound of the Cholesky route at span 1e8
            st = oc.maxstep_sdc(z, d * scale)
            M = CR.mat(z, CR.LD) - CR.LD(st) * CR.LD(scale) * CR.mat(d, CR.LD)
            assert CR.lambda_min_within(M, 0.0, CR.s_maxstep_bound(z, d, scale, st)), "oracle route"


# ------------------------------------------------------------------------------------------ sampled rows and probes
def _ld_terms(P, x):
    Pl = np.asarray(P, dtype=np.float64).astype(CR.LD)
    return Pl, CR.mat(x, CR.LD)


@pytest.mark.parametrize("r", [20, 70])
def test_sampled_and_probe_forms_agree_with_the_full_forms(r):
    """The sampled and probe forms against (a) the same formula evaluated in full in extended precision, to 1e-17 of the
    magnitude product (the sums run in another order: r 2^-64 < 1e-17 of the magnitudes), and (b) the existing full forms,
    which return their value rounded to fp64 in vecm coordinates: to 3 u of the value on top (the rounding, and the sqrt2 of
    vecm taken out again by mat).  The bounds agree to the rounding of their fp64 magnitude products."""
    rng = np.random.default_rng(r)
    S, W = CR.sample_rows(r, r), CR.probe_vectors(r, r)
    assert {0, r - 1, 63 if r > 64 else r - 1}.issubset(S.tolist()) and (r <= 64 or 64 in S) and len(S) <= 2 * (-(-r // 64)) + 10
    assert W.shape == (r, 2) and np.all(np.abs(W) == 1) and not np.array_equal(W[:, 0], W[:, 1])
    z, s, x = CR.s_point(r, 1e8, rng), CR.s_point(r, 1e8, rng), rng.standard_normal(r * (r + 1) // 2)
    P = rng.standard_normal((r, r))
    Pl, X = _ld_terms(P, x)
    Z = CR.mat(z, CR.LD)
    Pa, Xa, Za = np.abs(P), np.abs(CR.mat(x)), np.abs(CR.mat(z))
    PP, PPa = Pl @ Pl.T, Pa @ Pa.T
    full = {
        "P'XP": (Pl.T @ X @ Pl, Pa.T @ Xa @ Pa, CR.s_congruence(P, x, False), CR.s_congruence_rows(P, x, False, S), CR.s_congruence_probe(P, x, False, W)),
        "PXP'": (Pl @ X @ Pl.T, Pa @ Xa @ Pa.T, CR.s_congruence(P, x, True), CR.s_congruence_rows(P, x, True, S), CR.s_congruence_probe(P, x, True, W)),
        "F'F": (PP @ X @ PP, PPa @ Xa @ PPa, CR.s_ftf(P, x), CR.s_ftf_rows(P, x, S), CR.s_ftf_probe(P, x, W)),
        "prod": (X @ Z + Z @ X, Xa @ Za + Za @ Xa, CR.s_prod(x, z), CR.s_prod_rows(x, z, S), CR.s_prod_probe(x, z, W)),
    }
    for name, (Y, mag, (ref64, bnd64), (rows, rbnd), (prb, pbnd)) in full.items():
        assert rows.dtype == CR.LD and prb.dtype == CR.LD, name
        assert np.all(np.abs(rows - Y[S]) <= 1e-17 * mag[S]), name
        assert np.all(np.abs(prb - Y @ W) <= 1e-17 * mag.sum(1)[:, None]), name
        assert np.all(np.abs(CR.mat(ref64)[S] - rows.astype(np.float64)) <= 3 * CR.U * np.abs(CR.mat(ref64)[S]) + 1e-17 * mag[S]), name
        B = CR.mat(bnd64)                                       # the entrywise bound in matrix form
        np.testing.assert_allclose(rbnd, B[S], rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(pbnd, B.sum(1), rtol=1e-12, err_msg=name)
    # the two NT identities, with the oracle's R
    R = oc.nestod_sdc(z, s)
    Ri = np.linalg.inv(R)
    lam = np.diag(R.T @ oc.mat(z) @ R).copy()
    b = CR.s_nt(z, s)[1]
    Rl, Ril = R.astype(CR.LD), Ri.astype(CR.LD)
    D = np.diag(lam).astype(CR.LD)
    for Y, mag, (rows, rbnd), (prb, pbnd), B in (
            (Rl.T @ Z @ Rl - D, np.abs(R).T @ Za @ np.abs(R) + np.diag(lam), CR.s_rzr_rows(R, z, lam, b, S), CR.s_rzr_probe(R, z, lam, b, W),
             np.full((r, r), 2 * b)),
            (Ril @ CR.mat(s, CR.LD) @ Ril.T - D, np.abs(Ri) @ np.abs(CR.mat(s)) @ np.abs(Ri).T + np.diag(lam), CR.s_risri_rows(Ri, s, lam, b, S),
             CR.s_risri_probe(Ri, s, lam, b, W), CR.s_rinv_bound(lam, b))):
        assert np.all(np.abs(rows - Y[S]) <= 1e-17 * mag[S])
        assert np.all(np.abs(prb - Y @ W) <= 1e-17 * mag.sum(1)[:, None])
        np.testing.assert_allclose(rbnd, B[S], rtol=1e-12)
        np.testing.assert_allclose(pbnd, B.sum(1), rtol=1e-12)
        assert np.all(np.abs(rows) <= rbnd) and np.all(np.abs(prb) <= pbnd[:, None])        # the oracle's R meets them
    # Lambda: the rotated Jacobi and LAPACK against svals_ld
    sv, b0, _, _ = CR.s_nt(z, s)
    svr, br, _, _, b1 = CR.s_nt_rotated(z, s)
    assert b1 == b0 and b0 <= br <= b0 * (1 + 1e-3) and np.all(np.abs(svr - sv) <= 4 * CR.U * sv.max())
    svf, bf, _, _, b2 = CR.s_nt_fp64(z, s)
    assert b2 == b0 and bf == 2 * b0 and np.all(np.abs(svf - sv) <= b0)
    # the certificate with its informational ratio
    M = np.diag(np.array([3.0, 1e-14, 5.0])).astype(CR.LD)
    ok, ratio = CR.lambda_min_certified(M, 1e-13)
    assert ok and abs(ratio - 0.1) < 1e-6
    assert not CR.lambda_min_certified(M, 1e-15)[0]


def _reject(got, rows, rbnd, prb, pbnd, S, W):
    """(rejected by the sampled rows, rejected by a probe) for a full output matrix `got`"""
    G = np.asarray(got).astype(CR.LD)
    return (bool(np.any(~(np.abs(G[S] - rows) <= rbnd))), bool(np.any(~(np.abs(CR._mm(G, W) - prb) <= pbnd[:, None]))))


def test_sampled_rows_and_probes_reject_wrong_outputs():
    """a congruence at order 300, span 1e8: what a tiled GEMM and the vecm store can get wrong is caught by the sampled rows
    or by the probes, and the exact result rounded to fp64 passes"""
    r = 300
    rng = np.random.default_rng(300)
    x = CR.s_point(r, 1e8, rng)
    P = rng.standard_normal((r, r))
    S, W = CR.sample_rows(r, 300), CR.probe_vectors(r, 300)
    rows, rbnd = CR.s_congruence_rows(P, x, False, S)
    prb, pbnd = CR.s_congruence_probe(P, x, False, W)
    Pl, X = _ld_terms(P, x)
    T = CR._mm(X, Pl)
    Y = CR._mm(Pl.T, T)
    Y = 0.5 * (Y + Y.T)
    good = Y.astype(np.float64)
    assert _reject(good, rows, rbnd, prb, pbnd, S, W) == (False, False)
    t1, t2, t3 = slice(64, 128), slice(128, 192), slice(192, 256)

    def both(M, I, J, tile):
        M = M.copy()
        M[I, J] = tile
        M[J, I] = tile.T
        return M
    free = np.setdiff1d(np.arange(r), S)
    i, j = free[5], free[40]                                   # neither row i nor row j is sampled
    entry = good.copy()
    entry[i, j] = entry[j, i] = good[i, j] * (1 + 1e-6)
    srow = good.copy()
    srow[S[3], 17] = srow[17, S[3]] = good[S[3], 17] * (1 + 1e-6)
    sqrt2 = good.copy()
    sqrt2[i, :] *= np.sqrt(2.0)
    sqrt2[:, i] = sqrt2[i, :]
    sqrt2[i, i] = good[i, i]
    wrong = {
        "tile transposed": both(good, t1, t2, good[t1, t2].T),
        "tile from its neighbour": both(good, t1, t2, good[t1, t3]),
        "k-slab of 32 dropped": both(good, t1, t2, (Y[t1, t2] - CR._mm(Pl[32:64, t1].T, T[32:64, t2])).astype(np.float64)),
        "entry of a sampled row off by 1e-6": srow,
        "entry elsewhere off by 1e-6": entry,
        "sqrt2 missing in a row": sqrt2,
    }
    for name, M in wrong.items():
        by_rows, by_probe = _reject(M, rows, rbnd, prb, pbnd, S, W)
        assert by_rows or by_probe, name
        if name.startswith(("tile", "k-slab", "entry of a sampled")):
            assert by_rows, name                               # two full rows cross every tile
        if name == "entry elsewhere off by 1e-6":
            assert by_probe and not by_rows, name              # neither its row nor its column is sampled: the probes alone
        if name == "sqrt2 missing in a row":
            assert by_probe and by_rows, name                  # the row by the probes, its mirror column by every sampled row
