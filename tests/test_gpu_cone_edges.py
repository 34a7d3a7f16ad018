"""The per-cone kernels (csrc/cones.hip, csrc/sdp.hip, csrc/sdp_large.hip) at hard iterates, on every kernel path,
against the high-precision references and error bounds of tests/_cone_ref.py.

Hard iterates are those of the last interior-point iterations: R entries over 1e-12 .. 1e12, Q points whose relative
gap (x0 - |x1|) / x0 is 1e-2, 1e-6 or 1e-10, S matrices with eigenvalues log-spaced over spans 1e4 and 1e8.  Every
operation goes through the public device calls: set_scaling_from_iterate, apply_F (four modes, in place), cone_prod,
cone_div, maxstep (both forms, scale 1 and 1 / 0.99) and maxstep_pair.  R cones are checked bit for bit, Q cones
entrywise within their running-error bounds, S cones by extended-precision certificates and norm-wise bounds.

Set CONE_EDGE_RATIOS=<file> to have the largest error / bound ratio of each operation written there."""
import json
import os

import mpmath as mp
import numpy as np
import pytest

import _cone_ref as CR

gpu = pytest.mark.gpu

# name -> cone_dims; the comment names the paths the row reaches (see test_case_table_reaches_the_named_paths)
CASES = {
    # R: one work item of 2000 entries
    "r_one_chunk": [("R", 2000)],
    # R: 5000 entries = items of 2048, 2048 and 904; the limiting entry moves over 0, 2047, 2048 and the last item
    "r_three_chunks": [("R", 5000)],
    # Q runs of dimension <= 64 split by R cones: pack widths 1, 2, 4, 8, 16, 32 and 64
    "q_pack_widths": [("Q", 1), ("R", 3), ("Q", 2), ("R", 3), ("Q", 3), ("Q", 4), ("R", 3), ("Q", 7), ("Q", 5), ("R", 3),
                      ("Q", 16), ("R", 3), ("Q", 17), ("Q", 30), ("R", 3), ("Q", 64), ("Q", 40)],
    # 70 x Q(8): width 8, 32 cones per workgroup, three items, the last one of 6
    "q_pack_8_x70": [("Q", 8)] * 70,
    # 300 x Q(1): width 1, 256 cones per workgroup, the last item of 44
    "q_pack_1_x300": [("Q", 1)] * 300,
    # dimension > 64: all 256 lanes (block reductions through LDS); 300 and 257 are above 256 and not multiples of it;
    # nine cones, so that v and s meet every pair of gaps
    "q_lanes_256": [("Q", 65), ("Q", 129), ("Q", 300), ("Q", 257), ("Q", 65), ("Q", 129), ("Q", 300), ("Q", 257), ("Q", 70)],
}
S_ORDERS = [2, 7, 17, 48, 49, 64, 100, 132, 133, 200]
S_SPANS = [1e4, 1e8]
GAPS = [1e-2, 1e-6, 1e-10]

PATHS = {
    "r_one_chunk": {"R items": [2000]},
    "r_three_chunks": {"R items": [2048, 2048, 904]},
    "q_pack_widths": {"Q pack widths": [1, 2, 4, 8, 16, 32, 64]},
    "q_pack_8_x70": {"Q pack widths": [8], "Q pack sizes": [32, 32, 6]},
    "q_pack_1_x300": {"Q pack widths": [1], "Q pack sizes": [256, 44]},
    "q_lanes_256": {"Q 256 lanes": [65, 129, 300, 257, 65, 129, 300, 257, 70]},
}


def _paths(cone_dims):
    """the work items of cip_create (api.hip): R chunks of 2048, runs of Q cones <= 64 packed at width W = next power
    of two of the run's largest cone (256 / W cones per workgroup), larger Q cones on 256 lanes"""
    out = {}
    c = 0
    while c < len(cone_dims):
        t, k = cone_dims[c]
        if t == "R":
            out.setdefault("R items", []).extend(min(2048, k - st) for st in range(0, k, 2048))
            c += 1
        elif t == "Q" and k <= 64:
            e = c
            while e < len(cone_dims) and cone_dims[e][0] == "Q" and cone_dims[e][1] <= 64:
                e += 1
            W = 1
            while W < max(kk for _, kk in cone_dims[c:e]):
                W *= 2
            out.setdefault("Q pack widths", []).append(W)
            out.setdefault("Q pack sizes", []).extend(min(256 // W, e - q) for q in range(c, e, 256 // W))
            c = e
        else:
            out.setdefault("Q 256 lanes", []).append(k)
            c += 1
    return out


def _s_path(r):
    """sdp.hip: one workgroup of 256 threads up to order 48, 1024 threads (matrix in LDS) up to 132; sdp_large.hip above"""
    return "small-256" if r <= 48 else "small-1024" if r <= 132 else "large"


def test_case_table_reaches_the_named_paths():
    for name, cone_dims in CASES.items():
        got = _paths(cone_dims)
        for key, want in PATHS[name].items():
            assert got[key] == want, (name, key, got[key])
    assert [_s_path(r) for r in S_ORDERS] == ["small-256"] * 4 + ["small-1024"] * 4 + ["large"] * 2


# ------------------------------------------------------------------------------------------ ratio bookkeeping
RATIOS = {}


def _record(op, err, bnd):
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    bad = ~(err <= bnd)
    assert not bad.any(), "%s: %d entries over the bound; worst err %r bound %r" % (
        op, int(bad.sum()), err[bad][:3].tolist(), bnd[bad][:3].tolist())
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / bnd, 0.0)
    RATIOS[op] = max(RATIOS.get(op, 0.0), float(r.max()) if r.size else 0.0)


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("CONE_EDGE_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _bits_equal(a, b):
    """identical bits (so +0.0 != -0.0), NaN matching NaN of any payload"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


# ------------------------------------------------------------------------------------------ device plumbing
def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")


def _system(cone_dims, seed):
    import cipkkt
    rng = np.random.default_rng(seed)
    m = sum(k for _, k in cone_dims)
    n = 4
    M = rng.standard_normal((n, n))
    return cipkkt.KKTSystem(M @ M.T + np.eye(n), rng.standard_normal((m, n)), None, cone_dims)


def _offsets(cone_dims):
    o, out = 0, []
    for t, k in cone_dims:
        out.append((t, k, o))
        o += k
    return out


def _iterates(cone_dims, rng):
    """R entries over 1e-12 .. 1e12; the i-th Q cone has v at gap GAPS[i % 3] and s at gap GAPS[(i // 3) % 3], so any
    nine consecutive Q cones meet every pair of gaps"""
    v, s = [], []
    qi = 0
    for t, k in cone_dims:
        if t == "R":
            v.append(10.0 ** rng.uniform(-12, 12, k))
            s.append(10.0 ** rng.uniform(-12, 12, k))
        else:
            v.append(CR.q_point(k, GAPS[qi % 3], rng))
            s.append(CR.q_point(k, GAPS[(qi // 3) % 3], rng))
            qi += 1
    return np.concatenate(v), np.concatenate(s)


def _identity(cone_dims):
    return np.concatenate([np.ones(k) if t == "R" else np.eye(1, k)[0] for t, k in cone_dims])


# ------------------------------------------------------------------------------------------ R and Q cones
def _check_scaling(cone_dims, v, s, packed, lam):
    so = 0
    for t, k, o in _offsets(cone_dims):
        if t == "R":
            d = np.sqrt(s[o:o + k] / v[o:o + k])
            assert _bits_equal(packed[so:so + k], d), "R scaling"
            assert _bits_equal(lam[o:o + k], d * v[o:o + k]), "R lambda"
            so += k
            continue
        beta, w, lm = CR.q_nt(v[o:o + k], s[o:o + k])
        _record("nt beta", abs(packed[so] - float(beta.v)), beta.bound())
        _record("nt w", np.abs(packed[so + 1:so + 1 + k] - CR.values(w)), CR.bounds(w))
        _record("nt lambda", np.abs(lam[o:o + k] - CR.values(lm)), CR.bounds(lm))
        so += 1 + k


def _check_apply(ks, cone_dims, packed, x):
    from cipkkt import OP_F, OP_FINV, OP_FINVT, OP_FT
    dx = _dev(x)
    for mode in (OP_F, OP_FT, OP_FINV, OP_FINVT):
        out = _dev(np.zeros_like(x))
        ks.apply_F(mode, dx, out)
        got = out.cpu().numpy()
        y = dx.clone()
        ks.apply_F(mode, y, y)
        assert _bits_equal(y.cpu().numpy(), got), "apply_F in place, mode %d" % mode
        inv = mode in (OP_FINV, OP_FINVT)
        so = 0
        for t, k, o in _offsets(cone_dims):
            if t == "R":
                d = packed[so:so + k]
                assert _bits_equal(got[o:o + k], x[o:o + k] / d if inv else x[o:o + k] * d), "R apply %d" % mode
                so += k
                continue
            ref = CR.q_apply(packed[so], packed[so + 1:so + 1 + k], x[o:o + k], inv)
            _record("apply F^-1" if inv else "apply F", np.abs(got[o:o + k] - CR.values(ref)), CR.bounds(ref))
            so += 1 + k


def _check_prod_div(ks, cone_dims, x, y):
    out = _dev(np.zeros_like(x))
    ks.cone_prod(_dev(x), _dev(y), out)
    prod = out.cpu().numpy()
    ks.cone_div(_dev(x), _dev(y), out)
    div = out.cpu().numpy()
    for t, k, o in _offsets(cone_dims):
        sl = slice(o, o + k)
        if t == "R":
            assert _bits_equal(prod[sl], x[sl] * y[sl]) and _bits_equal(div[sl], x[sl] / y[sl]), "R prod / div"
            continue
        p, q = CR.q_prod(x[sl], y[sl]), CR.q_div(x[sl], y[sl])
        _record("prod", np.abs(prod[sl] - CR.values(p)), CR.bounds(p))
        _record("div", np.abs(div[sl] - CR.values(q)), CR.bounds(q))


KINDS = ["one", "far", "never"]


def _check_q_step(xc, dc, scale, got):
    """one Q cone's step (all other cones have d = 0): the alpha it stands for within the bound of alpha; where that
    bound settles the sign, the step within its bound and x - step scale d on the boundary within the bound"""
    alpha = CR.q_maxstep(xc, dc, scale)
    for label, err, bnd in CR.q_step_errors(alpha, got):
        _record(label, float(err), float(bnd))
    st = CR.step_of(alpha)
    if st is not None and st[0] != mp.inf:
        dist, slope = CR.q_distance(xc, dc, scale, got)
        _record("maxstep Q distance", abs(dist), slope * st[1])


def _q_directions(cone_dims, v, rng):
    """the i-th Q cone crosses the boundary the KINDS[(i // 9) % 3] way (crossed with the nine gap pairs)"""
    d = np.zeros_like(v)
    qi = 0
    for t, k, o in _offsets(cone_dims):
        if t == "Q":
            d[o:o + k] = CR.q_direction(v[o:o + k], KINDS[(qi // 9) % 3], rng)
            qi += 1
        else:
            d[o:o + k] = rng.standard_normal(k) * 10.0 ** rng.uniform(-3, 3, k)
    return d


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rq_cone_ops_at_the_edges(name):
    import torch
    cone_dims = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    ks = _system(cone_dims, 1)
    try:
        m = ks.m
        v, s = _iterates(cone_dims, rng)
        lam_d = _dev(np.zeros(m))
        ks.set_scaling_from_iterate(_dev(v), _dev(s), lam_d)
        packed, lam = ks.get_scaling_packed(), lam_d.cpu().numpy()
        _check_scaling(cone_dims, v, s, packed, lam)
        x = rng.standard_normal(m) * 10.0 ** rng.uniform(-4, 4, m)
        _check_apply(ks, cone_dims, packed, x)
        _check_prod_div(ks, cone_dims, x, v)
        _check_prod_div(ks, cone_dims, x, lam)            # the loop's divisor
        torch.cuda.synchronize()
    finally:
        ks.close()


def _r_direction(x, lim, rng):
    """d with random signs whose smallest ratio x_i / d_i (d_i > 0) sits at index lim"""
    d = rng.standard_normal(len(x)) * 10.0 ** rng.uniform(-6, 6, len(x))
    ratio = np.where(d > 0, x / np.where(d > 0, d, 1.0), np.inf)
    rmin = ratio.min()
    d[lim] = x[lim] / (rmin * 0.5)
    return d


@gpu
@pytest.mark.parametrize("name", ["r_one_chunk", "r_three_chunks"])
def test_r_maxstep_bit_for_bit(name):
    cone_dims = CASES[name]
    k = cone_dims[0][1]
    rng = np.random.default_rng(7 + k)
    ks = _system(cone_dims, 2)
    try:
        x = 10.0 ** rng.uniform(-12, 12, k)
        lims = [0, k - 1] if k <= 2048 else [0, 2047, 2048, 4096 + 500, k - 1]
        dirs = [_r_direction(x, lim, rng) for lim in lims] + [-np.abs(rng.standard_normal(k))]
        for d in dirs:
            for scale in (1.0, 1.0 / 0.99):
                got = ks.maxstep(_dev(x), _dev(d), scale)
                ref = CR.r_maxstep(x, d, scale)
                assert _bits_equal(got, ref), (got, ref)
                if np.isfinite(got):
                    dist, b = CR.r_distance_bound(x, d, scale, got)
                    _record("maxstep R distance", abs(float(dist)), b)
                for kk in (1, -1, 30, -30):
                    assert _bits_equal(ks.maxstep(_dev(x), _dev(d * 2.0 ** kk), scale), got * 2.0 ** -kk), kk
            assert _bits_equal(ks.maxstep_pair(_dev(x), _dev(d), _dev(x), _dev(-d)),
                               (ks.maxstep(_dev(x), _dev(d)), ks.maxstep(_dev(x), _dev(-d))))
        assert ks.maxstep(_dev(x), None) == 0.0
        xo = x.copy()
        xo[lims[-1]] = -3.5
        assert _bits_equal(ks.maxstep(_dev(xo), None), CR.r_maxstep(xo, None, 1.0))
    finally:
        ks.close()


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("q_")])
def test_q_maxstep_at_the_edges(name):
    cone_dims = CASES[name]
    rng = np.random.default_rng(11 + sum(map(ord, name)))
    ks = _system(cone_dims, 3)
    try:
        v, _ = _iterates(cone_dims, rng)
        d = _q_directions(cone_dims, v, rng)
        dv = _dev(v)
        # every Q cone (every gap of v) with every kind of direction, alone (d = 0 on the other cones)
        for t, k, o in _offsets(cone_dims):
            if t != "Q":
                continue
            for kind in KINDS:
                dc = np.zeros_like(d)
                dc[o:o + k] = CR.q_direction(v[o:o + k], kind, rng)
                for scale in (1.0, 1.0 / 0.99):
                    got = ks.maxstep(dv, _dev(dc), scale)
                    _check_q_step(v[o:o + k], dc[o:o + k], scale, got)
                    for kk in (1, -1, 30, -30):
                        assert _bits_equal(ks.maxstep(dv, _dev(dc * 2.0 ** kk), scale), got * 2.0 ** -kk), (o, kind, kk)
        for scale in (1.0, 1.0 / 0.99):
            got = ks.maxstep(dv, _dev(d), scale)
            assert _bits_equal(ks.maxstep_pair(dv, _dev(d), dv, _dev(-d), scale),
                               (got, ks.maxstep(dv, _dev(-d), scale)))
        # the `nothing` form: 0 inside; -1 - (|x1| - x0) for one cone moved outside, everything else at the identity
        assert ks.maxstep(dv, None) == 0.0
        e = _identity(cone_dims)
        for t, k, o in _offsets(cone_dims):
            if t != "Q" or k == 1:
                continue
            xo = e.copy()
            xo[o:o + k] = v[o:o + k]
            xo[o] = v[o] * (1 - 1e-6) - np.linalg.norm(v[o + 1:o + k]) * 0.5
            a = CR.q_maxstep_none(xo[o:o + k])
            got = ks.maxstep(_dev(xo), None)
            _record("maxstep Q nothing", abs(mp.mpf(got) - (-1 - a.v)), a.bound() + 2 * CR.U * abs(got))
    finally:
        ks.close()


@gpu
@pytest.mark.parametrize("name", ["r_three_chunks", "q_pack_widths", "q_pack_8_x70", "q_lanes_256"])
def test_maxstep_nan_follows_the_reference(name):
    """Julia's min / minimum propagate NaN: a NaN in x reaches the step wherever the reference evaluates it"""
    cone_dims = CASES[name]
    rng = np.random.default_rng(5)
    ks = _system(cone_dims, 4)
    try:
        v, _ = _iterates(cone_dims, rng)
        d = _q_directions(cone_dims, v, rng)
        for t, k, o in _offsets(cone_dims):
            for pos in sorted({o, o + k - 1}):
                x = v.copy()
                x[pos] = np.nan
                dx = _dev(x)
                dd = d.copy()
                if t == "R":
                    dd[pos] = abs(dd[pos]) + 1.0                    # d > 0 here: the reference divides the NaN
                    only = np.zeros_like(d)
                    only[pos] = -1.0                                # d <= 0: the reference skips the entry
                    assert ks.maxstep(dx, _dev(only)) == np.inf, ("R skipped", pos)
                assert np.isnan(ks.maxstep(dx, _dev(dd))), (t, pos)
                assert np.isnan(ks.maxstep(dx, None)), (t, pos)
                p = ks.maxstep_pair(dx, _dev(dd), _dev(v), _dev(dd))
                assert np.isnan(p[0]) and not np.isnan(p[1]), (t, pos, p)
                p = ks.maxstep_pair(_dev(v), _dev(dd), dx, _dev(dd))
                assert not np.isnan(p[0]) and np.isnan(p[1]), (t, pos, p)
    finally:
        ks.close()


# ------------------------------------------------------------------------------------------ S cones
def _sym_dir(r, rng, sign=0):
    M = rng.standard_normal((r, r))
    M = 0.5 * (M + M.T)
    if sign:
        M = sign * (M @ M.T + np.eye(r))
    return CR.vecm(M)


@gpu
@pytest.mark.parametrize("r", S_ORDERS)
def test_s_cone_ops_at_the_edges(r):
    import torch
    from cipkkt import OP_F, OP_FINV, OP_FINVT, OP_FT
    k = r * (r + 1) // 2
    cone_dims = [("S", k)]
    ks = _system(cone_dims, 5)
    try:
        for span in S_SPANS:
            rng = np.random.default_rng(r * 31 + int(np.log10(span)))
            v, s = CR.s_point(r, span, rng), CR.s_point(r, span, rng)
            lam_d = _dev(np.zeros(k))
            ks.set_scaling_from_iterate(_dev(v), _dev(s), lam_d)
            lam = lam_d.cpu().numpy()
            Lm = CR.mat(lam)
            assert np.all(Lm[~np.eye(r, dtype=bool)] == 0.0), "lambda is diagonal"
            Lam = np.sort(np.diag(Lm))
            sv, b, Lz, Ls = CR.s_nt(v, s)
            _record("S nt Lambda", np.abs(Lam - sv), np.full(r, b))
            packed = ks.get_scaling_packed()
            R = packed[:r * r].reshape(r, r, order="F")
            Ri = packed[r * r:].reshape(r, r, order="F")
            Rl, Ril = R.astype(CR.LD), Ri.astype(CR.LD)
            D = np.diag(np.diag(Lm)).astype(CR.LD)
            _record("S nt R'ZR", np.abs((Rl.T @ CR.mat(v, CR.LD) @ Rl - D).astype(np.float64)).max(), 2 * b)
            _record("S nt Ri S Ri'", np.abs((Ril @ CR.mat(s, CR.LD) @ Ril.T - D).astype(np.float64)),
                    CR.s_rinv_bound(np.diag(Lm), b))
            x = rng.standard_normal(k) * 10.0 ** rng.uniform(-2, 2, k)
            dx = _dev(x)
            # the F'F x invariant: F' (F x) = vecm(P X P), P = R R'
            fx, ftfx = _dev(np.zeros(k)), _dev(np.zeros(k))
            ks.apply_F(OP_F, dx, fx)
            ks.apply_F(OP_FT, fx, ftfx)
            ref, bnd = CR.s_ftf(R, x)
            _record("S F'F x", np.abs(ftfx.cpu().numpy() - ref), bnd)
            for mode, P, tr in ((OP_F, R, False), (OP_FT, R, True), (OP_FINV, Ri, False), (OP_FINVT, Ri, True)):
                out = _dev(np.zeros(k))
                ks.apply_F(mode, dx, out)
                got = out.cpu().numpy()
                y = dx.clone()
                ks.apply_F(mode, y, y)
                assert _bits_equal(y.cpu().numpy(), got), ("S apply in place", mode)
                ref, bnd = CR.s_congruence(P, x, tr)
                _record("S apply", np.abs(got - ref), bnd)
            out = _dev(np.zeros(k))
            ks.cone_prod(dx, _dev(v), out)
            ref, bnd = CR.s_prod(x, v)
            _record("S prod", np.abs(out.cpu().numpy() - ref), bnd)
            ks.cone_div(dx, lam_d, out)
            ref, bnd = CR.s_div_diag(x, np.diag(Lm))
            _record("S div by lambda", np.abs(out.cpu().numpy() - ref), bnd)
            ks.cone_div(dx, _dev(v), out)
            res, bnd = CR.s_div_residual(x, v, out.cpu().numpy())
            _record("S div general", res, bnd)
            # max step: lambda_min(X - alpha scale D) = 0 within the bound
            X = CR.mat(v, CR.LD)
            for d in (_sym_dir(r, rng), _sym_dir(r, rng) * 1e-4):
                for scale in (1.0, 1.0 / 0.99):
                    got = ks.maxstep(_dev(v), _dev(d), scale)
                    assert np.isfinite(got) and got > 0, got
                    bnd = CR.s_maxstep_bound(v, d, scale, got)
                    M = X - CR.LD(got) * CR.LD(scale) * CR.mat(d, CR.LD)
                    _record("S maxstep |lambda_min(X - alpha D)|", CR.lambda_min_ratio(M, bnd), 1.0)
                    for kk in (1, -30):
                        g2 = ks.maxstep(_dev(v), _dev(d * 2.0 ** kk), scale) * 2.0 ** kk
                        M = X - CR.LD(g2) * CR.LD(scale) * CR.mat(d, CR.LD)
                        assert CR.lambda_min_within(M, 0.0, CR.s_maxstep_bound(v, d, scale, g2)), ("S scaled", kk)
                assert _bits_equal(ks.maxstep_pair(_dev(v), _dev(d), _dev(s), _dev(d)),
                                   (ks.maxstep(_dev(v), _dev(d)), ks.maxstep(_dev(s), _dev(d))))
            assert ks.maxstep(_dev(v), _dev(_sym_dir(r, rng, -1))) == np.inf
            # the `nothing` form: 0 inside, -1 + lambda_min outside
            assert ks.maxstep(_dev(v), None) == 0.0
            xo = v - (np.linalg.eigvalsh(CR.mat(v)).min() + 0.3) * CR.vecm(np.eye(r))      # lambda_min about -0.3
            got = ks.maxstep(_dev(xo), None)
            assert -1.5 < got < -1.1, got
            bnd = 8 * r * CR.U * CR.fro(CR.mat(xo)) + 4 * CR.U
            _record("S maxstep nothing", CR.lambda_min_ratio(CR.mat(xo, CR.LD) - CR.LD(got + 1.0) * np.eye(r, dtype=CR.LD), bnd), 1.0)
            # NaN: the reference's eigvals refuses a NaN matrix (an error, not a NaN), so there is no NaN to follow on an S
            # cone; the pair still agrees with two single calls
            xn = v.copy()
            xn[k // 2] = np.nan
            dn = _sym_dir(r, rng)
            assert _bits_equal(ks.maxstep_pair(_dev(xn), _dev(dn), _dev(v), _dev(dn)),
                               (ks.maxstep(_dev(xn), _dev(dn)), ks.maxstep(_dev(v), _dev(dn))))
        torch.cuda.synchronize()
    finally:
        ks.close()


# ------------------------------------------------------------------------------------------ a small S cone beside a large one
def _small_cone_beside(r, r_large):
    """every output of the order-r cone's block from a handle [S(r)] or [S(r), S(r_large)]; the large cone sits at the
    identity and takes no part in either max-step (zero direction; the identity is inside the cone)"""
    from cipkkt import OP_F, OP_FINV, OP_FINVT, OP_FT
    k = r * (r + 1) // 2
    orders = [r] + ([r_large] if r_large else [])
    cone_dims = [("S", q * (q + 1) // 2) for q in orders]
    rest = [CR.vecm(np.eye(q)) for q in orders[1:]]
    zero = [np.zeros(kk) for _, kk in cone_dims[1:]]
    rng = np.random.default_rng(132)
    v, s = CR.s_point(r, 1e4, rng), CR.s_point(r, 1e4, rng)
    x, d = rng.standard_normal(k), _sym_dir(r, rng)
    xo = v - (np.linalg.eigvalsh(CR.mat(v)).min() + 0.3) * CR.vecm(np.eye(r))          # lambda_min about -0.3
    ks = _system(cone_dims, 6)
    try:
        m = ks.m
        lam_d = _dev(np.zeros(m))
        ks.set_scaling_from_iterate(_dev(np.concatenate([v] + rest)), _dev(np.concatenate([s] + rest)), lam_d)
        got = {"packed": ks.get_scaling_packed()[:2 * r * r], "lambda": lam_d.cpu().numpy()[:k]}
        out = _dev(np.zeros(m))
        for mode in (OP_F, OP_FT, OP_FINV, OP_FINVT):
            ks.apply_F(mode, _dev(np.concatenate([x] + zero)), out)
            got["apply %d" % mode] = out.cpu().numpy()[:k]
        dv = _dev(np.concatenate([v] + rest))
        for scale in (1.0, 1.0 / 0.99):
            got["maxstep(v, d) scale %r" % scale] = ks.maxstep(dv, _dev(np.concatenate([d] + zero)), scale)
        got["maxstep(x, nothing)"] = ks.maxstep(_dev(np.concatenate([xo] + rest)), None)
    finally:
        ks.close()
    assert 0 < got["maxstep(v, d) scale 1.0"] < np.inf and -1.5 < got["maxstep(x, nothing)"] < -1.1, got
    return got


@gpu
def test_small_s_cone_gives_the_same_bits_beside_a_large_one():
    """The workgroup-per-cone kernels of sdp.hip keep the one live matrix of a small cone in LDS.  An LDS budget sized
    from the handle's largest S cone would push the max-step of an order-132 cone out of LDS beside a cone of order
    >= 432 (r (r + 1) > 19280 - 4 rmax) and not beside one of order 431: its block of the packed scaling, its lambda,
    apply_F and both forms of maxstep must come out bit for bit as from a handle that holds the small cone alone."""
    alone = _small_cone_beside(132, 0)
    for r_large in (431, 432):
        beside = _small_cone_beside(132, r_large)
        assert list(beside) == list(alone)
        for key in alone:
            assert _bits_equal(beside[key], alone[key]), (r_large, key)
