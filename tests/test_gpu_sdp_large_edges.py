"""The large S-cone kernels (csrc/sdp_large.hip, sdp_large_nt.hip, sdp_large_eig.hip) above padded order 256 at hard iterates,
against the extended-precision references and error bounds of tests/_cone_ref.py.

tests/test_gpu_cone_edges.py stops at order 200, which is padded order rp = 256.  The large path has one form of
almost everything per rp in {256, 512, 1024, 2048}; the cases here reach the other three, the two tridiagonalisations
behind the max step above order 256 with the slab sizes of the cooperative one, the batched-64 GEMM path that replaces
k_gemm_nt_small above rp = 256, and a handle with two large cones of different order (the smaller one padded for its
neighbour, per-cone slots of different order).  test_case_table_reaches_the_named_paths holds the table against the
restatement of the dispatch rules in tests/_sdp_large_forms.py, which tests/test_sdp_large_forms.py holds against
csrc/cip_sdp_large_forms.h.

Iterates and device calls are those of test_s_cone_ops_at_the_edges: CR.s_point at spans 1e4 and 1e8 (1e8 only at
orders 1024 and 1025), set_scaling_from_iterate, get_scaling_packed, apply_F (four modes, in place), cone_prod, cone_div
by lambda, maxstep (both forms, scale 1 and 1 / 0.99) and maxstep_pair.  Every handle takes two scalings per span: the
second one is warm-started from the first (k_lg_ns, k_lg_warm_gate, the V-rebuild GEMM).

Checks.  Up to order 257 the full-matrix checks of test_s_cone_ops_at_the_edges.  Above, a full extended-precision
product is no longer affordable: the same quantities within the same entrywise bounds on the sampled rows of
CR.sample_rows (two full rows through every 64 x 64 tile) and, over the whole matrix, against two +-1 probe vectors
within the row sums of the entrywise bound.  Lambda: CR.s_nt at order 140; at orders 257 and 300 CR.s_nt_rotated, the
same extended-precision Jacobi from a rotated start (a cold svals_ld takes 8 to 15 s there, and a case runs four of
them), its bound b plus the 1e-17 the rotation can move a singular value by; LAPACK within 2 b above (CR.s_nt_fp64).
The max step is held to the certificate |lambda_min(X - alpha scale D)| <= bound by two extended-precision Choleskys per
verdict; |lambda_min| / bound from LAPACK is recorded for information only.

Left out: cone_div by a non-diagonal divisor.  Above order 132 it is one workgroup of k_sdp_div running a full
eigensolve; the interior-point loop never takes it (its divisor is lambda), and nobody has measured its run time at
order 1025.

Set SDP_LARGE_EDGE_RATIOS=<file> to have the largest error / bound ratio of each operation and case written there,
with the wall time of each case."""
import json
import os
import time

import numpy as np
import pytest

import _cone_ref as CR
from _sdp_large_forms import PATHS, _reach
from test_gpu_cone_edges import _bits_equal, _dev, _offsets, _sym_dir, _system

gpu = pytest.mark.gpu


def _s(r):
    return ("S", r * (r + 1) // 2)


# name -> cone_dims; the comment names what the row reaches
CASES = {
    # smallest rp = 512 with 255 padding rows; k_lg_jacobi<1024>; cooperative tridiagonalisation, slabs of 32; batched-64 GEMM
    "s257": [_s(257)],
    # r == rp: no padding
    "s512": [_s(512)],
    # smallest rp = 1024; k_lg_jacobi<512, 16>
    "s513": [_s(513)],
    # the last order whose 32-column slab fits the LDS budget of the cooperative form (lg_eig_form), and the first with 16 columns
    "s583": [_s(583)],
    "s584": [_s(584)],
    # the largest cooperative tridiagonalisation: 64 workgroups
    "s1024": [_s(1024)],
    # smallest rp = 2048; k_lg_jacobi<256, 32>; stepped tridiagonalisation
    "s1025": [_s(1025)],
    # order 140 inside rp = 512: Lanczos with its certificate at ldm = 512, no small-GEMM kernel, unpaired maxstep_pair; slots
    # li = 0, 1 of different order
    "mixed_140_300": [_s(140), ("R", 5), _s(300)],
}
SPANS = {name: [1e8] if name in ("s1024", "s1025") else [1e4, 1e8] for name in CASES}
FULL_MAX = 257                      # full-matrix checks up to here, sampled rows and probes above


def test_case_table_reaches_the_named_paths():
    for name, cone_dims in CASES.items():
        got = _reach(cone_dims)
        for key, want in PATHS[name].items():
            assert got[key] == want, (name, key, got[key])
    assert _reach(CASES["s257"])["padding"] == [255] and _reach(CASES["s512"])["padding"] == [0]
    # what test_gpu_cone_edges.py reaches: rp = 256 only
    assert _reach([_s(200)]) == {"rp": 256, "gemm": "small", "pairable": True, "jacobi": (256, 8, 8), "padding": [56],
                                 "maxstep": [("lanczos", 0, 1)]}


# ------------------------------------------------------------------------------------------ ratio bookkeeping
RATIOS = {}


def _record(case, op, err, bnd):
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    err, bnd = np.broadcast_arrays(err, bnd)
    bad = ~(err <= bnd)
    assert not bad.any(), "%s, %s: %d entries over the bound; worst err %r bound %r" % (
        case, op, int(bad.sum()), err[bad][:3].tolist(), bnd[bad][:3].tolist())
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd > 0, err / bnd, 0.0)
    _note(case, op, float(q.max()) if q.size else 0.0)
    print("%s %-34s %.3g" % (case, op, float(q.max()) if q.size else 0.0))


def _note(case, op, ratio):
    d = RATIOS.setdefault(case, {})
    d[op] = max(d.get(op, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("SDP_LARGE_EDGE_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------ the checks
def _compare(case, op, got, r, S, W, full, rows, probe):
    """a device vector `got` (vecm coordinates) against the full form up to FULL_MAX, sampled rows and probes above"""
    if r <= FULL_MAX:
        ref, bnd = full()
        _record(case, op, np.abs(got - ref), bnd)
        return
    G = CR.mat(got, CR.LD)
    ref, bnd = rows(S)
    _record(case, op + " (rows)", np.abs(G[S] - ref), bnd)
    ref, bnd = probe(W)
    _record(case, op + " (probes)", np.abs(CR._mm(G, W) - ref), bnd[:, None])


def _packed_offsets(cone_dims):
    so, out = 0, []
    for t, k in cone_dims:
        out.append(so)
        so += k if t == "R" else 2 * CR.order(k) ** 2
    return out


def _nt_reference(r, v, s):
    """(Lambda ascending, its bound, b)"""
    if r <= 200:                                                                  # the orders of test_gpu_cone_edges.py
        sv, b, _, _ = CR.s_nt(v, s)
        return sv, b, b
    sv, bnd, _, _, b = CR.s_nt_rotated(v, s) if r <= 300 else CR.s_nt_fp64(v, s)
    return sv, bnd, b


def _check_scaling(case, ks, cone_dims, v, s, x, seed):
    """one set_scaling_from_iterate and everything that depends on it, for every S cone of the handle"""
    from cipkkt import OP_F, OP_FINV, OP_FINVT, OP_FT
    m = len(v)
    lam_d = _dev(np.zeros(m))
    ks.set_scaling_from_iterate(_dev(v), _dev(s), lam_d)
    lam = lam_d.cpu().numpy()
    packed = ks.get_scaling_packed()
    dx = _dev(x)
    fx, ftfx = _dev(np.zeros(m)), _dev(np.zeros(m))
    ks.apply_F(OP_F, dx, fx)
    ks.apply_F(OP_FT, fx, ftfx)
    ftf = ftfx.cpu().numpy()
    applied = {}
    for mode in (OP_F, OP_FT, OP_FINV, OP_FINVT):
        out = _dev(np.zeros(m))
        ks.apply_F(mode, dx, out)
        applied[mode] = out.cpu().numpy()
        y = dx.clone()
        ks.apply_F(mode, y, y)
        assert _bits_equal(y.cpu().numpy(), applied[mode]), ("S apply in place", mode)
    out = _dev(np.zeros(m))
    ks.cone_div(dx, lam_d, out)
    div = out.cpu().numpy()
    for (t, k, o), so in zip(_offsets(cone_dims), _packed_offsets(cone_dims)):
        if t != "S":
            continue
        r = CR.order(k)
        sl = slice(o, o + k)
        vc, sc, xc = v[sl], s[sl], x[sl]
        S, W = CR.sample_rows(r, seed), CR.probe_vectors(r, seed)
        Lm = CR.mat(lam[sl])
        assert np.all(Lm[~np.eye(r, dtype=bool)] == 0.0), "lambda is diagonal"
        lamd = np.diag(Lm).copy()
        sv, bnd, b = _nt_reference(r, vc, sc)
        _record(case, "nt Lambda", np.abs(np.sort(lamd) - sv), bnd)
        R = packed[so:so + r * r].reshape(r, r, order="F")
        Ri = packed[so + r * r:so + 2 * r * r].reshape(r, r, order="F")
        if r <= FULL_MAX:
            Rl, Ril = R.astype(CR.LD), Ri.astype(CR.LD)
            D = np.diag(lamd).astype(CR.LD)
            _record(case, "nt R'ZR", np.abs(Rl.T @ CR.mat(vc, CR.LD) @ Rl - D), 2 * b)
            _record(case, "nt Ri S Ri'", np.abs(Ril @ CR.mat(sc, CR.LD) @ Ril.T - D), CR.s_rinv_bound(lamd, b))
        else:
            ref, bd = CR.s_rzr_rows(R, vc, lamd, b, S)
            _record(case, "nt R'ZR (rows)", np.abs(ref), bd)
            ref, bd = CR.s_rzr_probe(R, vc, lamd, b, W)
            _record(case, "nt R'ZR (probes)", np.abs(ref), bd[:, None])
            ref, bd = CR.s_risri_rows(Ri, sc, lamd, b, S)
            _record(case, "nt Ri S Ri' (rows)", np.abs(ref), bd)
            ref, bd = CR.s_risri_probe(Ri, sc, lamd, b, W)
            _record(case, "nt Ri S Ri' (probes)", np.abs(ref), bd[:, None])
        _compare(case, "F'F x", ftf[sl], r, S, W, lambda: CR.s_ftf(R, xc), lambda S: CR.s_ftf_rows(R, xc, S),
                 lambda W: CR.s_ftf_probe(R, xc, W))
        for mode, P, tr in ((OP_F, R, False), (OP_FT, R, True), (OP_FINV, Ri, False), (OP_FINVT, Ri, True)):
            _compare(case, "apply", applied[mode][sl], r, S, W, lambda: CR.s_congruence(P, xc, tr),
                     lambda S: CR.s_congruence_rows(P, xc, tr, S), lambda W: CR.s_congruence_probe(P, xc, tr, W))
        ref, bd = CR.s_div_diag(xc, lamd)
        _record(case, "div by lambda", np.abs(div[sl] - ref), bd)


def _inside(cone_dims, v, target):
    """a direction that never limits the step on the cones other than `target`: x - alpha d = (1 + alpha) x"""
    d = -v.copy()
    t, k, o = _offsets(cone_dims)[target]
    d[o:o + k] = 0.0
    return d


def _certify(case, op, M, bnd):
    ok, ratio = CR.lambda_min_certified(M, bnd)
    assert ok, "%s, %s: |lambda_min| is not within %g (LAPACK: %g of it)" % (case, op, bnd, ratio)
    _note(case, op + " (LAPACK, informational)", ratio)
    print("%s %-34s %.3g (LAPACK)" % (case, op, ratio))


def _check_maxstep(case, ks, cone_dims, target, v, s, rng):
    t, k, o = _offsets(cone_dims)[target]
    r = CR.order(k)
    sl = slice(o, o + k)
    vc = v[sl]
    X = CR.mat(vc, CR.LD)
    dv, ds = _dev(v), _dev(s)
    base = _inside(cone_dims, v, target)

    def full(dc):
        d = base.copy()
        d[sl] = dc
        return d
    d1 = _sym_dir(r, rng)
    for dc in (d1, d1 * 1e-4):
        for scale in (1.0, 1.0 / 0.99):
            got = ks.maxstep(dv, _dev(full(dc)), scale)
            assert np.isfinite(got) and got > 0, got
            M = X - CR.LD(got) * CR.LD(scale) * CR.mat(dc, CR.LD)
            _certify(case, "maxstep |lambda_min(X - alpha D)|", M, CR.s_maxstep_bound(vc, dc, scale, got))
            for kk in (1, -30):
                g2 = ks.maxstep(dv, _dev(full(dc * 2.0 ** kk)), scale) * 2.0 ** kk
                M = X - CR.LD(g2) * CR.LD(scale) * CR.mat(dc, CR.LD)
                assert CR.lambda_min_within(M, 0.0, CR.s_maxstep_bound(vc, dc, scale, g2)), ("S scaled", kk)
        dd = _dev(full(dc))
        assert _bits_equal(ks.maxstep_pair(dv, dd, ds, dd), (ks.maxstep(dv, dd), ks.maxstep(ds, dd)))
    assert ks.maxstep(dv, _dev(full(_sym_dir(r, rng, -1)))) == np.inf
    # the `nothing` form: 0 inside, -1 + lambda_min outside
    assert ks.maxstep(dv, None) == 0.0
    xo = v.copy()
    xo[sl] = vc - (np.linalg.eigvalsh(CR.mat(vc)).min() + 0.3) * CR.vecm(np.eye(r))      # lambda_min about -0.3
    got = ks.maxstep(_dev(xo), None)
    assert -1.5 < got < -1.1, got
    bnd = 8 * r * CR.U * CR.fro(CR.mat(xo[sl])) + 4 * CR.U
    _certify(case, "maxstep nothing", CR.mat(xo[sl], CR.LD) - CR.LD(got + 1.0) * np.eye(r, dtype=CR.LD), bnd)
    # a NaN in x (the reference's eigvals refuses a NaN matrix: there is no NaN to follow): the pair agrees with two calls
    xn = v.copy()
    xn[o + k // 2] = np.nan
    dn = _dev(full(_sym_dir(r, rng)))
    assert _bits_equal(ks.maxstep_pair(_dev(xn), dn, dv, dn), (ks.maxstep(_dev(xn), dn), ks.maxstep(dv, dn)))


def _point(cone_dims, span, rng):
    return np.concatenate([0.5 + rng.random(k) if t == "R" else CR.s_point(CR.order(k), span, rng) for t, k in cone_dims])


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_large_s_cone_ops_at_the_edges(name):
    import torch
    t0 = time.time()
    cone_dims = CASES[name]
    m = sum(k for _, k in cone_dims)
    ks = _system(cone_dims, 5)
    try:
        for span in SPANS[name]:
            seed = sum(map(ord, name)) * 31 + int(np.log10(span))
            rng = np.random.default_rng(seed)
            v, s = _point(cone_dims, span, rng), _point(cone_dims, span, rng)
            x = rng.standard_normal(m) * 10.0 ** rng.uniform(-2, 2, m)
            _check_scaling(name, ks, cone_dims, v, s, x, seed)
            # the second scaling of the handle starts its Jacobi from the first one's singular vectors
            v2, s2 = _point(cone_dims, span, rng), _point(cone_dims, span, rng)
            _check_scaling(name, ks, cone_dims, v2, s2, x, seed + 1)
            out = _dev(np.zeros(m))
            ks.cone_prod(_dev(x), _dev(v), out)
            prod = out.cpu().numpy()
            for target, (t, k, o) in enumerate(_offsets(cone_dims)):
                if t != "S":
                    continue
                r = CR.order(k)
                xc, vc = x[o:o + k], v[o:o + k]
                _compare(name, "prod", prod[o:o + k], r, CR.sample_rows(r, seed), CR.probe_vectors(r, seed),
                         lambda: CR.s_prod(xc, vc), lambda S: CR.s_prod_rows(xc, vc, S), lambda W: CR.s_prod_probe(xc, vc, W))
                _check_maxstep(name, ks, cone_dims, target, v, s, rng)
        torch.cuda.synchronize()
    finally:
        ks.close()
    _note(name, "seconds", time.time() - t0)
    print("%s %.1f s" % (name, time.time() - t0))
