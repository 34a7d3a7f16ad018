"""The layer that joins the primitives into a Newton step -- solve3x3_once, solve3x3_chunk, cip_solve2x2_dev, cip_solve4x4_dev
(conicip.jl_amd/csrc/solve.hip) and the fused k_s4_pre_r / k_s4_post_r (csrc/vecops.hip there) -- at late-iteration scalings (F over ten decades, Q
iterates with gaps down to 1e-10, S iterates with spans up to 1e8), judged STAGE BY STAGE in extended precision at the device's
own upstream outputs: the packed scaling read back with get_scaling_packed, the factor read back with kkt_matrix() after
factor().  Stages, bounds, the case table and the end-to-end record are those of tests/_newton_ref.py (checked on the CPU by
tests/test_newton_ref.py); the factor and the assembly keep their own suites and are not judged again here.

Then the path identities, bit for bit: the generic solve4x4 against the sequence of public calls it is written as (also on a
regularised handle), an in-place or partially overlapping dz against the unfused result, and the fused branch falling through
to the refined generic path when the resolve inside it switches the regularisation on.  (That the refined path is reached
is asserted where it is reached: the two tests that run it check the handle's reg_rel > 0 at the solve.  That the case table
reaches the paths it names needs no GPU: tests/test_newton_ref.py::test_case_table_reaches_the_named_paths.)  (Fused against unfused on the hard
all-R iterates: tests/test_gpu_kernels.py::test_solve4x4_fused_r_path_bitwise_on_hard_iterates.)

Set NEWTON_RATIOS=<file> to have every error / bound ratio and the end-to-end figures written there."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _ldlt_ref as LR
import _newton_ref as NR

pytestmark = pytest.mark.gpu

RATIOS = {}


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("NEWTON_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


class Live:
    """a case of the table on the device: the handle, scaled at the case's iterate and factored, with what the stage checks
    read back from it"""

    def __init__(self, name):
        import cipkkt
        self.P = P = NR.make_problem(name)
        self.ks = ks = cipkkt.KKTSystem(P.Q, P.A, P.G, P.cone_dims, route=P.route)
        assert (ks.N, ks.Npad) == (P.N, P.Npad)
        self.lam = _dev(np.zeros(P.m))
        if P.m:
            ks.set_scaling_from_iterate(_dev(P.v), _dev(P.s), self.lam)
        ks.factor()
        assert ks.health()["n_regularized"] == 0, "the case must not need the regularised factorisation"
        self.fac = np.tril(ks.kkt_matrix())
        self.cones = NR.Cones(P.cone_dims, ks.get_scaling_packed())
        self.lam_h = self.lam.cpu().numpy()
        self.Bs = LR.dispatch(P.Npad, 3, 0, 1024, 0)[1]
        self.sb = LR.SolveBound(self.fac, self.Bs)

    def solve4x4(self, r):
        dz = torch.full((self.P.n + self.P.p + 2 * self.P.m,), float("nan"), dtype=torch.float64, device="cuda")
        self.ks.solve4x4_dev(self.lam, _dev(r), dz)
        torch.cuda.synchronize()
        return dz.cpu().numpy()


@pytest.fixture(scope="module")
def live():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Live(name)
        return made[name]

    yield get
    for lv in made.values():
        lv.ks.close()


def _record(tag, checks):
    for st, c in checks.items():
        RATIOS["%s | %s" % (tag, st)] = c["ratio"]
        print("NEWTON | %s | %s | %.3g x bound" % (tag, st, c["ratio"]))
    bad = {st: c["ratio"] for st, c in checks.items() if not c["ok"]}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("name", list(NR.CASES))
def test_newton_step_stage_by_stage(live, name):
    lv = live(name)
    P, ks, cones, sb = lv.P, lv.ks, lv.cones, lv.sb
    c_s = LR.C_S["gemv"]
    has_oracle = NR.CASES[name].get("oracle", True)
    if has_oracle:
        margin, worst, _ = NR.case_margin(P)                     # on the host, from the fp64 model: never from the device
        RATIOS["%s | end to end, margin" % name] = margin
    for kind, draw, r in NR.rhs_table(P):
        if draw:
            continue
        dz = lv.solve4x4(r)
        _record("%s %s solve4x4" % (name, kind), NR.check_4x4(P, cones, sb, c_s, lv.lam_h, r, dz))
        e2e = NR.end_to_end(P, cones, lv.lam_h, r, dz)
        RATIOS["%s | %s | end to end" % (name, kind)] = list(e2e)
        if has_oracle:
            orc = NR.end_to_end(P, cones, lv.lam_h, r, NR.oracle_4x4(P, cones, lv.lam_h, r))
            RATIOS["%s | %s | end to end, oracle" % (name, kind)] = list(orc)
            ratio = NR.e2e_ratio(e2e, orc)
            print("NEWTON | %s %s | end to end %s | oracle %s | worst ratio %.3g | margin %.3g (model %.3g)" % (
                name, kind, np.array2string(e2e, precision=2), np.array2string(orc, precision=2), ratio, margin, worst))
            assert ratio <= margin, (name, kind, e2e, orc, ratio, margin)
        else:
            print("NEWTON | %s %s | end to end %s" % (name, kind, np.array2string(e2e, precision=2)))
    rng = np.random.default_rng(5)
    x, y, z = rng.standard_normal(P.n), rng.standard_normal(P.p), rng.standard_normal(P.m) * 10.0 ** rng.uniform(-8.0, 0.0, P.m)
    a, b, c = ks.solve3x3(x, y, z)
    _record("%s solve3x3" % name, NR.check_3x3(P, cones, sb, c_s, x, y, z if P.m else None, a, b, c))
    if P.route == "schur":
        dy, dw = ks.solve2x2(x, y)
        _record("%s solve2x2" % name, NR.check_3x3(P, cones, sb, c_s, x, y, None, dy, dw, None))


@pytest.mark.parametrize("name,nrhs", [(n, k) for n, ks_ in NR.MANY.items() for k in ks_])
def test_many_columns_stage_by_stage(live, name, nrhs):
    """solve3x3_many_dev with C aliasing Z: every column through the 3x3 stages (64 columns a chunk: 3, 64 and 65 columns are a
    short chunk, a full one, and a full one with a one-column chunk behind it); solve2x2_many_dev at 65 columns"""
    lv = live(name)
    P, ks = lv.P, lv.ks
    rng = np.random.default_rng(nrhs)
    X, Y = rng.standard_normal((nrhs, P.n)), rng.standard_normal((nrhs, P.p))
    Z = rng.standard_normal((nrhs, P.m)) * 10.0 ** rng.uniform(-8.0, 0.0, (nrhs, 1))
    Zd = _dev(Z)
    A, B = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((nrhs, P.n), (nrhs, P.p)))
    ks.solve3x3_many_dev(_dev(X), _dev(Y), Zd, A, B, Zd)
    torch.cuda.synchronize()
    Ah, Bh, Ch = A.cpu().numpy(), B.cpu().numpy(), Zd.cpu().numpy()
    worst = {}
    for j in range(nrhs):
        checks = NR.check_3x3(P, lv.cones, lv.sb, LR.C_S["many" if nrhs > 1 else "gemv"], X[j], Y[j], Z[j], Ah[j], Bh[j], Ch[j])
        for st, c in checks.items():
            assert c["ok"], (name, nrhs, j, st, c["ratio"])
            worst[st] = max(worst.get(st, 0.0), c["ratio"])
    for st, v in worst.items():
        RATIOS["%s many %d | %s" % (name, nrhs, st)] = v
    if nrhs == NR.MANY_CHUNK + 1:
        DY, DW = (torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((nrhs, P.n), (nrhs, P.p)))
        ks.solve2x2_many_dev(_dev(X), _dev(Y), DY, DW)
        torch.cuda.synchronize()
        DYh, DWh = DY.cpu().numpy(), DW.cpu().numpy()
        w2 = 0.0
        for j in range(nrhs):
            c = NR.check_3x3(P, lv.cones, lv.sb, LR.C_S["many"], X[j], Y[j], None, DYh[j], DWh[j], None)["rhs+sweeps"]
            assert c["ok"], (name, "2x2", j, c["ratio"])
            w2 = max(w2, c["ratio"])
        RATIOS["%s many %d 2x2 | rhs+sweeps" % (name, nrhs)] = w2


# ------------------------------------------------------------------------------------------------------- path identities
def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _public_sequence(ks, P, lam, r):
    """cip_solve4x4_dev's generic path as the public calls it is written as (solve.hip): cone_div, F' in place, two axpby,
    solve3x3_dev with c aliasing z, F, F', axpby"""
    from cipkkt import OP_F, OP_FT
    n, p, m = P.n, P.p, P.m
    dz = torch.full((n + p + 2 * m,), float("nan"), dtype=torch.float64, device="cuda")
    ry, rw, rv, rs = r[:n], r[n:n + p], r[n + p:n + p + m], r[n + p + m:]
    dy, dw, dv, ds = dz[:n], dz[n:n + p], dz[n + p:n + p + m], dz[n + p + m:]
    u = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    ks.cone_div(rs, lam, ds)
    ks.apply_F(OP_FT, ds, ds)
    ks.axpby(1.0, rv, 0.0, dv)
    ks.axpby(1.0, ds, 1.0, dv)
    ks.solve3x3_dev(ry, rw, dv, dy, dw, dv)
    ks.apply_F(OP_F, dv, u)
    ks.apply_F(OP_FT, u, u)
    ks.axpby(-1.0, u, 1.0, ds)
    torch.cuda.synchronize()
    return dz.cpu().numpy()


@pytest.mark.parametrize("rel", [0.0, 1e-10], ids=["plain", "regularised"])
@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_generic_solve4x4_is_its_sequence_of_public_calls(route, rel):
    """R, Q and S cones (orders 7 and 3), both routes, plain and on a regularised handle (the refined path: reg_rel > 0 is asserted);
    then the same call in place and with dz overlapping the end of r"""
    import cipkkt
    cone_dims = [("R", 9), ("Q", 8), ("S", 28), ("Q", 65), ("R", 4), ("S", 6)]
    P = NR.make_problem("generic", dict(n=40, p=3, cones=cone_dims, route=route, csr=route == "schur", mu=1e-6))
    ks = cipkkt.KKTSystem(P.Q, P.A, P.G, P.cone_dims, route=route)
    try:
        if rel:
            assert ks.lib.cip_set_regularization(ks.h, C.c_double(rel), 0) == 0
        lam = _dev(np.zeros(P.m))
        ks.set_scaling_from_iterate(_dev(P.v), _dev(P.s), lam)
        ks.factor()
        assert ks.health()["reg_rel"] == rel
        for kind in ("normal", "graded"):
            r = _dev(NR.rhs4(P, kind, np.random.default_rng(3)))
            dz = torch.full_like(r, float("nan"))
            ks.solve4x4_dev(lam, r, dz)
            torch.cuda.synchronize()
            got = dz.cpu().numpy()
            assert np.isfinite(got).all()
            assert _bits(got, _public_sequence(ks, P, lam, r)), (route, rel, kind)
            # include/cipkkt.h: dz may be r itself, and may start behind r.v -- with Q and small S cones (their kernels stage a
            # cone before they write it) and on the refined path (it copies x, y, z before it refines) as well
            rr = r.clone()
            ks.solve4x4_dev(lam, rr, rr)
            k, len4 = 5, r.numel()
            buf = torch.full((2 * len4 - k,), float("nan"), dtype=torch.float64, device="cuda")
            buf[:len4] = r
            ks.solve4x4_dev(lam, buf[:len4], buf[len4 - k:])
            torch.cuda.synchronize()
            assert _bits(rr.cpu().numpy(), got) and _bits(buf[len4 - k:].cpu().numpy(), got), (route, rel, kind)
    finally:
        ks.close()


@pytest.mark.parametrize("rel", [0.0, 1e-10], ids=["plain", "regularised"])
@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_host_pointer_entry_points_return_their_device_twins_bits(route, rel):
    """cip_solve3x3, cip_solve2x2 (Schur route) and the host cip_solve3x3_many / cip_solve2x2_many at 1 and 65 columns stage their
    blocks through the handle and call the device entry point: exactly (torch.equal) what the _dev twin writes for the same inputs
    on the same factor.  n = 96, p = 8, R(16) + Q(5) + S(3x3): every block of the right-hand side, Npad = 128 (Schur) or 256 (full
    3x3), and a second 64-column chunk; on a plain factor and on a regularised one (the refined solves, column by column)."""
    import cipkkt
    P = NR.make_problem("hostdev", dict(n=96, p=8, cones=[("R", 16), ("Q", 5), ("S", 6)], route=route, csr=False, mu=1e-2))
    n, p, m = P.n, P.p, P.m
    ks = cipkkt.KKTSystem(P.Q, P.A, P.G, P.cone_dims, route=route)
    try:
        assert ks.Npad == (128 if route == "schur" else 256)
        if rel:
            assert ks.lib.cip_set_regularization(ks.h, C.c_double(rel), 0) == 0
        ks.set_scaling_from_iterate(_dev(P.v), _dev(P.s), _dev(np.zeros(m)))
        ks.factor()
        assert ks.health() == dict(reg_rel=rel, n_regularized=0, n_chain_fallbacks=0)
        rng = np.random.default_rng(17)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        same = lambda host, dev: torch.equal(torch.from_numpy(np.ascontiguousarray(host.T)), dev.cpu())    # (rows, k) against (k, rows)

        x, y, z = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
        a, b, c = nan(n), nan(p), nan(m)
        ks.solve3x3_dev(_dev(x), _dev(y), _dev(z), a, b, c)
        assert all(same(h_, d_) for h_, d_ in zip(ks.solve3x3(x, y, z), (a, b, c))), "solve3x3"
        if route == "schur":
            dy, dw = nan(n), nan(p)
            ks.solve2x2_dev(_dev(x), _dev(y), dy, dw)
            assert all(same(h_, d_) for h_, d_ in zip(ks.solve2x2(x, y), (dy, dw))), "solve2x2"
        for k in (1, 65):
            X, Y, Z = rng.standard_normal((k, n)), rng.standard_normal((k, p)), rng.standard_normal((k, m))
            A, B, Cm = nan(k, n), nan(k, p), nan(k, m)
            ks.solve3x3_many_dev(_dev(X), _dev(Y), _dev(Z), A, B, Cm)
            assert all(same(h_, d_) for h_, d_ in zip(ks.solve3x3_many(X.T, Y.T, Z.T), (A, B, Cm))), ("solve3x3_many", k)
            if route == "schur":
                DY, DW = nan(k, n), nan(k, p)
                ks.solve2x2_many_dev(_dev(X), _dev(Y), DY, DW)
                assert all(same(h_, d_) for h_, d_ in zip(ks.solve2x2_many(X.T, Y.T), (DY, DW))), ("solve2x2_many", k)
        assert ks.health()["reg_rel"] == rel
    finally:
        ks.close()


@pytest.mark.parametrize("name", ["allR_330_csr", "allR_150_dense"])
def test_in_place_and_overlapping_dz_take_the_unfused_path(name):
    """include/cipkkt.h, cip_solve4x4_dev: dz may be r itself, or start inside or behind r's s block; such a call runs the
    element-wise generic path (the fused kernels gather r across threads while dz is written) and gives the bits of the unfused
    result of the same problem"""
    import cipkkt
    P = NR.make_problem(name)
    n, p, m = P.n, P.p, P.m
    len4 = n + p + 2 * m
    r = NR.rhs4(P, "graded", np.random.default_rng(11))
    outs = {}
    for which in ("unfused", "separate", "in place", "overlap"):
        if which == "unfused":
            os.environ["CIP_S4_FUSED"] = "0"
        try:
            ks = cipkkt.KKTSystem(P.Q, P.A, P.G, P.cone_dims, route=P.route)
            try:
                lam = _dev(np.zeros(m))
                ks.set_scaling_from_iterate(_dev(P.v), _dev(P.s), lam)
                ks.factor()
                if which in ("unfused", "separate"):
                    rd, dz = _dev(r), torch.full((len4,), float("nan"), dtype=torch.float64, device="cuda")
                elif which == "in place":
                    rd = _dev(r)
                    dz = rd
                else:
                    k = 37                                                  # dz starts 37 entries before the end of r.s
                    buf = torch.full((2 * len4 - k,), float("nan"), dtype=torch.float64, device="cuda")
                    buf[:len4] = _dev(r)
                    rd, dz = buf[:len4], buf[len4 - k:]
                ks.solve4x4_dev(lam, rd, dz)
                torch.cuda.synchronize()
                outs[which] = dz.cpu().numpy()
                assert ks.health()["n_regularized"] == 0
            finally:
                ks.close()
        finally:
            os.environ.pop("CIP_S4_FUSED", None)
    assert np.isfinite(outs["unfused"]).all()
    for which in ("separate", "in place", "overlap"):
        assert _bits(outs[which], outs["unfused"]), which


def test_fused_branch_falls_through_when_its_resolve_regularises():
    """An all-R Schur handle whose first factorisation meets a zero pivot (Q = 0 on free variables that only the equalities
    pin, as test_singular_schur_block_is_regularised_and_refined): factor(check=False) leaves the pivot flag unresolved, so the
    first solve4x4 resolves it INSIDE the fused branch, which switches the regularisation on and must fall through to the
    refined generic path -- the bits of a fresh handle regularised up front, and the reference's step."""
    import cipkkt
    from oracle.conicip import make_cone_ops
    from oracle.kktsolvers import kktsolver_qr
    rng = np.random.default_rng(12)
    n, p, k = 30, 12, 14
    Q = np.zeros((n, n))
    Q[k:k + 4, k:k + 4] = np.eye(4)
    A = np.zeros((k, n))
    A[np.arange(k), np.arange(k)] = 1.0
    G = rng.standard_normal((p, n))
    cone_dims = [("R", k)]
    v, s = rng.random(k) + 0.1, rng.random(k) + 0.1
    r = rng.standard_normal(n + p + 2 * k)
    outs = []
    for up_front in (False, True):
        ks = cipkkt.KKTSystem(Q, A, G, cone_dims)
        try:
            if up_front:
                assert ks.lib.cip_set_regularization(ks.h, C.c_double(LR.REG_AUTO), 1) == 0
            lam = _dev(np.zeros(k))
            ks.set_scaling_from_iterate(_dev(v), _dev(s), lam)
            ks.factor(check=up_front)
            assert ks.health()["n_regularized"] == 0
            dz = torch.full((n + p + 2 * k,), float("nan"), dtype=torch.float64, device="cuda")
            ks.solve4x4_dev(lam, _dev(r), dz)
            torch.cuda.synchronize()
            h = ks.health()
            assert h["reg_rel"] == LR.REG_AUTO and h["n_regularized"] == (0 if up_front else 1)
            outs.append(dz.cpu().numpy())
            lam_h = lam.cpu().numpy()
        finally:
            ks.close()
    assert _bits(outs[0], outs[1])
    # the true operator: the reference's solve4x4 on its null-space QR solver (src/ConicIP.jl:684-692)
    _, nt_scaling, cone_div, _ = make_cone_ops(cone_dims)
    F = nt_scaling(v, s)
    t1 = F.tmul(cone_div(r[n + p + k:], lam_h))
    dy, dw, dv = kktsolver_qr(Q, A, G, cone_dims)(F, F.inv_adjoint())(r[:n], r[n:n + p], r[n + p:n + p + k] + t1)
    ref = np.concatenate([dy, dw, dv, t1 - F.tmul(F.mul(dv))])
    np.testing.assert_allclose(outs[0], ref, rtol=1e-8, atol=1e-9)
