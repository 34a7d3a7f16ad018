"""tests/_newton_ref.py on the CPU: the fp64 model of the shipped Newton-step chain passes every stage check on every case
of the table, the checks reject each planted defect at the stage that owns it, the table reaches the paths it names, and the
end-to-end margin of every case follows its rule (model against oracle).  No GPU."""
import functools

import numpy as np
import pytest

import _ldlt_ref as LR
import _newton_ref as NR


@functools.lru_cache(maxsize=None)
def _setup(name):
    P = NR.make_problem(name)
    cones, lam = NR.model_inputs(P)
    model = NR.Model(P, cones)
    return P, cones, lam, model, LR.SolveBound(model.fac, model.Bs)


def _rhs(P, kind):
    return NR.rhs4(P, kind, np.random.default_rng([len(P.name), P.n, kind == "graded"]))


def _failed(checks):
    return {k: v["ratio"] for k, v in checks.items() if not v["ok"]}


@pytest.mark.parametrize("name", list(NR.CASES))
def test_model_passes_every_stage(name):
    P, cones, lam, model, sb = _setup(name)
    assert model.wrong_signs == 0, "the case would need the regularised factorisation"
    c_s = LR.C_S["gemv"]
    for kind in ("normal", "graded"):
        r = _rhs(P, kind)
        dz = model.solve4x4(lam, r)
        checks = NR.check_4x4(P, cones, sb, c_s, lam, r, dz, pad=model.pad)
        assert not _failed(checks), (name, kind, _failed(checks))
        assert {"rhs+sweeps", "padding"} <= set(checks) and (P.m == 0) == ("ds" not in checks)
    rng = np.random.default_rng(5)
    x, y, z = rng.standard_normal(P.n), rng.standard_normal(P.p), rng.standard_normal(P.m)
    a, b, c = model.solve3x3(x, y, z if P.m else None)
    checks = NR.check_3x3(P, cones, sb, c_s, x, y, z if P.m else None, a, b, c, pad=model.pad)
    assert not _failed(checks), (name, "solve3x3", _failed(checks))
    if P.route == "schur":
        a, b, _ = model.solve3x3(x, y, None)
        checks = NR.check_3x3(P, cones, sb, c_s, x, y, None, a, b, None, pad=model.pad)
        assert not _failed(checks), (name, "solve2x2", _failed(checks))


# defect -> the cases it is planted in (a case must have what the defect needs: an S cone for F against F', an R row,
# padding rows, equality rows)
PLANTED = {
    "dv_entry": ["RQ_schur_dense", "allR_330_csr"],
    "F_for_FT": ["S7_schur", "S7_full"],
    "f_for_ff": ["allR_330_dense", "RQ_schur_csr"],
    "csr_last_A": ["allR_150_csr", "RQ_schur_dense"],
    "csr_last_At": ["RQ_schur_csr", "S7_schur"],
    "pad_one": ["allR_330_csr", "RQ_full_dense"],
    "ds_before": ["RQ_schur_csr", "S7_full"],
    "shift_yw": ["RQ_schur_dense", "RQ_full_dense"],
}


def test_every_defect_is_planted():
    assert set(PLANTED) == set(NR.DEFECTS)


@pytest.mark.parametrize("defect,name", [(d, n) for d, ns in PLANTED.items() for n in ns])
@pytest.mark.parametrize("kind", ["normal", "graded"])
def test_planted_defect_fails_the_stage_that_owns_it(defect, name, kind):
    P, cones, lam, model, sb = _setup(name)
    r = _rhs(P, kind)
    if defect == "dv_entry":
        # the entry whose bound is smallest against its size: 1e-10 relative must stand out there
        dz = model.solve4x4(lam, r)
        clean = NR.check_4x4(P, cones, sb, LR.C_S["gemv"], lam, r, dz)
        dv = dz[P.n + P.p:P.n + P.p + P.m]
        model.dv_at = int(np.argmax(np.abs(dv) / clean["backsub"]["bound"]))
    if defect == "csr_last_At":
        # t spans twenty decades: an entry of A' that meets a small t_j is legitimately below the row's bound.  Take the row
        # whose last stored entry weighs most against the clean bound.  (The cases are those whose K determines the solution
        # well enough: SolveBound is a backward-error bound, it grows with the solution, and on the all-R cases a dropped
        # entry moves the solution along a nearly singular direction of K and the bound with it -- there the bitwise
        # identities of tests/test_gpu_newton.py pin the gathers instead.)
        clean = NR.check_4x4(P, cones, sb, LR.C_S["gemv"], lam, r, model.solve4x4(lam, r))
        n, p, m = P.n, P.p, P.m
        t1 = cones.apply(NR.OP_FT, cones.div64(r[n + p + m:], lam), np.float64)
        t = cones.ftf_inv(r[n + p:n + p + m] + t1, np.float64)
        last = np.array([np.nonzero(P.Ad[:, i])[0][-1] for i in range(n)])
        model.at_row = int(np.argmax(np.abs(P.Ad[last, np.arange(n)] * t[last]) / clean["rhs+sweeps"]["bound"][:n]))
    dz = model.solve4x4(lam, r, defect)
    checks = NR.check_4x4(P, cones, sb, LR.C_S["gemv"], lam, r, dz, pad=model.pad)
    owner = NR.DEFECTS[defect]
    assert not all(checks[st]["ok"] for st in NR.OWNERS.get(owner, (owner,))), (defect, name, kind, {k: v["ratio"] for k, v in checks.items()})


def test_case_table_reaches_the_named_paths():
    reached = set().union(*(NR.paths(n) for n in NR.CASES))
    assert {"fused m>Npad", "fused m<Npad", "fused two workgroups", "csr", "dense", "generic", "schur", "full3x3", "no padding",
            "chunk short", "chunk edge 64", "chunk edge 65"} <= reached
    for name, want in (("allR_330_dense", {"fused m>Npad", "fused two workgroups", "dense"}), ("allR_330_csr", {"fused m>Npad", "csr"}),
                       ("allR_150_dense", {"fused m<Npad", "dense"}), ("allR_150_csr", {"fused m<Npad", "csr"}),
                       ("RQ_schur_csr", {"generic", "csr"}), ("RQ_full_dense", {"generic", "full3x3"}), ("N128_RQ", {"no padding"})):
        assert want <= NR.paths(name), name
    for name, c in NR.CASES.items():
        m = sum(k for _, k in c["cones"])
        if "fused" in NR.paths(name):
            # section starts of the 4-block vectors off the 64-lane boundaries
            assert all(o % 64 for o in (c["n"], c["n"] + c["p"], c["n"] + c["p"] + m) if o), name
    assert {t for c in NR.CASES.values() for t, _ in c["cones"]} == {"R", "Q", "S"}
    assert {k for c in NR.CASES.values() for t, k in c["cones"] if t == "Q"} >= {1, 8, 64, 70}
    assert {k for c in NR.CASES.values() for t, k in c["cones"] if t == "S"} == {28, 1225, 8911}
    assert any(not c["cones"] for c in NR.CASES.values()) and any(c["p"] == 0 for c in NR.CASES.values())
    assert {c["mu"] for c in NR.CASES.values()} == {1e-2, 1e-6, 1e-10}


def test_margin_rule():
    """the larger of 4 and twice the worst model / oracle ratio, the oracle's figure floored at 16 u"""
    assert NR.margin_of(0.3) == 4.0 and NR.margin_of(2.0) == 4.0 and NR.margin_of(3.5) == 7.0 and NR.margin_of(2e10) == 4e10
    assert NR.E2E_FLOOR == 16 * NR.U
    assert NR.e2e_ratio([2.0 ** -10, 0.0, 4e-16, 1e-16], [2.0 ** -40, 0.0, 1e-17, 1e-16]) == 2.0 ** 30     # 4e-16 / 16 u = 0.225, not 40
    assert NR.e2e_ratio([0.0, 0.0, 4e-16, 1e-16], [0.0, 0.0, 1e-17, 1e-16]) == 4e-16 / (16 * NR.U)
    P = NR.make_problem("m0_schur")
    table = NR.rhs_table(P)
    assert [(k, d) for k, d, _ in table] == [(k, d) for k in ("normal", "graded") for d in range(3)]
    assert np.array_equal(table[0][2], _rhs(P, "normal")) and np.array_equal(table[3][2], _rhs(P, "graded"))
    assert len({r.tobytes() for _, _, r in table}) == 6


@pytest.mark.parametrize("name", [n for n, c in NR.CASES.items() if c.get("oracle", True)])
def test_case_margin_is_measured_from_the_model(name):
    """case_margin follows the rule on the model's own figures (what tests/test_gpu_newton.py holds the device to), and the
    figures are finite; the line printed per case is the CPU column of the table in DESIGN_LOG.md"""
    P, cones, lam, model, _ = _setup(name)
    margin, worst, rows = NR.case_margin(P, model, cones, lam)
    assert len(rows) == 6 and all(np.isfinite(mo).all() and np.isfinite(orc).all() for _, _, mo, orc in rows)
    assert worst == max(NR.e2e_ratio(mo, orc) for _, _, mo, orc in rows) and margin == NR.margin_of(worst) >= 4.0
    print("MARGIN | %s | worst model / oracle ratio %.3g | margin %.3g" % (name, worst, margin))
