"""tests/_ldlt_ref.py on its own (no GPU): known answers for the two bounds, the fp64 model of the shipped algorithm inside
both bounds on every matrix family, and every matrix the GPU tests factor shown to be factorisable in the static pivot
order -- pivots of the expected sign, no zero / non-finite pivot -- which is the condition for no GPU case being skipped."""
import numpy as np
import pytest

import _ldlt_ref as R

# (family member, outer-block widths of the model, solve blocks): orders up to 768, long-double products stay short
MEMBERS = [
    ("benign", (384, 38), [256, 128], (128,)),
    ("schur_graded", (448, 64, 3), [128] * 4, (128, 512)),
    ("schur_graded", (704, 64, 6), [512, 256], (256,)),
    ("schur_graded", (448, 64, 6), [512], (512,)),
    ("full3x3_graded", (256, 384, 128, 6), [512, 256], (128, 256)),
    ("full3x3_graded", (300, 400, 68, 3), [768], (256,)),
    ("regularised", (448, 64, R.REG_AUTO), [512], (512,)),
    ("regularised", (448, 64, 1e-8), [512], (128, 512)),
]


def _ids(v):
    return "%s%s" % (v[0], "-".join(str(a) for a in v[1]))


def test_unit_lower_inverse_is_an_inverse():
    rng = np.random.default_rng(3)
    L = np.tril(rng.standard_normal((2, 256, 256)), -1) * 0.3 + np.eye(256)
    X = R.unit_lower_inverse(L.astype(R.LD))
    for J in range(2):
        Lq = L[J].astype(R.LD)
        assert np.all(np.abs(X[J] @ Lq - np.eye(256)) <= 256 * 2.0 ** -63 * (np.abs(X[J]) @ np.abs(Lq)))
        assert np.abs(np.triu(X[J], 1)).max() == 0.0


def test_the_graded_families_are_graded():
    """what the module docstring claims for them, so that the GPU table reaches what it says it reaches"""
    F, _, _, info = R.model_factor(R.benign(384, 38).K)
    L, d = R.split_factor(F)
    assert info == 0 and np.abs(np.tril(L, -1)).max() <= 1.0 and np.abs(d).max() / np.abs(d).min() < 1e3
    for spread in (3, 6):
        F, _, _, info = R.model_factor(R.schur_graded(448, 64, spread).K)
        L, d = R.split_factor(F)
        assert info == 0 and np.abs(d).max() / np.abs(d).min() > 10.0 ** (2 * spread - 1) and np.abs(np.tril(L, -1)).max() > 3.0
        F, _, _, info = R.model_factor(R.full3x3_graded(256, 384, 128, spread).K)
        L, d = R.split_factor(F)
        assert info == 0 and np.abs(np.tril(L, -1)).max() > 10.0 ** (spread - 1)


def test_factor_bound_known_answers():
    """the last pivot moved by k N u B_nn changes exactly one entry of L D L' by that much: inside the bound for small k,
    outside for large k (the model's own residual there is a few u B)"""
    for case in (R.benign(384, 0), R.schur_graded(448, 64, 6)):
        F, _, _, _ = R.model_factor(case.K)
        N = F.shape[0]
        L, d = R.split_factor(F)
        Bnn = float(np.sum(L[-1].astype(R.LD) ** 2 * np.abs(d).astype(R.LD)))
        for k, want in ((0.5, True), (2.0, True), (4.0, False), (100.0, False)):
            F2 = F.copy()
            F2[-1, -1] += k * N * R.U * Bnn
            got = R.factor_check(case.K, F2)
            assert got["ok"] == want, (case.name, k, got)
            if not want:
                assert got["at"] == (N - 1, N - 1)
        # an entry of L under a micro-block: row i of L D L' moves in the columns j >= c; the largest move relative to the
        # bound is made k times the bound
        i, c = N - 5, 37
        base = R.factor_check(case.K, F)
        assert base["ok"] and base["ratio"] < 0.05, base
        for k, want in ((0.5, True), (50.0, False)):
            step = 2.0 ** -40 * abs(F[i, c])
            F2 = F.copy()
            F2[i, c] += step
            r = R.factor_check(case.K, F2)["ratio"]                   # linear in the step as long as the step dominates
            F2[i, c] = F[i, c] + step * k / r
            assert R.factor_check(case.K, F2)["ok"] == want, (case.name, k)


def test_solve_bound_known_answers():
    for case, Bs in ((R.benign(384, 38), 128), (R.full3x3_graded(256, 384, 128, 6), 256)):
        F, rho, Xm, _ = R.model_factor(case.K)
        N = F.shape[0]
        b = np.random.default_rng(5).standard_normal(N)
        x = R.model_solve(F, rho, R.model_block_inverses(F, Xm, Bs), b)
        sb = R.SolveBound(F, Bs, knorm=np.linalg.norm(case.K))
        base = sb.check(b, x, R.C_S["gemv"])
        assert base["ok"] and base["ratio"] < 0.05, base
        L, d = R.split_factor(F)
        i = N // 3
        col = (L * d) @ L[i]                                          # column i of L D L'
        j = int(np.argmax(np.abs(col) / base["bound"]))
        for k, want in ((0.5, True), (4.0, False), (1e3, False)):
            x2 = x.copy()
            x2[i] += k * base["bound"][j] / abs(col[j])              # moves r_j by k bound_j, every other r_l by less
            assert sb.check(b, x2, R.C_S["gemv"])["ok"] == want, (case.name, k)
        x2 = x.copy()
        x2[3] = np.nan
        assert not sb.check(b, x2, R.C_S["gemv"])["ok"]


@pytest.mark.parametrize("member", MEMBERS, ids=_ids)
def test_model_meets_both_bounds(member):
    fam, args, widths, blocks = member
    case = R.FAMILIES[fam](*args)
    F, rho, Xm, info = R.model_factor(case.K, widths)
    assert info == 0
    assert np.array_equal(np.sign(np.diag(F)), R.expected_signs(case))
    fc = R.factor_check(case.K, F)
    print("%-34s factor: |E| <= %.3g x bound, %.1f u B, micro |L11||inv L11| <= %.3g" % (case.name, fc["ratio"], fc["textbook"], fc["micro"]))
    assert fc["ok"], fc
    assert fc["textbook"] < F.shape[0]                                 # the scale the issue measured: far below N
    knorm = np.linalg.norm(case.K)
    rng = np.random.default_rng(11)
    for Bs in blocks:
        sb = R.SolveBound(F, Bs, knorm)
        X = R.model_block_inverses(F, Xm, Bs)
        for trial in range(2):
            b = rng.standard_normal(F.shape[0]) * (10.0 ** rng.uniform(-3, 3, F.shape[0]) if trial else 1.0)
            sc = sb.check(b, R.model_solve(F, rho, X, b), R.C_S["gemv"])
            print("%-34s solve Bs %4d: |r| <= %.3g x bound, %.3g x plain substitution, backward error %.2g"
                  % (case.name, Bs, sc["ratio"], sc["plain"], sc["nbe"]))
            assert sc["ok"], {k: v for k, v in sc.items() if k not in ("r", "bound")}


def test_the_table_of_gpu_cases_matches_the_dispatch_rules():
    for name, c in R.GPU_CASES.items():
        case_N = -(-{"benign": lambda a: a[0], "schur_graded": lambda a: a[0] + a[1], "regularised": lambda a: a[0] + a[1],
                     "full3x3_graded": lambda a: a[0] + a[1] + a[2]}[c["fam"]](c["args"]) // 128) * 128
        widths, Bs, fused = R.dispatch(case_N, c["chain"], c["nbo"], c["bs"], c["fused"])
        assert (widths, Bs, fused) == (list(c["expect"][0]), c["expect"][1], c["expect"][2]), name
    reached = {k: set() for k in ("chain", "bs", "fused", "trail")}
    for c in R.GPU_CASES.values():
        reached["chain"].add(c["chain"])
        reached["bs"].add(c["expect"][1])
        reached["fused"].add(c["expect"][2])
        reached["trail"].update(c["expect"][0][:-1])                   # K of the trailing updates
    assert reached["chain"] == {0, 3} and reached["bs"] == {128, 256, 512, 1024} and reached["fused"] == {False, True}
    assert {128, 512, 896, 1024} <= reached["trail"]
    # side preparation on and off: only on a handle row whose order makes the factorisation fork
    side_rows = [n for n, h in R.HANDLES.items() if h[6]]
    assert side_rows and all(set(R.HANDLES[n][6]) == {0, 1} and R.side_prep_forks(R.handle_order(n)) for n in side_rows)
    assert not any(R.side_prep_forks(R.handle_order(n)) for n in R.HANDLES if n not in side_rows)
    assert not any("side" in c for c in R.GPU_CASES.values())          # the stand-alone entry has no side stream


@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_every_gpu_case_is_factorisable_in_the_static_order(name):
    """the model, run with the case's own outer blocks, meets no zero / non-finite pivot and every pivot has the sign of its
    block: the device must factor it too, so no GPU case may be skipped or expected to fail"""
    case = R.build_case(name)
    F, _, _, info = R.model_factor(case.K, R.GPU_CASES[name]["expect"][0])
    assert info == 0
    assert np.array_equal(np.sign(np.diag(F)), R.expected_signs(case))
    assert np.isfinite(F).all()
