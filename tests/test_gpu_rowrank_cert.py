"""The device full-row-rank certificate (cip_rowrank_cert / cipkkt.full_row_rank_hip) on the GPU.

Verdicts on matrices whose rho = sigma_min / ||M||_F is known by construction (M = U diag(s) V'), at the smallest shapes at which the
padding to 128 rows, the staging panels (1024 columns, multiples of 16) and the in-place path can go wrong, through every way of
handing the same matrix over (dense / CSR blocks, host / device pointers).  The certificate is ONE-SIDED: with thr = max(100 eps,
1e-6), "certified" may only be answered when rho >= thr -- a condition, not a tolerance; "not certified" is always allowed, and it
is demanded only where rho is far below thr.  Then the outputs (fro2, the shift's documented formula, same bits on every run) and the
pre-solve with certificate="device"."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = 1e-8
THR = max(100.0 * EPS, 1e-6)
# n x L: one row; tiny; just below / at / just above one 128-tile; two and three tiles with L % 16 != 0 and L beyond one panel;
# n = 40 with one block wider than the 1024-column staging panel
SHAPES = [(1, 1), (3, 40), (127, 130), (128, 128), (129, 300), (257, 515), (384, 1040), (40, 1100)]
BAND = [THR / 4.0 * 32.0 ** (i / 11.0) for i in range(12)]       # twelve values log-spaced over [thr / 4, 8 thr]


@functools.lru_cache(maxsize=None)
def _factors(n, L):
    rng = np.random.default_rng(1000 * n + L)
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    V = np.linalg.qr(rng.standard_normal((L, n)))[0]            # L x n, orthonormal columns
    return U, V


def with_rho(n, L, rho):
    """(M, rho of M): singular values from 1 down to s_min, log-spaced, with s_min / ||s||_2 = rho"""
    U, V = _factors(n, L)
    smin = rho
    for _ in range(60):
        s = np.geomspace(1.0, smin, n) if n > 1 else np.ones(1)
        smin = rho * np.linalg.norm(s)
    M = (U * s) @ V.T
    return M, float(s[-1] / np.linalg.norm(M))


def call(n, specs, mode="host", eps=EPS):
    """cip_rowrank_cert on blocks given as ("dense", B, ld) or ("csr", S); mode: "host" (flags 0), "dev" (dense blocks on the device,
    CSR arrays on the host), "alldev".  Rows n..ld-1 of a dense block hold NaN: they must never be read.  -> (certified, fro2, shift)"""
    import torch
    from cipkkt import _lib as L
    lib = L.load()
    keep, arr = [], (L.CipCertBlock * max(len(specs), 1))()
    for i, spec in enumerate(specs):
        if spec[0] == "dense":
            _, B, ld = spec
            k = B.shape[1]
            buf = np.full((k, ld), np.nan)
            buf[:, :n] = B.T
            arr[i].cols, arr[i].ld = k, ld
            if k:
                if mode != "host":
                    buf = torch.from_numpy(buf).cuda()
                arr[i].dense = buf.data_ptr() if mode != "host" else buf.ctypes.data
            keep.append(buf)
        else:
            S = sp.csr_matrix(spec[1])
            trio = [S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)]
            if mode == "alldev":
                trio = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in trio]
            keep += trio
            ptr = [a.data_ptr() if mode == "alldev" else a.ctypes.data for a in trio]
            arr[i].cols = S.shape[1]
            arr[i].rowptr, arr[i].colind, arr[i].val = ptr
    torch.cuda.synchronize()
    flags = {"host": 0, "dev": L.FLAG_DEVICE_PTRS | L.FLAG_CSR_HOST, "alldev": L.FLAG_DEVICE_PTRS}[mode]
    ok, fro2, shift = C.c_int(-1), C.c_double(-1.0), C.c_double(-1.0)
    L.check(lib.cip_rowrank_cert(n, len(specs), arr, float(eps), flags, C.byref(ok), C.byref(fro2), C.byref(shift)))
    del keep
    assert ok.value in (0, 1)
    return bool(ok.value), fro2.value, shift.value


def cuts(L):
    """two cut points: multiples of 16 where L allows three blocks of that kind (the device then reads them in place)"""
    return (L // 3 // 16 * 16, 2 * L // 3 // 16 * 16) if L >= 48 else (L // 3, 2 * L // 3)


def splits(M, tail=None):
    """the same matrix [M tail] as block lists; `tail` (a scipy matrix) always goes over as a CSR block"""
    n, L = M.shape
    c1, c2 = cuts(L)
    extra = [("csr", tail)] if tail is not None else []
    return {
        "one dense": [("dense", M, n)] + extra,
        "three dense": [("dense", M[:, :c1], n + 3), ("dense", M[:, c1:c2], n + 2), ("dense", M[:, :0], n), ("dense", M[:, c2:], 3 * n + 20)] + extra,
        "all csr": [("csr", M[:, :c2]), ("csr", M[:, c2:])] + extra,
        "dense + csr": [("csr", M[:, :c1]), ("dense", M[:, c1:], n + 1)] + extra,
    }


def verdicts(M, tail=None):
    """{(split, mode): certified} over every split and pointer mode, with fro2 checked against numpy on the way"""
    n = M.shape[0]
    ref = float(np.sum(M * M)) + (float(tail.multiply(tail).sum()) if tail is not None else 0.0)
    out = {}
    for name, specs in splits(M, tail).items():
        for mode in ("host", "dev", "alldev"):
            ok, fro2, _ = call(n, specs, mode)
            assert abs(fro2 - ref) <= 1e-13 * ref, (name, mode, fro2, ref)
            out[name, mode] = ok
    return out


def test_host_parity_on_the_five_cases_of_the_host_certificates_test():
    """the inputs of tests/test_preprocess.py::test_full_row_rank_certificate_agrees_with_the_pivoted_qr, restated, through the
    public function: the device's verdict is the host's"""
    import cipkkt
    from cipkkt import preprocess as pp
    rng = np.random.default_rng(3)
    n = 40
    Q = rng.standard_normal((n, n)); Q = Q @ Q.T / n
    A = sp.identity(n, format="csr")
    Z = np.zeros((2 * n, 2 * n))
    A2 = sp.hstack([sp.identity(n), sp.identity(n)], format="csr")
    G = rng.standard_normal((3, n))
    G[2] = G[0] + 1e-6 * rng.standard_normal(n)
    cases = [([Q, A.T.tocsr(), np.zeros((n, 0))], True), ([Z, A2.T.tocsr()], False), ([G], False),
             ([rng.standard_normal((3, n))], True), ([np.zeros((3, n))], False)]
    for blocks, expect in cases:
        assert bool(pp._full_row_rank(blocks, 1e-8)) is expect
        assert cipkkt.full_row_rank_hip(blocks, 1e-8) is expect
    # the public function takes device tensors and the transposes of row-major arrays where they lie
    import torch
    Arow = rng.standard_normal((25, n))                                  # A (m x n, row-major): the dual test wants A'
    blocks = [torch.from_numpy(Q).cuda(), torch.from_numpy(Arow).cuda().t(), sp.identity(n, format="csc")]
    assert cipkkt.full_row_rank_hip(blocks) is True
    assert cipkkt.full_row_rank_hip([Q, Arow.T, sp.identity(n, format="csr")]) is True           # a row-major block: device mode
    assert cipkkt.full_row_rank_hip([np.asfortranarray(Q), Arow.T, sp.identity(n, format="csr")]) is True   # host pointers only
    assert cipkkt.full_row_rank_hip([np.asfortranarray(G), np.zeros((3, 0))]) is False
    with pytest.raises(ValueError, match="same number of rows"):
        cipkkt.full_row_rank_hip([Q, np.zeros((n + 1, 2))])


@pytest.mark.parametrize("n, L", SHAPES[1:], ids=["%dx%d" % s for s in SHAPES[1:]])
def test_prescribed_spectra_give_the_verdict_every_way(n, L):
    for rho in (1e-3, 1e-4):
        M, r = with_rho(n, L, rho)
        assert abs(r - rho) < 1e-6 * rho
        v = verdicts(M)
        assert all(v.values()), (rho, v)
    for rho in (1e-8, 1e-10):
        v = verdicts(with_rho(n, L, rho)[0])
        assert not any(v.values()), (rho, v)
    M = with_rho(n, L, 1e-3)[0].copy()
    M[n - 1] = M[0]                                                      # an exactly repeated row
    v = verdicts(M)
    assert not any(v.values()), v
    # a CSR identity beside a nearly rank-deficient block: [M I] has sigma_min^2 = s_min^2 + 1 and ||.||_F^2 = ||M||_F^2 + n
    M, r = with_rho(n, L, 1e-8)
    rho_wide = np.sqrt((r * np.linalg.norm(M)) ** 2 + 1.0) / np.sqrt(np.linalg.norm(M) ** 2 + n)
    assert rho_wide > 100 * THR
    v = verdicts(M, tail=sp.identity(n, format="csr"))
    assert all(v.values()), v


@pytest.mark.parametrize("n, L", SHAPES[1:], ids=["%dx%d" % s for s in SHAPES[1:]])
def test_around_the_threshold_the_certificate_is_one_sided(n, L):
    """either answer passes, but certified => rho >= thr, exactly; and the verdict is the same every way the matrix is handed over"""
    seen = []
    for rho in BAND:
        M, r = with_rho(n, L, rho)
        v = verdicts(M)
        assert len(set(v.values())) == 1, (rho, v)
        ok = next(iter(v.values()))
        seen.append((r / THR, ok))
        assert (not ok) or r >= THR, (r, THR, seen)
    print("rho / thr -> certified:", ", ".join("%.3f %d" % s for s in seen))


def test_one_by_one_and_empty_blocks():
    one = np.array([[3.0]])
    for mode in ("host", "dev", "alldev"):
        assert call(1, [("dense", one, 1)], mode)[0] is True             # rho = 1
        assert call(1, [("dense", one[:, :0], 1), ("csr", one), ("dense", one[:, :0], 4)], mode)[0] is True
        assert call(1, [("dense", 0.0 * one, 2)], mode) == (False, 0.0, 0.0)
    assert call(0, [], "host") == (False, 0.0, 0.0)
    assert call(5, [("dense", np.zeros((5, 0)), 5)], "dev") == (False, 0.0, 0.0)


def test_outputs_follow_the_documented_formulas_and_repeat_bit_for_bit():
    for (n, L) in [(3, 40), (129, 300), (384, 1040)]:
        M, _ = with_rho(n, L, 1e-3)
        tail = sp.identity(n, format="csr")
        for name, specs in splits(M, tail).items():
            for mode in ("host", "alldev"):
                for eps in (1e-8, 1e-7, 0.0):
                    a = call(n, specs, mode, eps)
                    b = call(n, specs, mode, eps)
                    assert a == b                                             # verdict, and the bits of fro2 and shift
                    thr = max(100.0 * eps, 1e-6)
                    assert a[2] == (thr * thr + 2.0 * float(L + n + n) * 2.0 ** -53) * a[1], (name, mode, eps)
                    ref = float(np.sum(M * M)) + n
                    assert abs(a[1] - ref) <= 1e-13 * ref
        # the pointer mode changes nothing in the bits either
        specs = splits(M, tail)["three dense"]
        assert call(n, specs, "host") == call(n, specs, "dev") == call(n, specs, "alldev")


def test_a_non_finite_entry_is_refused():
    from cipkkt import _lib as L
    M, _ = with_rho(129, 300, 1e-3)
    for bad in (np.nan, np.inf, -np.inf, 1e200):                          # (1e200: its square overflows)
        B = M.copy()
        B[77, 201] = bad
        for specs in (splits(B)["one dense"], splits(B)["all csr"]):
            for mode in ("host", "alldev"):
                with pytest.raises(L.CipError, match="non-finite entry") as e:
                    call(129, specs, mode)
                assert e.value.code == -1                                  # CIP_E_INVALID
    assert call(129, splits(M)["one dense"], "host")[0] is True            # nothing lingers


@pytest.mark.parametrize("rank_solver", ["host", "device"])
@pytest.mark.parametrize("check", ["check_redundant", "check_bad_dual", "check_infeasible", "check_miles"])
def test_presolve_with_the_device_certificate(check, rank_solver, monkeypatch):
    import cipkkt
    import test_preprocess as TP
    from cipkkt import preprocess as pp

    def host_must_not_run(*a, **k):
        raise AssertionError("the host certificate ran under certificate=\"device\"")
    monkeypatch.setattr(pp, "_full_row_rank", host_must_not_run)
    getattr(TP, check)(functools.partial(cipkkt.preprocess_conicIP, certificate="device", rank_solver=rank_solver))


def test_a_full_rank_box_qp_goes_through_untouched(monkeypatch):
    """n = 300: both the pre-solve and conicIP called directly return the same bits, because the certificate holds and nothing is
    dropped or augmented; the device certificate is what ran"""
    import cipkkt
    from cipkkt import qrcp
    rng = np.random.default_rng(11)
    n = 300
    Mq = rng.standard_normal((n, n))
    Q = Mq.T @ Mq / n
    c = rng.standard_normal(n)
    A = sp.identity(n, format="csr")
    b = -rng.random(n)
    calls = []
    real = qrcp.full_row_rank_hip

    def spy(blocks, eps=1e-8):
        calls.append(real(blocks, eps))
        return calls[-1]
    monkeypatch.setattr(qrcp, "full_row_rank_hip", spy)
    got = cipkkt.preprocess_conicIP(Q, c, A, b, [("R", n)], certificate="device", optTol=1e-7)
    ref = cipkkt.conicIP(Q, c, A, b, [("R", n)], optTol=1e-7)
    assert calls == [True]                                                 # (no equality rows: the dual certificate alone)
    assert got.status == ref.status == "Optimal" and got.Iter == ref.Iter
    assert got.y.tobytes() == ref.y.tobytes() and got.v.tobytes() == ref.v.tobytes()
    assert got.w.shape == (0,)
