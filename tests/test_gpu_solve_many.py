"""Many right-hand sides for one LDL' factor: cip_ldlt_solve_many_dev (stand-alone) and cip_solve3x3_many* / cip_solve2x2_many*
(handle), against numpy and against the single-column entry points, with the bit-level promises of include/cipkkt.h."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problems as P  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = dict(dtype=torch.float64, device="cuda")
POISON = 1 << 29


@pytest.fixture(scope="module")
def lib():
    import cipkkt
    return cipkkt._lib.load()


@contextlib.contextmanager
def solve_settings(lib, block_max=None, fused=None):
    pb = lib.cip_set_solve_block_max(block_max if block_max else 0)
    pf = lib.cip_set_solve_fused(fused if fused is not None else -1)
    try:
        yield
    finally:
        lib.cip_set_solve_block_max(pb)
        lib.cip_set_solve_fused(pf)


# ---------------------------------------------------------------------------------------------------- stand-alone
def _quasi_definite(N, seed):
    """[[SPD, G'], [G, -I]] of order N (torch, on the GPU), SPD block of order 3N/4."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n1 = N - N // 4
    M = torch.randn(n1, n1, generator=g, **F64)
    S = M @ M.t() / n1 + torch.eye(n1, **F64)
    G = torch.randn(N - n1, n1, generator=g, **F64) / np.sqrt(n1)
    K = torch.zeros(N, N, **F64)
    K[:n1, :n1] = S
    K[n1:, :n1] = G
    K[:n1, n1:] = G.t()
    K[n1:, n1:] = -torch.eye(N - n1, **F64)
    return K


class Factored:
    """K factored by cip_ldlt_factor_dev in a (N x ld) buffer."""

    def __init__(self, lib, K, ld):
        from cipkkt import _lib as L
        self.lib, self.N, self.ld, self.K = lib, K.shape[0], ld, K
        nb = C.c_size_t()
        L.check(lib.cip_ldlt_workspace_bytes(self.N, C.byref(nb)))
        self.ws = torch.empty(nb.value // 8 + 1, **F64)
        self.buf = torch.full((self.N, ld), float("nan"), **F64)       # column j = row j of the tensor
        self.buf[:, :self.N] = K.t()
        info = C.c_int()
        L.check(lib.cip_ldlt_factor_dev(None, self.buf.data_ptr(), self.N, ld, self.ws.data_ptr(), C.byref(info)))
        torch.cuda.synchronize()
        assert info.value == 0

    def many(self, B, ldb=None, scratch=None):
        """B: (nrhs, ldb) tensor = column-major N x nrhs with leading dimension ldb; solved in place."""
        from cipkkt import _lib as L
        nrhs = B.shape[0]
        ldb = ldb or B.shape[1]
        if scratch is None:
            nb = C.c_size_t()
            L.check(self.lib.cip_ldlt_solve_many_scratch_bytes(self.N, nrhs, C.byref(nb)))
            scratch = torch.empty(max(nb.value // 8, 1), **F64)
        L.check(self.lib.cip_ldlt_solve_many_dev(None, self.buf.data_ptr(), self.N, self.ld, self.ws.data_ptr(), scratch.data_ptr(),
                                                 B.data_ptr(), ldb, nrhs))
        torch.cuda.synchronize()
        return B

    def single(self, b):
        from cipkkt import _lib as L
        x = b.clone()
        L.check(self.lib.cip_ldlt_solve_dev(None, self.buf.data_ptr(), self.N, self.ld, self.ws.data_ptr(), x.data_ptr()))
        return x


def _check_against_numpy_and_single(f, nrhs, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = torch.randn(nrhs, f.N, generator=g, **F64)
    X = f.many(B.clone())
    R = X @ f.K - B                                  # rows: K x_j - b_j (K symmetric)
    knorm = float(torch.linalg.norm(f.K))
    rel = (torch.linalg.norm(R, dim=1) / (knorm * torch.linalg.norm(X, dim=1))).max().item()
    assert rel <= 1e-12, (f.N, f.ld, nrhs, rel)
    Xs = torch.stack([f.single(B[j]) for j in range(nrhs)])
    torch.cuda.synchronize()
    d = ((X - Xs).abs().max(dim=1).values / Xs.abs().max(dim=1).values).max().item()
    assert d <= 1e-11, (f.N, f.ld, nrhs, d)


@pytest.mark.parametrize("N", [128, 1024, 4608, 8192])
@pytest.mark.parametrize("pad", [0, 128])
def test_standalone_many_against_numpy_and_the_single_solve(lib, N, pad):
    f = Factored(lib, _quasi_definite(N, 10 + N + pad), N + pad)
    for nrhs in ([2, 7, 16, 33, 64, 100] if N <= 4608 else [2, 33, 100]):
        _check_against_numpy_and_single(f, nrhs, nrhs)


@pytest.mark.parametrize("block_max", [128, 256, 512, 1024])
@pytest.mark.parametrize("fused", [0, 2])
def test_standalone_many_every_solve_block_and_solve_mode(lib, block_max, fused):
    with solve_settings(lib, block_max, fused):
        f = Factored(lib, _quasi_definite(2048, 77 + block_max + fused), 2048)
        for nrhs in (2, 33, 70):
            _check_against_numpy_and_single(f, nrhs, nrhs + block_max)


def test_standalone_many_leaves_the_padding_rows_alone(lib):
    N, ldb, nrhs = 1024, 1024 + 37, 9
    f = Factored(lib, _quasi_definite(N, 5), N)
    g = torch.Generator(device="cuda").manual_seed(1)
    B = torch.full((nrhs, ldb), float("nan"), **F64)
    B[:, :N] = torch.randn(nrhs, N, generator=g, **F64)
    b0 = B.clone()
    f.many(B, ldb=ldb)
    assert torch.isfinite(B[:, :N]).all()
    assert torch.isnan(B[:, N:]).all()
    X = B[:, :N]
    rel = (torch.linalg.norm(X @ f.K - b0[:, :N], dim=1) / (float(torch.linalg.norm(f.K)) * torch.linalg.norm(X, dim=1))).max().item()
    assert rel <= 1e-12


def test_standalone_many_bits(lib):
    N = 4608
    f = Factored(lib, _quasi_definite(N, 3), N)
    g = torch.Generator(device="cuda").manual_seed(2)
    B = torch.randn(64, N, generator=g, **F64)
    # nrhs = 1 is the single solve, bit for bit
    one = f.many(B[5:6].clone())
    assert torch.equal(one[0], f.single(B[5]))
    # column j of a 64-column call == the same column of a 2-column call with another partner, and repeats are identical
    X64 = f.many(B.clone())
    assert torch.equal(X64, f.many(B.clone()))
    for j in (0, 17, 40, 63):
        partner = torch.randn(1, N, generator=g, **F64)
        pair = f.many(torch.cat([partner, B[j:j + 1]]).contiguous())
        assert torch.equal(pair[1], X64[j]), j
    # ... and in a 100-column call (second chunk of 64)
    X100 = f.many(torch.cat([torch.randn(36, N, generator=g, **F64), B]).contiguous())
    assert torch.equal(X100[36:], X64)


# ---------------------------------------------------------------------------------------------------- handle level
def _problem(kind, p, dense, seed=1):
    if kind == "R":
        Q, _, A, _, cd, G, _, _ = P.random_mixed(n=40, nq=0, p=max(p, 1), seed=seed)
    elif kind == "mixed":
        Q, _, A, _, cd, G, _, _ = P.random_mixed(n=40, nq=3, kq=6, p=max(p, 1), seed=seed)
        rng = np.random.default_rng(seed)
        A = np.vstack([A, rng.standard_normal((6, 40)) * 0.3])        # one S cone of order 3
        cd = list(cd) + [("S", 6)]
    else:
        from cipkkt import workloads as W
        Q, _, A, _, cd, G, _ = W.c4_sdp(r=133, n=12, p=max(p, 1))
    G = np.asarray(G)[:p]
    A = np.asarray(A)
    return Q, (A if dense else sp.csr_matrix(A)), G, cd


def _blocks(ks, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ks.n, k)), rng.standard_normal((ks.p, k)), rng.standard_normal((ks.m, k))


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


CASES = [("R", 0), ("R", 4), ("mixed", 4), ("sdp133", 2), ("sdp133", 0)]


@pytest.mark.parametrize("route", ["schur", "full"])
@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("kind,p", CASES)
def test_handle_many_against_single_solves(route, dense, kind, p):
    import cipkkt
    Q, A, G, cd = _problem(kind, p, dense)
    ks = cipkkt.KKTSystem(Q, A, G, cd, route=route)
    try:
        ks.set_scaling_identity()
        ks.factor(check=True)
        for k in (1, 5, 40, 70):
            X, Y, Z = _blocks(ks, k, k)
            A3, B3, C3 = ks.solve3x3_many(X, Y, Z)
            single = [ks.solve3x3(X[:, j], Y[:, j], Z[:, j]) for j in range(k)]
            for got, ref in zip((A3, B3, C3), [np.stack([s[i] for s in single], axis=1) for i in range(3)]):
                if k == 1:
                    assert np.array_equal(got, ref), (kind, p, route, dense)
                else:
                    assert _rel(got, ref) <= 1e-11, (kind, p, route, dense, k, _rel(got, ref))
            if route == "schur":
                DY, DW = ks.solve2x2_many(X, Y)
                single2 = [ks.solve2x2(X[:, j], Y[:, j]) for j in range(k)]
                for got, ref in zip((DY, DW), [np.stack([s[i] for s in single2], axis=1) for i in range(2)]):
                    assert (np.array_equal(got, ref) if k == 1 else _rel(got, ref) <= 1e-11), (kind, p, dense, k)
            else:
                with pytest.raises(cipkkt.CipError) as e:
                    ks.solve2x2_many(X, Y)
                assert e.value.code == cipkkt._lib.E_UNSUPPORTED
    finally:
        ks.close()


def test_regularised_handle_many_is_refined_single_solves():
    import cipkkt
    n = 12
    Q = np.zeros((n, n))
    A = np.zeros((n, n))
    A[:n - 2, :n - 2] = np.eye(n - 2)
    A[n - 2, 0] = 1.0
    A[n - 1, 1] = 1.0
    G = np.zeros((2, n))
    G[0, n - 2] = 1.0
    G[1, n - 1] = 1.0
    ks = cipkkt.KKTSystem(Q, A, G, [("R", n)])
    try:
        ks.set_scaling_identity()
        ks.factor(check=True)
        rel, switched = C.c_double(), C.c_int()
        cipkkt._lib.check(ks.lib.cip_get_regularization(ks.h, C.byref(rel), C.byref(switched)))
        assert rel.value > 0 and switched.value == 1
        X, Y, Z = _blocks(ks, 9, 3)
        A3, B3, C3 = ks.solve3x3_many(X, Y, Z)
        single = [ks.solve3x3(X[:, j], Y[:, j], Z[:, j]) for j in range(9)]
        for i, got in enumerate((A3, B3, C3)):
            assert np.array_equal(got, np.stack([s[i] for s in single], axis=1))
        DY, DW = ks.solve2x2_many(X, Y)
        single2 = [ks.solve2x2(X[:, j], Y[:, j]) for j in range(9)]
        assert np.array_equal(DY, np.stack([s[0] for s in single2], axis=1))
        assert np.array_equal(DW, np.stack([s[1] for s in single2], axis=1))
        cipkkt._lib.check(ks.lib.cip_get_regularization(ks.h, C.byref(rel), C.byref(switched)))
        assert switched.value == 1
    finally:
        ks.close()


def test_speculative_many_solve_after_a_poisoned_giveup(lib):
    """As test_gpu_giveup.py's speculative single solve: order 4096, the handle's second factorisation poisoned; the many-solve right
    behind cip_factor or cip_check_factor says "repeat them" (CIP_E_RETRY), and the repeated answer solves the true system (F = I)."""
    import cipkkt
    from cipkkt import _lib as L
    from cipkkt import workloads as W
    n, k = 4096, 6
    Q, _, A, _, cd = W.c2_problem(n, seed=91)
    Q = np.asarray(Q)
    ks = cipkkt.KKTSystem(Q, A, None, cd)
    try:
        ks.set_scaling_identity()
        ks.factor(check=True)
        g = torch.Generator(device="cuda").manual_seed(4)
        X, Z = torch.randn(k, n, generator=g, **F64), torch.randn(k, n, generator=g, **F64)
        Y, Bo = torch.zeros(k, 0, **F64), torch.zeros(k, 0, **F64)
        A3, C3 = torch.zeros(k, n, **F64), torch.zeros(k, n, **F64)
        lib.cip_debug_chain_giveup(1 | POISON)
        try:
            ks.factor(check=False)
            repeats = 0
            try:
                ks.solve3x3_many_dev(X, Y, Z, A3, Bo, C3)
            except cipkkt.CipError as e:
                assert e.code == L.E_RETRY, str(e)
                ks.solve3x3_many_dev(X, Y, Z, A3, Bo, C3)
                repeats += 1
            rc = lib.cip_check_factor(ks.h)
            if rc == L.E_RETRY:
                ks.solve3x3_many_dev(X, Y, Z, A3, Bo, C3)
                repeats += 1
            else:
                L.check(rc)
            torch.cuda.synchronize()
            assert repeats <= 1, repeats
            assert lib.cip_debug_chain_giveup(-1) == 0
        finally:
            lib.cip_debug_chain_giveup(0)
        assert lib.cip_get_chain_fallbacks(ks.h) == 1
        Qd, Ad = torch.as_tensor(Q, **F64), torch.as_tensor(A.toarray(), **F64)
        r1 = A3 @ Qd - C3 @ Ad - X                        # rows: Q a - A'c - x (Q symmetric)
        r3 = A3 @ Ad.t() + C3 - Z                          # A a + c - z
        scale = 1 + max(float(torch.linalg.norm(v)) for v in (A3, C3))
        assert max(float(torch.linalg.norm(r1)), float(torch.linalg.norm(r3))) < 1e-8 * scale
    finally:
        ks.close()


def test_python_layer_matches_the_c_calls():
    import cipkkt
    Q, A, G, cd = _problem("mixed", 4, True)
    ks = cipkkt.KKTSystem(Q, A, G, cd)
    try:
        ks.set_scaling_identity()
        ks.factor(check=True)
        X, Y, Z = _blocks(ks, 12, 8)
        A3, B3, C3 = ks.solve3x3_many(X, Y, Z)
        dX, dY, dZ = (torch.as_tensor(np.ascontiguousarray(M.T), **F64) for M in (X, Y, Z))
        dA, dB = torch.empty_like(dX), torch.empty_like(dY)
        ks.solve3x3_many_dev(dX, dY, dZ, dA, dB, dZ)          # C may alias Z
        torch.cuda.synchronize()
        assert np.array_equal(dA.cpu().numpy().T, A3) and np.array_equal(dB.cpu().numpy().T, B3)
        assert np.array_equal(dZ.cpu().numpy().T, C3)
        DY, DW = ks.solve2x2_many(X, Y)
        dY2, dW2 = torch.empty_like(dX), torch.empty_like(dY)
        dX = torch.as_tensor(np.ascontiguousarray(X.T), **F64)
        dYin = torch.as_tensor(np.ascontiguousarray(Y.T), **F64)
        ks.solve2x2_many_dev(dX, dYin, dY2, dW2)
        torch.cuda.synchronize()
        assert np.array_equal(dY2.cpu().numpy().T, DY) and np.array_equal(dW2.cpu().numpy().T, DW)
    finally:
        ks.close()
