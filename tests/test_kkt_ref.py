"""The reference builder of the assembly parity tests (tests/_kkt_ref.py) against the oracle's own matrices:
oracle.kktsolvers.schur2x2 (exact (F'F)^-1) and assemble3x3 (the literal 3x3 matrix), at small shapes with R, Q and S
cones, both routes, dense and CSR A.  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp

import _kkt_ref as KR
from oracle.block import Block, Diagonal
from oracle.cones import mat, vecm
from oracle.conicip import make_cone_ops
from oracle.kktsolvers import assemble3x3, schur2x2


def _interior(cone_dims, rng):
    xs = []
    for t, k in cone_dims:
        if t == "R":
            xs.append(rng.random(k) + 0.1)
        elif t == "Q":
            x = rng.standard_normal(k)
            x[0] = np.linalg.norm(x[1:]) + rng.random() + 0.1
            xs.append(x)
        else:
            r = KR._order(k)
            M = rng.standard_normal((r, r))
            xs.append(vecm(M @ M.T / r + 0.5 * np.eye(r)))
    return np.concatenate(xs)


CASES = [
    [("R", 7)],
    [("Q", 1), ("Q", 2), ("Q", 5), ("R", 3)],
    [("S", 6), ("S", 1)],
    [("R", 4), ("Q", 6), ("S", 10), ("Q", 3)],
]


def _problem(cone_dims, n, p, seed, csr):
    rng = np.random.default_rng(seed)
    m = sum(k for _, k in cone_dims)
    M = rng.standard_normal((n, n))
    Q = M @ M.T / n + 0.5 * np.eye(n)
    A = rng.standard_normal((m, n))
    if csr:
        A = A * (rng.random((m, n)) < 0.5)
        A[np.arange(m), rng.integers(0, n, m)] = 1.0
    G = rng.standard_normal((p, n))
    _, nt_scaling, _, _ = make_cone_ops(cone_dims)
    F = nt_scaling(_interior(cone_dims, rng), _interior(cone_dims, rng))
    return Q, (sp.csr_matrix(A) if csr else A), G, F


@pytest.mark.parametrize("cone_dims", CASES, ids=["R", "Q", "S", "RQS"])
@pytest.mark.parametrize("csr", [False, True], ids=["denseA", "csrA"])
@pytest.mark.parametrize("identity", [False, True], ids=["nt", "identity"])
def test_schur_reference_matches_the_oracle(cone_dims, csr, identity):
    n, p = 9, 2
    Q, A, G, F = _problem(cone_dims, n, p, 7, csr)
    if identity:
        F = Block([Diagonal(np.full(k, 1.0)) for _, k in cone_dims])
    Npad = 128
    K, copied, bound = KR.reference(Q, A, G, cone_dims, F, "schur", Npad, csr=csr)
    ref = schur2x2(Q, A, G, F)
    N = n + p
    np.testing.assert_allclose(np.tril(K[:N, :N]), np.tril(ref), rtol=1e-10, atol=1e-10 * np.abs(ref).max())
    # copied entries: the G block, the zero block, the padding identity, bit for bit
    assert np.array_equal(K[n:N, :n], G) and not copied[:n, :n].any() and copied[n:, :].all()
    assert np.array_equal(np.tril(K[N:, N:]), np.eye(Npad - N))
    # the bound covers the oracle's own rounding and is far below a wrong term
    low = np.tri(n, dtype=bool)
    assert np.all(np.abs(K[:n, :n] - ref[:n, :n])[low] <= bound[:n, :n][low] + 1e-12 * np.abs(ref).max())
    assert np.all(bound[:n, :n] < 1e-11 * (np.abs(Q) + np.abs(ref[:n, :n] - Q)).max())


@pytest.mark.parametrize("cone_dims", CASES, ids=["R", "Q", "S", "RQS"])
@pytest.mark.parametrize("csr", [False, True], ids=["denseA", "csrA"])
def test_full3x3_reference_matches_the_oracle(cone_dims, csr):
    n, p = 8, 3
    Q, A, G, F = _problem(cone_dims, n, p, 11, csr)
    m = A.shape[0]
    Npad = 128
    K, copied, bound = KR.reference(Q, A, G, cone_dims, F, "full3x3", Npad)
    Z = assemble3x3(Q, A, G, F)                # [Q G' -A'; G 0 0; A 0 F'F], order (y, w, v)
    perm = np.concatenate([np.arange(n + p, n + p + m), np.arange(n + p)])
    Zs = Z.copy()
    Zs[n + p:, :] *= -1.0
    ref = Zs[np.ix_(perm, perm)]
    N = n + p + m
    low = np.tri(N, dtype=bool)
    np.testing.assert_allclose(K[:N, :N][low], ref[low], rtol=1e-11, atol=1e-12 * np.abs(ref).max())
    cp = low & copied[:N, :N]
    assert np.array_equal(K[:N, :N][cp], ref[cp])                  # -A', Q, G, zeros: the oracle's bits
    assert not copied[:m, :m][np.add.outer(np.arange(m), 0) >= np.arange(m)].all()
    assert np.array_equal(np.tril(K[N:, N:]), np.eye(Npad - N))
    err = np.abs(K[:m, :m] - ref[:m, :m])
    assert np.all(err[np.tri(m, dtype=bool)] <= bound[:m, :m][np.tri(m, dtype=bool)] + 1e-13 * np.abs(ref).max())


def test_symkron_and_column_mat_vecm_match_the_oracle():
    rng = np.random.default_rng(3)
    for r in (1, 2, 5):
        k = r * (r + 1) // 2
        R = rng.standard_normal((r, r))
        from oracle.block import VecCongurance
        F = VecCongurance(R)
        np.testing.assert_allclose(KR.symkron(R @ R.T), F.square().matrix(), rtol=1e-12, atol=1e-12)
        X = rng.standard_normal((k, 4))
        Z = KR.mat_cols(X, r)
        for j in range(4):
            assert np.array_equal(Z[j], mat(X[:, j]))
        np.testing.assert_array_equal(KR.vecm_cols(Z), np.stack([vecm(Z[j]) for j in range(4)], axis=1))


def test_check_finds_a_wrong_small_entry_and_a_flipped_copy():
    cone_dims = [("R", 5), ("Q", 4)]
    Q, A, G, F = _problem(cone_dims, 6, 2, 5, False)
    K, copied, bound = KR.reference(Q, A, G, cone_dims, F, "schur", 128)
    KR.check(K.copy(), K, copied, bound)
    Kb = K.copy()
    Kb[3, 1] += 4 * bound[3, 1]
    with pytest.raises(AssertionError, match="outside the bound"):
        KR.check(Kb, K, copied, bound)
    Kb = K.copy()
    Kb[7, 2] = np.nextafter(Kb[7, 2], np.inf)                 # one ulp in the G block
    with pytest.raises(AssertionError, match="copied entries differ"):
        KR.check(Kb, K, copied, bound)
