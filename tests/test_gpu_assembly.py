"""Entrywise parity of the device KKT assembly (csrc/assemble.hip, the Schur formation of csrc/gemm_f64.hip, the scalings
of A' in csrc/cones.hip and csrc/sdp*.hip) with a plain fp64 reference (tests/_kkt_ref.py), on every kernel path.

cip_set_scaling_packed -> cip_assemble_only -> cip_get_kkt_matrix, then on the lower triangle: copied entries (Q, G, -A',
zeros, the padding identity) bit for bit, computed entries (the Schur block, the -F'F blocks) within an entrywise rounding
bound.  The shapes are chosen by the dispatch rules of cip_syrk_split / syrk_split_128 (gemm_f64.hip; npad = n rounded
up to 128, the reduction length mpad = m rounded up to 16) and copy_lower_vectorisable (assemble.hip).  The scalings are
Nesterov-Todd scalings of iterate pairs near the edge of the cones, and the identity.

Also here: the values of the static regularisation (k_rowmax_lower, k_regularize_rows), bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _kkt_ref as KR
from oracle.block import Block, Diagonal
from oracle.cones import vecm
from oracle.conicip import make_cone_ops

pytestmark = pytest.mark.gpu


def _hard_iterates(cone_dims, rng):
    """a valid interior pair (v, s) whose Nesterov-Todd scaling is hard: R entries of d = sqrt(s / v) over 1e-6 .. 1e6, Q
    iterates with x0 - |x1| = 1e-6 x0, S iterates with condition number 1e6"""
    vs, ss = [], []
    for t, k in cone_dims:
        if t == "R":
            e = rng.uniform(-6.0, 6.0, k)
            e[:min(k, 2)] = (-6.0, 6.0)[:min(k, 2)]
            vs.append(10.0 ** -e * (0.5 + rng.random(k)))
            ss.append(10.0 ** e * (0.5 + rng.random(k)))
            continue
        for out in (vs, ss):
            if t == "Q":
                x = rng.standard_normal(k)
                x[0] = np.linalg.norm(x[1:]) / (1.0 - 1e-6) if k > 1 else 0.5 + rng.random()
                out.append(x)
            else:
                r = KR._order(k)
                U, _ = np.linalg.qr(rng.standard_normal((r, r)))
                lam = np.logspace(-3.0, 3.0, r) if r > 1 else np.array([0.5 + rng.random()])
                M = (U * rng.permutation(lam)) @ U.T
                out.append(vecm(0.5 * (M + M.T)))
    return np.concatenate(vs), np.concatenate(ss)


def _csr(m, n, density, rng):
    A = rng.standard_normal((m, n)) * (rng.random((m, n)) < density)
    A[np.arange(m), rng.integers(0, n, m)] = 1.0              # no empty row
    return sp.csr_matrix(A)


def _gram_dev(X):
    t = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    return (t.T @ t).cpu().numpy()


def _q_boxqp(n):
    from cipkkt.workloads import c2_dense_qp
    Q, _ = c2_dense_qp(n, 4000)
    return np.asarray(Q)


# (route, A, n, p, cone_dims): each row names the forms it reaches
CASES = {
    # npad 1024 = 36 128-tiles, 144 quarter-tile workgroups < 640, mpad 4112 >= 4096: split-K 64, ceil(1280 / 144) = 9 slices
    # of 464 rows, the last one 400 (uneven); R items of <= 2048 rows: three chunks in k_scale_At_r
    "splitk64_uneven": ("schur", "dense", 1000, 0, [("R", 4100)]),
    # odd n, npad 1280 = 55 tiles <= 64 and mpad 16400 >= 16384: split-K 128 (512 / 55 = 9 slices); R chunks of 2048 rows,
    # one Q cone of 390 (k_scale_At_qbig), the p rows through k_fill_rest
    "splitk128_odd_n": ("schur", "dense", 1153, 3, [("R", 9000), ("Q", 390), ("R", 7000)]),
    # npad 1536 = 78 tiles > 64: split-K 64 although mpad 20000 >= 16384; 312 workgroups -> 5 slices
    "splitk64_many_tiles": ("schur", "dense", 1536, 0, [("R", 19000), ("Q", 1000)]),
    # npad 2304 = 171 tiles, 684 workgroups >= 640: no split, k_syrkq_64 over the whole lower triangle.  Runs of Q cones of
    # dimension <= 64 are packed in k_scale_At with the next power of two of the run's largest cone as the pack width
    # (api.hip): [1] width 1, [2, 3] width 4, [64] width 64 (the run ends at the 65), [2] width 2; the cones of 65 and 129
    # get a workgroup each in k_scale_At_qbig
    "syrkq_no_split": ("schur", "dense", 2177, 5,
                       [("Q", 1), ("R", 50), ("Q", 2), ("Q", 3), ("R", 20), ("Q", 64), ("Q", 65), ("Q", 2), ("Q", 129),
                        ("R", 700)]),
    # cip_sdp_scale_At on a dense A': the small S path (order 8) and the large one (order 133), beside R cones.  npad 256 =
    # 3 tiles, 12 workgroups, mpad 9008 >= 4096 but < 16384: split-K 64 with 16 slices (the cap) of 576 rows, the last 368
    "dense_sdp_small_large": ("schur", "dense", 256, 2, [("R", 40), ("S", 36), ("S", 8911), ("R", 13)]),
    # CSR A: rows of ~130 non-zeros (the lane loop of k_schur_rows), 20 Q cones (nqpad 32: the rank-nq update over two
    # k-tiles), odd n, p > 0, k_schur_qcols
    "csr_many_q": ("schur", "csr", 301, 4, [("R", 60)] + [("Q", 5)] * 12 + [("Q", 17), ("R", 9)] + [("Q", 2)] * 6 + [("Q", 70)]),
    # CSR A, a single Q cone (nq = 1, nqpad 16)
    "csr_one_q": ("schur", "csr", 200, 0, [("Q", 150), ("R", 33)]),
    # CSR A with S cones: k_scatter_AtS, cip_sdp_scale_At on AtS (small and large S), the WtS GEMM; plus Q and R rows
    "csr_sdp": ("schur", "csr", 190, 3, [("S", 36), ("R", 20), ("S", 8911), ("Q", 6)]),
    # the box-QP family (CSR A = I, R cone): the eager K (assemble_only never takes the lazy copy)
    "boxqp_2048": ("schur", "identity", 2048, 0, [("R", 2048)]),
    # full 3x3, dense A, m = 541 odd and n = 256 even: the odd row offset r0 = m alone sends the copy of Q to the scalar
    # k_copy_block_lower; k_copy_block of -A' (at row m) and G (at row m + n), k_fill_ftf_qbig with k = 300 > 128 (its
    # gridDim.y loop) and k = 65, packed Q cones in k_fill_ftf, p > 0, k_pad_identity
    "full_dense_odd_m": ("full3x3", "dense", 256, 5, [("R", 100), ("Q", 300), ("Q", 3), ("Q", 8), ("Q", 64), ("Q", 65), ("Q", 1)]),
    # full 3x3, CSR A, even m and n: k_scatter_negA, the 16-byte k_copy_block_lower_v, k_sdp_fill_ftf for order 8 and 133
    "full_csr_sdp": ("full3x3", "csr", 300, 3, [("S", 36), ("R", 53), ("S", 8911)]),
    # a large S cone above padded order 256 (order 257 -> rp = 512): cip_sdp_large_scale_At on the batched-64 GEMM path, the
    # second product with the lower tiles selected, then k_lg_vecm_cols at rp = 512.  npad 128 = 1 tile and mpad 33168 >=
    # 16384: split-K 128 with 16 slices (the cap) of 2080 rows, the last one 1968
    "dense_sdp_257": ("schur", "dense", 40, 2, [("R", 10), ("S", 257 * 258 // 2)]),
    # the same cones from a CSR A: k_scatter_AtS, then the same scaling at rp = 512
    "csr_sdp_257": ("schur", "csr", 40, 2, [("R", 10), ("S", 257 * 258 // 2)]),
    # order 513 -> rp = 1024: cip_sdp_large_scale_At on the batched-64 path with the lower tiles selected and k_lg_vecm_cols at
    # rp = 1024, the S cone first (row offset 0).  mpad 131856: split-K 128, 16 slices of 8256 rows, the last one 8016
    "dense_sdp_513": ("schur", "dense", 12, 0, [("S", 513 * 514 // 2), ("R", 7)]),
}


def _syrk_form(n, m):
    """(form, slices) of the Schur formation: the rules of cip_syrk_split / syrk_split_128 (gemm_f64.hip) at their defaults"""
    npad, mpad = -(-n // 128) * 128, -(-max(m, 1) // 16) * 16
    tm = npad // 128
    t128 = tm * (tm + 1) // 2
    wgs = 4 * t128
    form, k = "syrkq_64", 1
    if wgs < 640 and mpad >= 4096:
        if t128 <= 64 and mpad >= 16384:
            form, k = "splitk_128", max(1, min(16, 512 // (wgs // 4)))
        else:
            form, k = "splitk_64", min(16, -(-1280 // wgs))
    ln = -(-(-(-mpad // k)) // 16) * 16
    return form, -(-mpad // ln)


# what the comments of CASES claim, kept in step with the dispatch rules
FORMS = {"splitk64_uneven": ("splitk_64", 9), "splitk128_odd_n": ("splitk_128", 9), "splitk64_many_tiles": ("splitk_64", 5),
         "syrkq_no_split": ("syrkq_64", 1), "dense_sdp_small_large": ("splitk_64", 16),
         "dense_sdp_257": ("splitk_128", 16), "csr_sdp_257": ("splitk_128", 16), "dense_sdp_513": ("splitk_128", 16)}


def test_case_table_reaches_the_named_forms():
    for name, (route, akind, n, p, cone_dims) in CASES.items():
        m = sum(k for _, k in cone_dims)
        if name in FORMS:
            assert _syrk_form(n, m) == FORMS[name], name
        if route == "full3x3":
            # copy_lower_vectorisable (assemble.hip): the copy of Q at row offset m is 16-byte only for even n and m
            assert (n % 2 == 0 and m % 2 == 0) == (name == "full_csr_sdp"), name
    _, _, n, _, cone_dims = CASES["full_dense_odd_m"]
    assert n % 2 == 0 and sum(k for _, k in cone_dims) % 2 == 1      # the odd offset alone picks the scalar copy


def _build(name):
    import cipkkt
    route, akind, n, p, cone_dims = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    m = sum(k for _, k in cone_dims)
    if akind == "identity":
        Q = _q_boxqp(n)
        A = sp.identity(n, format="csr")
    else:
        M = rng.standard_normal((n, n))
        Q = M @ M.T / n + 0.5 * np.eye(n)
        A = rng.standard_normal((m, n)) if akind == "dense" else _csr(m, n, 0.4 if n > 250 else 0.15, rng)
    G = rng.standard_normal((p, n)) if p else None
    ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route)
    return ks, Q, A, G, cone_dims, route, akind, rng


def _scalings(cone_dims, rng):
    _, nt_scaling, _, _ = make_cone_ops(cone_dims)
    yield "nt-hard", nt_scaling(*_hard_iterates(cone_dims, rng))
    yield "identity", Block([Diagonal(np.ones(k)) for _, k in cone_dims])


@pytest.mark.parametrize("name", list(CASES))
def test_assembly_matches_the_reference_entrywise(name):
    ks, Q, A, G, cone_dims, route, akind, rng = _build(name)
    if name == "csr_many_q":
        assert np.diff(A.indptr).max() > 64
    try:
        for label, F in _scalings(cone_dims, rng):
            ks.set_scaling_packed(ks.pack_scaling(F, F.inv_adjoint()))
            ks.assemble_only()
            Kd = ks.kkt_matrix()
            K, copied, bound = KR.reference(Q, A, G, cone_dims, F, route, ks.Npad, csr=akind != "dense", gram=_gram_dev)
            try:
                KR.check(Kd, K, copied, bound)
            except AssertionError as e:
                raise AssertionError("%s, %s scaling: %s" % (name, label, e)) from None
            del Kd, K, copied, bound
    finally:
        ks.close()


def _expected_regularised(K0, N, p0, p1, rel):
    """K_ii + s_i rel max_j |K_ij| over the full symmetric row i < N (stored row part j <= i, column part below the
    diagonal), s_i = +1 on [p0, p1), -1 elsewhere; everything else unchanged"""
    L = np.abs(np.tril(K0[:N, :N]))
    mx = np.maximum(L.max(axis=1), L.max(axis=0))
    out = K0.copy()
    i = np.arange(N)
    delta = rel * mx
    out[i, i] = K0[i, i] + np.where((i >= p0) & (i < p1), delta, -delta)
    return out


@pytest.mark.parametrize("route", ["schur", "full3x3"])
def test_regularisation_values_bit_for_bit(route):
    """cip_set_regularization(h, rel, 0) -> the next assembly adds s_i rel max_j |K_ij| to K_ii: fmax is exact and there
    is one multiply and one add, so the expected matrix, computed on the host from the device's unregularised K, matches
    bit for bit (padding included)"""
    import cipkkt
    rng = np.random.default_rng(17)
    if route == "schur":
        n, p = 300, 4
        cone_dims = [("R", 150), ("Q", 40), ("Q", 3), ("Q", 130), ("Q", 8)]
        m = sum(k for _, k in cone_dims)
        A = rng.standard_normal((m, n))
    else:
        n, p = 120, 3
        cone_dims = [("R", 90), ("Q", 30), ("Q", 4), ("S", 10)]
        m = sum(k for _, k in cone_dims)
        A = _csr(m, n, 0.2, rng)
    M = rng.standard_normal((n, n))
    Q = M @ M.T / n + 0.5 * np.eye(n)
    G = rng.standard_normal((p, n))
    ks = cipkkt.KKTSystem(Q, A, G, cone_dims, route=route)
    try:
        _, nt_scaling, _, _ = make_cone_ops(cone_dims)
        F = nt_scaling(*_hard_iterates(cone_dims, rng))
        ks.set_scaling_packed(ks.pack_scaling(F, F.inv_adjoint()))
        ks.assemble_only()
        K0 = ks.kkt_matrix()
        N = ks.N
        p0, p1 = (0, n) if route == "schur" else (m, m + n)
        lib = ks.lib
        for rel in (1e-13, 1e-6):
            assert lib.cip_set_regularization(ks.h, rel, 0) == 0
            ks.assemble_only()
            K1 = ks.kkt_matrix()
            exp = _expected_regularised(K0, N, p0, p1, rel)
            low = np.tri(ks.Npad, dtype=bool)
            bad = low & (K1.view(np.int64) != exp.view(np.int64))
            assert not bad.any(), (rel, np.argwhere(bad)[:5].tolist())
            d = np.arange(N)
            assert np.all(K1[d, d] != K0[d, d]), rel         # every row moved (no zero row maximum here)
        assert lib.cip_set_regularization(ks.h, 0.0, 0) == 0
        ks.assemble_only()
        assert np.array_equal(np.tril(ks.kkt_matrix()).view(np.int64), np.tril(K0).view(np.int64))
    finally:
        ks.close()
