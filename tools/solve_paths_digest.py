"""One SHA-256 per line over the raw fp64 bytes of what every path of the Newton-step solves (csrc/solve.hip) writes, and the
handles' n_solve counters: compare two builds line by line,

    CIPKKT_LIB=/path/to/libcipkkt.so python tools/solve_paths_digest.py

one process per library (and once more per library with CIP_GRAPH=1: the recorded sweeps).  Asserts nothing.  Inputs come from
the portable generator of cipkkt/workloads.py, element-wise only (no host BLAS product).  All orders are N <= 256.
  handles          Schur and literal 3x3 route; dense and CSR A; dense and CSR Q; p = 0; m = 0; an all-R cone set (the fused
                   solve4x4 on the Schur route) and a mixed R / Q / S one (the generic solve4x4); Npad = 256 under
                   cip_set_solve_block_max(128) (two solve blocks).  Each on a plain factor and after
                   cip_set_regularization(1e-10, 0) (the refined solves).
  per handle       solve3x3 / solve2x2 (Schur route), device and host pointers; solve4x4 with dz apart from r and dz == r; every
                   *_many* entry point at 1, 2, 64 and 65 columns; n_solve at the end.
  lock-step        two groups of three problems of which one needs the regularised factor, built by tests/
                   test_gpu_lockstep_regularized.py's own functions (all R cones: the fused solve4x4 under a split mask; with a Q
                   cone: one refined solve3x3 for the group; these inputs alone use numpy's generator and a host product): the
                   solutions and (Iter, n_factor, n_solve)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + '/conicip.jl_amd'): sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch, cipkkt
from cipkkt import _lib as L
from cipkkt.batch import _solve_problems_native
from cipkkt.workloads import randn_np as _randn_np

F64 = dict(dtype=torch.float64, device="cuda")
lib = L.load()


def randn_np(seed, *shape):
    return _randn_np(seed, *shape) if np.prod(shape) else np.zeros(shape)


def line(label, *xs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for x in xs:
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        h.update(np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes())
    print("%s  %s" % (h.hexdigest(), label), flush=True)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), **F64)


def nan(*shape):
    return torch.full(shape, float("nan"), **F64)


def sym_pd(n, seed, band=None):
    """symmetric, eigenvalues within 2 +- 1 or so: a scaled Wigner matrix + 2 I (band: entries within that distance of the diagonal)"""
    R = randn_np(seed, n, n)
    Q = (R + R.T) / (2.0 * np.sqrt(2.0 * n))
    if band is not None:
        i = np.arange(n)
        Q = Q * (np.abs(i[:, None] - i[None, :]) <= band) / 2.0
    return Q + 2.0 * np.eye(n)


def vecm(Z):
    iu = np.triu_indices(Z.shape[0])
    x = Z[iu].copy()
    x[iu[0] != iu[1]] *= np.sqrt(2.0)
    return x


def iterate(cone_dims, seed):
    """(v, s) inside the cones: R entries over a few decades with v s ~ 1e-3, Q points 10 % inside, S points sym_pd"""
    vs, ss = [], []
    for i, (t, k) in enumerate(cone_dims):
        g, g2 = randn_np(seed + 7 * i, k), randn_np(seed + 7 * i + 3, k)
        if t == "R":
            v = 10.0 ** g
            vs.append(v); ss.append(1e-3 / v * (1.0 + 0.3 * np.tanh(g2)))
        elif t == "Q":
            for out, x in ((vs, g), (ss, g2)):
                x = x.copy()
                x[0] = 1.1 * np.sqrt(np.sum(x[1:] ** 2)) + 0.1
                out.append(x)
        else:
            r = int(round((np.sqrt(1.0 + 8.0 * k) - 1.0) / 2.0))
            vs.append(vecm(sym_pd(r, seed + 7 * i))); ss.append(vecm(sym_pd(r, seed + 7 * i + 3)))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    return cat(vs), cat(ss)


ALL_R = [("R", 60), ("R", 50)]
MIXED = [("R", 16), ("Q", 5), ("S", 6), ("Q", 65), ("R", 4)]
# label -> (n, p, cones, route, CSR A, CSR Q, solve-block limit or None)
HANDLES = {
    "schur all-R dense": (100, 7, ALL_R, "schur", False, False, None),
    "schur all-R csr A": (100, 7, ALL_R, "schur", True, False, None),
    "schur all-R csr Q": (100, 7, ALL_R, "schur", False, True, None),
    "schur all-R csr A csr Q p = 0": (100, 0, ALL_R, "schur", True, True, None),
    "schur mixed dense": (96, 8, MIXED, "schur", False, False, None),
    "schur mixed csr A": (96, 8, MIXED, "schur", True, False, None),
    "schur mixed csr Q": (96, 8, MIXED, "schur", False, True, None),
    "full all-R dense": (100, 7, ALL_R, "full3x3", False, False, None),
    "full mixed dense": (96, 8, MIXED, "full3x3", False, False, None),
    "full mixed csr A csr Q": (96, 8, MIXED, "full3x3", True, True, None),
    "full mixed p = 0": (96, 0, MIXED, "full3x3", False, False, None),
    "schur m = 0": (50, 6, [], "schur", False, False, None),
    "full m = 0": (50, 6, [], "full3x3", False, False, None),
    "schur all-R Npad 256, solve blocks of 128": (200, 7, [("R", 130)], "schur", False, False, 128),
    "schur all-R Npad 256": (200, 7, [("R", 130)], "schur", False, False, None),
    "full mixed Npad 256, solve blocks of 128": (150, 6, [("R", 40), ("Q", 9), ("S", 6)], "full3x3", True, False, 128),
}


def handle_case(label, spec, rel, seed):
    n, p, cone_dims, route, csr_a, csr_q, block = spec
    m = sum(k for _, k in cone_dims)
    tag = "%s, %s" % (label, "regularised" if rel else "plain")
    Q = sym_pd(n, seed, band=3 if csr_q else None)
    A = randn_np(seed + 1, m, n) / np.sqrt(n) if m else None
    if m and csr_a:
        keep = np.abs(randn_np(seed + 2, m, n)) > 1.2
        keep[np.arange(m), np.arange(m) % n] = True
        A = sp.csr_matrix(A * keep)
    G = randn_np(seed + 3, p, n) if p else None
    prev = lib.cip_set_solve_block_max(block) if block else None
    ks = cipkkt.KKTSystem(sp.csr_matrix(Q) if csr_q else Q, A, G, cone_dims, route=route, sparse_q=csr_q)
    try:
        if rel:
            L.check(lib.cip_set_regularization(ks.h, rel, 0))
        lam = nan(m)
        if m:
            v, s = iterate(cone_dims, seed + 10)
            ks.set_scaling_from_iterate(dev(v), dev(s), lam)
        ks.factor()
        x, y, z = randn_np(seed + 20, n), randn_np(seed + 21, p), randn_np(seed + 22, m)
        a, b, c = nan(n), nan(p), nan(m)
        ks.solve3x3_dev(dev(x), dev(y), dev(z), a, b, c)
        line("%s: solve3x3_dev" % tag, a, b, c)
        line("%s: solve3x3" % tag, *ks.solve3x3(x, y, z))
        if route == "schur":
            dy, dw = nan(n), nan(p)
            ks.solve2x2_dev(dev(x), dev(y), dy, dw)
            line("%s: solve2x2_dev" % tag, dy, dw)
            line("%s: solve2x2" % tag, *ks.solve2x2(x, y))
        r = dev(randn_np(seed + 23, n + p + 2 * m))
        dz = nan(n + p + 2 * m)
        ks.solve4x4_dev(lam, r, dz)
        line("%s: solve4x4_dev" % tag, dz)
        ks.solve4x4_dev(lam, r, r)
        line("%s: solve4x4_dev, dz == r" % tag, r)
        for k in (1, 2, 64, 65):
            X, Y, Z = randn_np(seed + 30 + k, k, n), randn_np(seed + 130 + k, k, p), randn_np(seed + 230 + k, k, m)
            Ao, Bo, Co = nan(k, n), nan(k, p), nan(k, m)
            ks.solve3x3_many_dev(dev(X), dev(Y), dev(Z), Ao, Bo, Co)
            line("%s: solve3x3_many_dev, %d columns" % (tag, k), Ao, Bo, Co)
            line("%s: solve3x3_many, %d columns" % (tag, k), *[o.T for o in ks.solve3x3_many(X.T, Y.T, Z.T)])
            if route == "schur":
                DY, DW = nan(k, n), nan(k, p)
                ks.solve2x2_many_dev(dev(X), dev(Y), DY, DW)
                line("%s: solve2x2_many_dev, %d columns" % (tag, k), DY, DW)
                line("%s: solve2x2_many, %d columns" % (tag, k), *[o.T for o in ks.solve2x2_many(X.T, Y.T)])
        print("%s: n_solve %d, reg_rel %g" % (tag, ks.stats()["n_solve"], ks.health()["reg_rel"]), flush=True)
    finally:
        ks.close()
        if prev is not None:
            lib.cip_set_solve_block_max(prev)


def lockstep_group(label, prs):
    sols = _solve_problems_native(prs, torch.device("cuda:0"), 1, "lockstep", keep_regularized=True)
    for k, s in enumerate(sols):
        line("%s, problem %d: y, w, v" % (label, k), s.y, s.w, s.v)
        print("%s, problem %d: %s, (Iter, n_factor, n_solve) = (%d, %d, %d)" % (label, k, s.status, s.Iter, s.n_factor, s.n_solve), flush=True)


for i, (label, spec) in enumerate(HANDLES.items()):
    for rel in (0.0, 1e-10):
        handle_case(label, spec, rel, 1000 * (i + 1))
# the mixed groups of tests/test_gpu_lockstep_regularized.py, by its own builders: problems 1 .. 3 of test_mixed_group_keeps_its_lps (a
# definite QP, an LP whose first factorisation meets a zero pivot, a definite QP) and the first three of the "schur-qcone" variant of
# test_mixed_group_through_the_generic_solve (QP, LP, QP with a Q cone)
sys.path.insert(0, ROOT + "/tests")
import test_gpu_lockstep_regularized as TLR
lockstep_group("lock-step, all R", TLR._six_of_the_ejection_test()[1:4])
rng = np.random.default_rng(15)
lockstep_group("lock-step, R + Q", [(TLR._lp if k % 2 else TLR._definite_qp)(16, rng, q_cone=True) for k in range(3)])
