"""ms per `cip_conicip_mixed` pass over box QPs whose CSR Q differ in their numbers of non-zeros, with the nnz as part of the shape
(cip_set_lockstep_ragged(0), the default: every problem a bin of its own, the thread pool solves them) and without it (1: one
lock-step bin, run as the library's groups).

Workload: `count` problems of order n, min 1/2 y'Qy - c'y over y >= -1 (A = I in CSR, one R cone, b = -1).  Q is a random
symmetric matrix in CSR, diagonally dominant (positive definite), with a density drawn per problem from [dmin, dmax]: rows of
about 10 to 40 entries at n = 2048, the wave-per-row mat-vec form, another nnz for every problem.

    python tools/lockstep_ragged_timing.py [--counts 16,64] [--n 2048] [--dmin 0.005] [--dmax 0.02] [--passes 5] [--in-flight 4]

The structs are built once; a pass is the library call alone, on a host clock around the synchronous call.  One untimed pass per
setting first, then `passes` timed ones per setting, the two settings ALTERNATING.  Prints per setting: the passes in ms, their
median and spread (max - min), the groups formed, and whether every problem ended Optimal; then how far the two settings'
solutions are apart (the thread pool's handles use another solve block: rounding)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "conicip.jl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def ragged_box_qps(count, n, dmin, dmax, seed):
    import scipy.sparse as sp
    prs = []
    for i in range(count):
        rng = np.random.default_rng(seed + i)
        density = rng.uniform(dmin, dmax)
        B = sp.triu(sp.random(n, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csr"), 1)
        S = (B + B.T).tocsr()
        Q = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 0.1)).tocsr()
        Q.eliminate_zeros()
        Q.sort_indices()
        prs.append(dict(Q=Q, c=rng.standard_normal(n), A=sp.identity(n, format="csr"), b=-np.ones(n), cone_dims=[("R", n)]))
    return prs


def run(prs, passes, in_flight, device):
    import torch
    from cipkkt import _lib as L
    from cipkkt.kkt import make_problem
    lib = L.load()
    k = len(prs)
    structs = (L.CipProblem * k)()
    keep = []
    for i, pr in enumerate(prs):
        st, kp, _ = make_problem(pr["Q"], pr["A"], None, pr["cone_dims"], "schur", device, sparse_q=True)
        structs[i] = st
        keep.append(kp)
    torch.cuda.synchronize()
    n = structs[0].n
    vp = C.c_void_p * k
    arr = lambda xs: vp(*[x.ctypes.data for x in xs])
    cs = [np.ascontiguousarray(pr["c"], dtype=np.float64) for pr in prs]
    bs = [np.ascontiguousarray(pr["b"], dtype=np.float64) for pr in prs]
    zs = [np.zeros(1) for _ in prs]
    opt = L.CipOptions(1e-6, 0.01, -1.0, -1.0, 3, 100, 0)
    times = {0: [], 1: []}
    last = {}
    prev = lib.cip_set_lockstep_ragged(-1)
    try:
        for it in range(passes + 1):
            for on in (0, 1):
                lib.cip_set_lockstep_ragged(on)
                ys, vs = ([np.zeros(n) for _ in range(k)] for _ in range(2))
                res = (L.CipResult * k)()
                t0 = time.perf_counter()
                L.check(lib.cip_conicip_mixed(k, structs, arr(cs), arr(bs), arr(zs), C.byref(opt), arr(ys), arr(zs), arr(vs), res, int(in_flight)))
                t = 1e3 * (time.perf_counter() - t0)
                if it > 0:
                    times[on].append(t)
                st = (C.c_int * 3)()
                lib.cip_lockstep_stats(st)
                last[on] = (tuple(st), [int(res[i].status) for i in range(k)], [int(res[i].iter) for i in range(k)], np.concatenate(ys + vs))
    finally:
        lib.cip_set_lockstep_ragged(prev)
    for on in (0, 1):
        st, status, iters, _ = last[on]
        t = times[on]
        print("%3d problems, switch %d: passes %s ms, median %.1f, spread %.1f; %d group(s) of %d problem(s), %d left; iterations %d..%d, all Optimal: %s"
              % (k, on, " ".join("%.1f" % x for x in t), np.median(t), max(t) - min(t), st[0], st[1], st[2], min(iters), max(iters),
                 all(L.STATUS_NAMES[s] == "Optimal" for s in status)), flush=True)
    a, b = last[0][3], last[1][3]
    print("%3d problems: thread pool / lock-step medians %.1f / %.1f ms (x %.2f); largest |difference| of the solutions %.3g (relative to %.3g)"
          % (k, np.median(times[0]), np.median(times[1]), np.median(times[0]) / np.median(times[1]), np.abs(a - b).max(), np.abs(a).max()), flush=True)
    del keep


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="16,64")
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--dmin", type=float, default=0.005)
    ap.add_argument("--dmax", type=float, default=0.02)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--seed", type=int, default=7000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for count in (int(x) for x in a.counts.split(",")):
        prs = ragged_box_qps(count, a.n, a.dmin, a.dmax, a.seed)
        nnz = [pr["Q"].nnz for pr in prs]
        print("%d problems, n = %d, nnz(Q) %d..%d (%d distinct)" % (count, a.n, min(nnz), max(nnz), len(set(nnz))), flush=True)
        run(prs, a.passes, a.in_flight, dev)


if __name__ == "__main__":
    main()
