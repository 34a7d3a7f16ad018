"""ms per `cip_conicip_lockstep` pass over problems that need the regularised LDL', with the problems leaving their group
(cip_set_lockstep_regularize(0): one serial one-problem solve each) and staying in it (1).

Workload: `count` problems of the config-5 family (cipkkt.workloads.c5_batch, dense Q of order n, A = I in CSR, one R cone),
each with `free` variables made free: their column of A removed, their row and column of Q zeroed, each pinned by a row of G
(G y = 1).  Every problem then meets an exactly zero pivot at its first free column in its first factorisation.

    python tools/lockstep_lp_timing.py [--count 64] [--n 2048] [--free 8] [--passes 3] [--modes off,on]

The structs are built once; a pass is the library call alone (warm: one untimed pass per mode first).  Prints one line per
mode: the passes in ms, their mean and spread (max - min), how many problems left / were regularised in their group, and
whether the two modes returned the same bits.  `--modes off` alone runs on a library without the switch (the parent's)."""
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


def free_variable_batch(count, n, free, seed, device):
    import scipy.sparse as sp
    from cipkkt.workloads import c5_batch
    prs = c5_batch(count=count, n=n, seed=seed, device=device)
    idx = np.arange(n - free, n)
    keep = np.arange(n - free)
    for pr in prs:
        pr["Q"][n - free:, :] = 0.0
        pr["Q"][:, n - free:] = 0.0
        pr["A"] = sp.identity(n, format="csr")[keep, :].tocsr()
        pr["b"] = np.zeros(n - free)
        pr["cone_dims"] = [("R", n - free)]
        G = np.zeros((free, n))
        G[np.arange(free), idx] = 1.0
        pr["G"], pr["d"] = G, np.ones(free)
        assert pr["A"][:, idx].nnz == 0 and not bool(pr["Q"][n - free:, :].any())      # the zero pivot is certain
    return prs


def run(prs, modes, passes, device):
    import torch
    from cipkkt import _lib as L
    from cipkkt.kkt import make_problem
    lib = L.load()
    k = len(prs)
    structs = (L.CipProblem * k)()
    keep = []
    for i, pr in enumerate(prs):
        st, kp, _ = make_problem(pr["Q"], pr["A"], pr["G"], pr["cone_dims"], "schur", device)
        structs[i] = st
        keep.append(kp)
    torch.cuda.synchronize()
    n, m, p = structs[0].n, structs[0].m, structs[0].p
    vp = C.c_void_p * k
    arr = lambda xs: vp(*[x.ctypes.data for x in xs])
    cs = [np.ascontiguousarray(pr["c"], dtype=np.float64) for pr in prs]
    bs = [np.ascontiguousarray(pr["b"], dtype=np.float64) for pr in prs]
    ds = [np.ascontiguousarray(pr["d"], dtype=np.float64) for pr in prs]
    opt = L.CipOptions(1e-6, 0.01, -1.0, -1.0, 3, 100, 0)
    results = {}
    for mode in modes:
        prev = lib.cip_set_lockstep_regularize(1 if mode == "on" else 0) if hasattr(lib, "cip_set_lockstep_regularize") else None
        try:
            times = []
            for it in range(passes + 1):
                ys, ws, vs = ([np.zeros(max(q, 1)) for _ in range(k)] for q in (n, p, m))
                res = (L.CipResult * k)()
                t0 = time.perf_counter()
                L.check(lib.cip_conicip_lockstep(k, structs, arr(cs), arr(bs), arr(ds), C.byref(opt), arr(ys), arr(ws), arr(vs), res))
                if it > 0:
                    times.append(1e3 * (time.perf_counter() - t0))
            st = (C.c_int * 3)()
            lib.cip_lockstep_stats(st)
            kreg = C.c_int(0)
            if prev is not None:
                lib.cip_lockstep_regularized(C.byref(kreg))
        finally:
            if prev is not None:
                lib.cip_set_lockstep_regularize(prev)
        statuses = sorted({int(res[i].status) for i in range(k)})
        print("switch %-3s: passes %s ms, mean %.1f, spread %.1f; left the group %d, regularised inside %d; iterations %d..%d, "
              "factorisations %d, status codes %s"
              % (mode, " ".join("%.1f" % t for t in times), np.mean(times), max(times) - min(times), st[2], kreg.value,
                 min(res[i].iter for i in range(k)), max(res[i].iter for i in range(k)), sum(res[i].n_factor for i in range(k)), statuses),
              flush=True)
        results[mode] = np.concatenate(ys + ws + vs)
    if len(results) == 2:
        a, b = results.values()
        print("same bits in both modes: %s" % bool(np.array_equal(a, b, equal_nan=True)))
    del keep


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--free", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4000)
    ap.add_argument("--modes", default="off,on")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prs = free_variable_batch(a.count, a.n, a.free, a.seed, dev)
    print("%d problems, n = %d, %d free variables each" % (a.count, a.n, a.free), flush=True)
    run(prs, a.modes.split(","), a.passes, dev)


if __name__ == "__main__":
    main()
