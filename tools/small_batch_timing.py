"""Batches of small dense QPs: problems per second of cip_conicip_small (one workgroup per problem) and, in the same process on
the same problems, of cip_conicip_mixed (the lock-step groups: the library's capability before the small path) -- alternated,
best of three.  The wall time of both INCLUDES the upload of the problem matrices (host pointers) and the download of the results.

    python tools/small_batch_timing.py [--n 16 64 120] [--count 64 1024 8192] [--reps 3] [--out FILE]

Problems: Q = M'M/n (cipkkt/workloads.py: c2_dense_qp), m = 2n rows of one R cone with A ~ 0.3 N(0,1) and slacks in (0.5, 1.5) at
y = 1, p = 0 and p = min(n/8, 128 - n) equalities (n + p <= 128 is the path's limit) G ~ N(0,1), d = G 1; 64 distinct instances per shape (seeds 7000 + i), instance i mod 64 at
position i.  Also printed: the time of one k_small_step launch (all live problems of an iteration) from HIP events.
Prints a markdown table; --out also writes the rows as JSON."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "conicip.jl_amd")]
DISTINCT = 64


def instance(n, p, seed):
    from cipkkt.workloads import c2_dense_qp, randn_np, uniform_np
    Q, c = c2_dense_qp(n, seed)
    m = 2 * n
    A = 0.3 * randn_np(seed + 17, m, n)
    b = A @ np.ones(n) - (uniform_np(seed + 29, m) + 0.5)
    G = randn_np(seed + 31, p, n) if p else None
    d = G @ np.ones(n) if p else None
    return Q, c, A, b, [("R", m)], G, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16, 64, 120])
    ap.add_argument("--count", type=int, nargs="+", default=[64, 1024, 8192])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from cipkkt import _lib as L, batch
    lib = L.load()
    opt = L.CipOptions(1e-6, 0.01, -1.0, -1.0, 3, 100, 0)
    rows = []
    print("wall time includes the upload of the matrices and the download of the results; best of %d, alternated" % args.reps)
    print("| n | m | p | count | small: problems/s | mixed: problems/s | small / mixed | iterations (max) | k_small_step ms per iteration | handed over |")
    print("|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for n in args.n:
        for p in (0, min(n // 8, 128 - n)):
            m = 2 * n
            base = [instance(n, p, 7000 + i) for i in range(DISTINCT)]
            structs0, keep = [], []
            for pr in base:
                st, kp = batch._host_problem(pr[0], pr[2], pr[5], pr[4])
                structs0.append(st)
                keep.append(kp)
            for count in args.count:
                vp = C.c_void_p * count
                structs = (L.CipProblem * count)(*[structs0[i % DISTINCT] for i in range(count)])
                hold = [[np.ascontiguousarray(pr[k]) if pr[k] is not None else np.zeros(1) for pr in base] for k in (1, 3, 6)]
                ins = [vp(*[hold[j][i % DISTINCT].ctypes.data for i in range(count)]) for j in range(3)]
                outs = {}
                for who in ("small", "mixed"):
                    bufs = [np.zeros((count, max(x, 1))) for x in (n, p, m)]
                    outs[who] = (bufs, [vp(*[bufs[j][i].ctypes.data for i in range(count)]) for j in range(3)], (L.CipResult * count)())
                best = {"small": np.inf, "mixed": np.inf}
                step_ms, handed = None, 0
                lib.cip_small_step_time(1, None)
                for rep in range(args.reps + 1):                      # the first round warms both paths up (module load, arenas)
                    for who in ("small", "mixed"):
                        bufs, ptrs, res = outs[who]
                        t0 = time.perf_counter()
                        if who == "small":
                            L.check(lib.cip_conicip_small(count, structs, ins[0], ins[1], ins[2], C.byref(opt), ptrs[0], ptrs[1], ptrs[2], res))
                        else:
                            L.check(lib.cip_conicip_mixed(count, structs, ins[0], ins[1], ins[2], C.byref(opt), ptrs[0], ptrs[1], ptrs[2], res, 4))
                        dt = time.perf_counter() - t0
                        if rep > 0:
                            best[who] = min(best[who], dt)
                        if who == "small":
                            t2 = (C.c_double * 2)()
                            lib.cip_small_step_time(-1, t2)
                            step_ms = t2[1] / max(t2[0], 1.0)
                            handed = batch.small_stats()["handed_over"]
                lib.cip_small_step_time(0, None)
                rs, rm = outs["small"][2], outs["mixed"][2]
                same = all(rs[i].status == rm[i].status and rs[i].iter == rm[i].iter for i in range(count))
                dy = max(np.linalg.norm(outs["small"][0][0][i] - outs["mixed"][0][0][i]) / (1 + np.linalg.norm(outs["mixed"][0][0][i])) for i in range(min(count, DISTINCT)))
                row = dict(n=n, m=m, p=p, count=count, small_pps=count / best["small"], mixed_pps=count / best["mixed"],
                           iters_max=max(r.iter for r in rs), step_ms=step_ms, handed_over=handed, same_status_and_iterations=same, max_rel_dy=dy)
                rows.append(row)
                print("| %d | %d | %d | %d | %.0f | %.0f | %.1f | %d | %.3f | %d |%s" % (
                    n, m, p, count, row["small_pps"], row["mixed_pps"], row["small_pps"] / row["mixed_pps"], row["iters_max"], step_ms, handed,
                    "" if same and dy < 1e-6 else " (paths disagree: same %s, dy %.1e)" % (same, dy)), flush=True)
                if args.out:
                    with open(args.out, "w") as f:
                        json.dump(rows, f, indent=1)
            batch.release_cached_memory()


if __name__ == "__main__":
    main()
