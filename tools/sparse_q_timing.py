"""Dense Q against sparse_q=True (CIP_FLAG_Q_CSR) on the same build: what level 1 costs, what a Newton step costs, what the
handle holds, what one Q mat-vec costs.  Prints one JSON document.

    python tools/sparse_q_timing.py                  # the two configurations below, three repeats per form
    python tools/sparse_q_timing.py --rows 4096      # the mat-vec alone on banded matrices of 1 .. 2048 entries per row
                                                     # (with CIP_QSPMV_WAVE_MIN=0 / =1000000 in the environment: one wave per
                                                     # row / one thread per row whatever the row length -- the threshold's data)

Configurations: the n = 8192 box QP with Q = I (A = I in CSR, one R cone) and cipkkt.workloads.c3_socp (Q = I, 512 Q cones,
dense A, 512 equalities).  Per form and repeat:
  create_s   wall time of KKTSystem(...) from host data
  step_ms    ms per Newton step (NT scaling + factor + 2 x solve4x4) over 20 steps after 3 warm-up steps, HIP events
  bytes      device memory held by the handle (free device memory before / after level 1, torch's cache emptied)
  gemv_ms    ms of one gemv(CIP_MAT_Q), mean of 50 behind 5 warm-up calls, HIP events"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "conicip.jl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cipkkt                                   # noqa: E402
from cipkkt import _lib as L                    # noqa: E402
from cipkkt import workloads as W               # noqa: E402


def _timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _interior(cone_dims, rng):
    xs = []
    for t, k in cone_dims:
        if t == "R":
            xs.append(rng.random(k) + 0.5)
        else:
            x = rng.standard_normal(k)
            x[0] = np.linalg.norm(x[1:]) + 1.0
            xs.append(x)
    return np.concatenate(xs)


def measure(Q, A, G, cone_dims, sparse_q, seed=0):
    rng = np.random.default_rng(seed)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    ks = cipkkt.KKTSystem(Q, A, G, cone_dims, sparse_q=sparse_q)
    torch.cuda.synchronize()
    create_s = time.perf_counter() - t0
    torch.cuda.empty_cache()
    held = free0 - torch.cuda.mem_get_info()[0]
    try:
        n, m, p = ks.n, ks.m, ks.p
        dev = dict(dtype=torch.float64, device=ks.device)
        v, s = (torch.from_numpy(_interior(cone_dims, rng)).to(ks.device) for _ in range(2))
        lam = torch.empty(m, **dev)
        r = torch.from_numpy(rng.standard_normal(n + p + 2 * m)).to(ks.device)
        dz = torch.empty(n + p + 2 * m, **dev)

        def step():
            ks.set_scaling_from_iterate(v, s, lam)
            ks.factor(check=False)
            ks.solve4x4_dev(lam, r, dz)
            ks.solve4x4_dev(lam, r, dz)

        step()
        ks.check_factor()
        step_ms = _timed(step, 20, 3)
        x, y = torch.from_numpy(rng.standard_normal(n)).to(ks.device), torch.empty(n, **dev)
        gemv_ms = _timed(lambda: ks.gemv(L.MAT_Q, 0, 1.0, x, 0.0, y), 50, 5)
        assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(y).all())
    finally:
        ks.close()
    return dict(create_s=create_s, step_ms=step_ms, bytes=int(held), gemv_ms=gemv_ms)


def configs():
    n = 8192
    yield "boxqp_n8192_Q_I", (sp.identity(n, format="csr"), sp.identity(n, format="csr"), None, [("R", n)])
    Q, _, A, _, cone_dims, G, _ = W.c3_socp()
    yield "c3_socp", (sp.identity(Q.shape[0], format="csr"), A, G, cone_dims)


def rows_sweep(n):
    """gemv(CIP_MAT_Q) on symmetric banded matrices with 1 .. 2048 entries per row, in the form the environment selects"""
    out = {}
    x = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).cuda()
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    for half in (0, 1, 2, 4, 8, 12, 16, 24, 32, 64, 128, 256, 512, 1024):
        offs = list(range(-half, half + 1))
        Q = sp.diags([np.full(n - abs(o), 1.0 / (1 + abs(o))) for o in offs], offs, format="csr")
        ks = cipkkt.KKTSystem(Q, sp.identity(n, format="csr"), None, [("R", n)], sparse_q=True)
        try:
            out[str(2 * half + 1)] = _timed(lambda: ks.gemv(L.MAT_Q, 0, 1.0, x, 0.0, y), 200, 10) * 1e3      # microseconds
        finally:
            ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=0, help="n of the banded row-length sweep (0: the two configurations)")
    args = ap.parse_args()
    if args.rows:
        print(json.dumps(dict(n=args.rows, wave_min=os.environ.get("CIP_QSPMV_WAVE_MIN"), gemv_us_by_row_length=rows_sweep(args.rows))))
        return
    out = {}
    for name, (Q, A, G, cone_dims) in configs():
        out[name] = {form: [measure(Q, A, G, cone_dims, form == "sparse_q", seed=k) for k in range(args.repeats)]
                     for form in ("dense", "sparse_q")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
