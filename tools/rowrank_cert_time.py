"""The pre-solve's full-row-rank certificate: `preprocess._full_row_rank` (host: numpy Gram matrix + LAPACK eigvalsh, the BLAS threads
the environment gives it) against `full_row_rank_hip` (device: csrc/rowrank.hip) on the same inputs.

    python tools/rowrank_cert_time.py [--no-host] [--no-big] [--reps R]

Cases: the box-QP dual matrix [Q I] with a dense Q = M'M / n and a CSR identity at n = 2048 and 4096, and -- the headline size --
[Q A'] with a dense A of 16384 rows at n = 8192 (8192 x 24576).  The device is timed twice, on a synchronised host clock around the
whole call: with the blocks as the pre-solve hands them over (numpy arrays in pageable host memory: the time includes their upload,
panel by panel) and with the dense blocks resident on the device.  One warm-up each, then the median of R runs (the host certificate
of the headline case runs once).  Both verdicts must agree."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/conicip.jl_amd"):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402
import cipkkt  # noqa: E402
from cipkkt.preprocess import _full_row_rank  # noqa: E402


def wall(fn, reps, warm=True):
    if warm:
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    out.sort()
    return out[len(out) // 2], r


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    host, big = "--no-host" not in args, "--no-big" not in args
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    rng = np.random.default_rng(5)
    out = []
    print("%-28s %14s %12s %14s %14s %10s" % ("case", "n x L", "host s", "device s", "resident s", "host/dev"), flush=True)
    for n, m_dense in [(2048, 0), (4096, 0)] + ([(8192, 16384)] if big else []):
        M = rng.standard_normal((n, n))
        Q = M.T @ M / n
        del M
        if m_dense:
            A = rng.standard_normal((m_dense, n))                # row-major m x n: A' is handed over where it lies
            blocks, name = [Q, A.T], "[Q A'], dense A %d x %d" % A.shape
        else:
            blocks, name = [Q, sp.identity(n, format="csr")], "[Q I], CSR identity"
        L = sum(B.shape[1] for B in blocks)
        td, vd = wall(lambda: cipkkt.full_row_rank_hip(blocks, 1e-8), reps)
        resident = [torch.from_numpy(np.ascontiguousarray(B.T)).cuda().t() if isinstance(B, np.ndarray) else B for B in blocks]
        tr, vr = wall(lambda: cipkkt.full_row_rank_hip(resident, 1e-8), reps)
        del resident
        torch.cuda.empty_cache()
        th = vh = None
        if host:
            th, vh = wall(lambda: _full_row_rank(blocks, 1e-8), 1 if n >= 8192 else reps, warm=n < 8192)
            assert bool(vh) == vd == vr, (name, vh, vd, vr)
        out.append(dict(case=name, n=n, L=L, host_s=th, device_s=td, device_resident_s=tr, certified=bool(vd),
                        threads=os.environ.get("OMP_NUM_THREADS")))
        print("%-28s %14s %12s %14.4f %14.4f %10s" % (name, "%d x %d" % (n, L), "%.3f" % th if th else "-", td, tr,
                                                      "%.1f" % (th / td) if th else "-"), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
