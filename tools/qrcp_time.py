"""`imcols_hip` (device rank-revealing QR, csrc/qrcp.hip) against the host `imcols` (scipy geqp3) on the same inputs.

    python tools/qrcp_time.py [--no-host] [--no-big] [--reps R]

Cases: the pre-solve's rank-deficient dual matrix [Q A'] of the Q = 0, A = [I I] family at n = 2048 and 4096 variables (n x 1.5 n,
rank n / 2: the QR stops at its rank), one full-rank 4096 x 12288 matrix, and -- device only, the host refuses it
(preprocess.DENSE_QR_LIMIT) -- the headline-size 8192 x 24576 one.  The device inputs are staged on the GPU beforehand (the timed
region is the concatenation of the blocks, the scaled working copy, the QR, the consistency solve); the host gets numpy arrays.
One warm-up each, then the median of R runs on a synchronised host clock.  For the device the stand-alone factorisation
(cip_qrcp_dev) is also timed with device events on a copy of the same matrix: steps, launches per step, and the bytes the column
updates move (16 bytes per trailing entry and step: one read, one write) over the time of the whole chain -- a lower bound of the
update kernel's own rate, against the 6.3 TB/s a copy achieves."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/conicip.jl_amd"):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cipkkt  # noqa: E402
from cipkkt import _lib as L  # noqa: E402

F64 = dict(dtype=torch.float64, device="cuda")
COPY_BYTES = 6.3e12


def wall(fn, reps):
    fn()                                                  # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    out.sort()
    return out[len(out) // 2], r


def qr_chain(lib, A, eps):
    """cip_qrcp_dev on a scaled copy of A' (rows of A = columns): (ms, k, update bytes)"""
    cnt, ln = A.shape
    nb = C.c_size_t()
    L.check(lib.cip_qrcp_workspace_bytes(ln, cnt, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    k = C.c_int(0)
    scale = float(torch.linalg.norm(A))
    ms = []
    for _ in range(2):                                    # the first is the warm-up
        W = (A / scale).contiguous()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.cip_qrcp_dev(None, W.data_ptr(), ln, cnt, ln, eps, ws.data_ptr(), None, None, None, C.byref(k)))
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        del W
    kk = k.value
    moved = 16.0 * sum((ln - j) * (cnt - j - 1) for j in range(kk))
    return ms[-1], kk, moved


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    host, big = "--no-host" not in args, "--no-big" not in args
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(11)
    cases = []
    for n in (2048, 4096):                                # [Q A'] with Q = 0 (n x n) and A = [I I] (n/2 x n)
        h = n // 2
        At = torch.cat([torch.eye(h, **F64), torch.eye(h, **F64)], dim=0)
        cases.append(("Q=0, A=[I I], n=%d" % n, [torch.zeros(n, n, **F64), At], True))
    cases.append(("full rank 4096 x 12288", [torch.randn(4096, 12288, generator=g, **F64)], True))
    if big:
        cases.append(("full rank 8192 x 24576", [torch.randn(8192, 24576, generator=g, **F64)], False))
    out = []
    print("%-26s %12s %7s %12s %12s %9s %14s %8s" % ("case", "rows x len", "rank", "device s", "host s", "host/dev", "QR chain ms", "TB/s"))
    for name, blocks, with_host in cases:
        rows, ln = blocks[0].shape[0], sum(B.shape[1] for B in blocks)
        b = torch.cat(blocks, dim=1) @ torch.randn(ln, generator=g, **F64)       # consistent right-hand side
        td, (kept, ok) = wall(lambda: cipkkt.imcols_hip(blocks, b), reps)
        th = None
        if with_host and host:
            Ah, bh = np.hstack([B.cpu().numpy() for B in blocks]), b.cpu().numpy()
            th, (kept_h, ok_h) = wall(lambda: cipkkt.imcols(Ah, bh), 1 if rows >= 4096 else reps)
            assert (len(kept_h), ok_h) == (len(kept), ok), (name, len(kept_h), ok_h, len(kept), ok)
            del Ah
        A = torch.cat(blocks, dim=1)
        ms, k, moved = qr_chain(lib, A, 1e-8)
        del A
        rate = moved / (ms * 1e-3) if k else 0.0
        rec = dict(case=name, rows=rows, len=ln, rank=len(kept), consistent=bool(ok), device_s=td, host_s=th, qr_chain_ms=ms, qr_steps=k,
                   launches_per_step=2, update_bytes=moved, update_bytes_per_s=rate, share_of_copy=rate / COPY_BYTES)
        out.append(rec)
        print("%-26s %12s %7d %12.4f %12s %9s %14.2f %8.2f" % (name, "%d x %d" % (rows, ln), len(kept), td, "%.4f" % th if th else "-",
                                                              "%.1f" % (th / td) if th else "-", ms, rate / 1e12), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
