"""Many right-hand sides against k single solves at N = 8192 (device events after a warm-up, repeats alternated in one process).

    python tools/solve_many_time.py [N] [reps]

Stand-alone: a random quasi-definite K ([[SPD, G'], [G, -I]]), cip_ldlt_solve_many_dev(k) against k x cip_ldlt_solve_dev.
Handle: the headline dense QP (config 2, A = I), cip_solve3x3_many_dev(k) against k x cip_solve3x3_dev.
Share of peak from DESIGN.md section 5: a many-solve does 4 N^2 k flop (fp64 MFMA, 78.6 TFLOP/s) and reads 8 N (N + 1) bytes of factor
(HBM, 8 TB/s) per chunk of <= 64 columns; a single solve reads the same bytes for one column."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/conicip.jl_amd"):
    sys.path.insert(0, p)
import torch  # noqa: E402
import cipkkt  # noqa: E402
from cipkkt import _lib as L  # noqa: E402
from cipkkt import workloads as W  # noqa: E402

F64 = dict(dtype=torch.float64, device="cuda")
PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8.0e12
KS = (1, 8, 32, 64)


def timed(fn, reps):
    """ms per call: median over reps of one call between two events."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return out[len(out) // 2]


def bound(N, k, ms):
    flop = 4.0 * N * N * k
    byts = 8.0 * N * (N + 1) * ((k + 63) // 64)
    t_mfma, t_hbm = flop / PEAK_FLOPS, byts / PEAK_BYTES
    which = "MFMA" if t_mfma > t_hbm else "HBM"
    return which, max(t_mfma, t_hbm) / (ms * 1e-3)


def standalone(lib, N, reps):
    g = torch.Generator(device="cuda").manual_seed(7)
    n1 = N - N // 4
    M = torch.randn(n1, n1, generator=g, **F64)
    K = torch.zeros(N, N, **F64)
    K[:n1, :n1] = M @ M.t() / n1 + torch.eye(n1, **F64)
    G = torch.randn(N - n1, n1, generator=g, **F64) / n1 ** 0.5
    K[n1:, :n1] = G
    K[:n1, n1:] = G.t()
    K[n1:, n1:] = -torch.eye(N - n1, **F64)
    del M, G
    nb = C.c_size_t()
    L.check(lib.cip_ldlt_workspace_bytes(N, C.byref(nb)))
    ws = torch.empty(nb.value // 8 + 1, **F64)
    L.check(lib.cip_ldlt_factor_dev(None, K.data_ptr(), N, N, ws.data_ptr(), None))
    L.check(lib.cip_ldlt_solve_many_scratch_bytes(N, 64, C.byref(nb)))
    scratch = torch.empty(nb.value // 8, **F64)
    B = torch.randn(64, N, generator=g, **F64)
    s = torch.cuda.current_stream().cuda_stream
    rows = []
    for k in KS:
        Bk = B[:k].clone()

        def many():
            L.check(lib.cip_ldlt_solve_many_dev(C.c_void_p(s), K.data_ptr(), N, N, ws.data_ptr(), scratch.data_ptr(), Bk.data_ptr(), N, k))

        def singles():
            for j in range(k):
                L.check(lib.cip_ldlt_solve_dev(C.c_void_p(s), K.data_ptr(), N, N, ws.data_ptr(), Bk[j].data_ptr()))
        many(); singles(); torch.cuda.synchronize()                   # warm-up
        tm, ts = [], []
        for _ in range(3):                                            # alternated
            tm.append(timed(many, reps)); ts.append(timed(singles, max(2, reps // 4)))
        rows.append(("ldlt_solve_many_dev", k, min(tm), min(ts)))
    return rows


def handle(N, reps):
    Q, c, A, b, cd = W.c2_problem(N, seed=1234, device="cuda")
    ks = cipkkt.KKTSystem(Q, A, None, cd)
    ks.set_scaling_identity()
    ks.factor(check=True)
    g = torch.Generator(device="cuda").manual_seed(3)
    n, m = ks.n, ks.m
    X, Z = torch.randn(64, n, generator=g, **F64), torch.randn(64, m, generator=g, **F64)
    Y = torch.zeros(64, 1, **F64)
    Ao, Co, Bo = torch.empty(64, n, **F64), torch.empty(64, m, **F64), torch.zeros(64, 1, **F64)
    rows = []
    for k in KS:
        def many():
            ks.solve3x3_many_dev(X[:k], Y[:k], Z[:k], Ao[:k], Bo[:k], Co[:k])

        def singles():
            for j in range(k):
                ks.solve3x3_dev(X[j], Y[j], Z[j], Ao[j], Bo[j], Co[j])
        many(); singles(); torch.cuda.synchronize()
        tm, ts = [], []
        for _ in range(3):
            tm.append(timed(many, reps)); ts.append(timed(singles, max(2, reps // 4)))
        rows.append(("solve3x3_many_dev", k, min(tm), min(ts)))
    ks.close()
    return rows


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lib = L.load()
    rows = standalone(lib, N, reps) + handle(N, reps)
    print("%-22s %4s %10s %10s %12s %12s %7s  %s" % ("call", "k", "many ms", "k x 1 ms", "many ms/rhs", "single ms/rhs", "ratio", "bound, share of peak"))
    out = []
    for name, k, tm, ts in rows:
        which, share = bound(N, k, tm)
        print("%-22s %4d %10.3f %10.3f %12.4f %12.4f %7.3f  %s %.1f %%" % (name, k, tm, ts, tm / k, ts / k, tm / ts, which, 100 * share))
        out.append(dict(call=name, N=N, k=k, many_ms=tm, singles_ms=ts, ratio=tm / ts, bound=which, share_of_peak=share))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
