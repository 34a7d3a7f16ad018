"""Independent-problem batches sharded one problem per GPU (BASELINE config 5).

A single KKT system never leaves its GPU (north-star), so the only multi-GPU structure
is data parallelism over independent problems: problem i -> rank (i mod world).  There
is no data-path collective; one tiny all-reduce (RCCL over xGMI on the GPU box, gloo in
the CPU tests) combines convergence / timing statistics.
"""
import ctypes as C
import os
import time

import numpy as np
import torch


def release_cached_memory():
    """Give back the device arena the library keeps between lock-step batches (cip_release_cached_memory)."""
    from . import _lib as L
    L.check(L.load().cip_release_cached_memory())


def shard_indices(n_problems, rank, world):
    """Static round-robin assignment: problem i -> rank i % world."""
    return list(range(rank, n_problems, world))


def _solve_on_stream(pr, device):
    """One problem on its own HIP stream: small systems (n ~ 2048) are latency-bound -- a factorisation is a
    chain of tiny dependent launches -- so several of them in flight on different streams fill the chip."""
    from .driver import conicIP
    from .kkt import KKTSystem
    st = torch.cuda.Stream(device=device)
    with torch.cuda.stream(st):
        ks = KKTSystem(pr["Q"], pr["A"], pr.get("G"), pr["cone_dims"], device=device)
        ks.set_stream(st.cuda_stream)
        try:
            sol = conicIP(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], pr.get("G"), pr.get("d"), system=ks,
                          **pr.get("kwargs", {}))
        finally:
            st.synchronize()
            ks.close()
    return sol


def _native_options(kw):
    """cip_options of a batch's keyword dict (both native batch paths).  `infeasTol` / `refinementThreshold`: absent or None
    -> -1.0, which the library resolves to its defaults (optTol, optTol / 1e7); every number a caller gives goes through --
    0.0 too ("never certify" / "always refine")."""
    from . import _lib as L

    def given(key):
        x = kw.get(key)
        return -1.0 if x is None else float(x)

    return L.CipOptions(kw.get("optTol", 1e-6), kw.get("DTB", 0.01), given("infeasTol"), given("refinementThreshold"),
                        kw.get("maxRefinementSteps", 3), kw.get("maxIters", 100), 0)


class _Vectors:
    """What every native batch entry point takes behind the problems: the host vectors c, b, d of the problem dicts `prs` (a missing
    one: zeros) and y, w, v to be filled -- each of max(size, 1) entries, problem i's sizes being dims[i] = (n, m, p) -- and the
    result array.  `args(opt)`: the run of arguments from c to res; `solutions()`: the Solutions behind the call."""

    def __init__(self, prs, dims):
        from . import _lib as L

        def host(key, i, size):
            x = prs[i].get(key)
            return np.zeros(max(size, 1)) if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))

        self.dims = dims
        self.inputs = [[host(key, i, nmp[j]) for i, nmp in enumerate(dims)] for key, j in (("c", 0), ("b", 1), ("d", 2))]
        self.y, self.v, self.w = ([np.zeros(max(nmp[j], 1)) for nmp in dims] for j in range(3))      # (j: n, m, p)
        self.res = (L.CipResult * len(dims))()

    def args(self, opt):
        arr = lambda xs: (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])
        return tuple(arr(xs) for xs in self.inputs) + (C.byref(opt), arr(self.y), arr(self.w), arr(self.v), self.res)

    def solutions(self):
        from .driver import solution_from_result
        return [solution_from_result(self.res[i], self.y[i][:n], self.w[i][:p], self.v[i][:m]) for i, (n, m, p) in enumerate(self.dims)]


def _problem_array(prs, build):
    """(cip_problem array, keep-alive list, [(n, m, p)]) of the problem dicts `prs`; build(pr, its cone list as [(str, int)])
    returns one problem's (cip_problem, keep-alive, ...)"""
    from . import _lib as L
    built = [build(pr, [(str(t), int(k)) for t, k in pr["cone_dims"]])[:2] for pr in prs]
    return (L.CipProblem * len(prs))(*[st for st, _ in built]), [kp for _, kp in built], [(st.n, st.m, st.p) for st, _ in built]


def _solve_many_native(prs, device, in_flight, sparse_q=False):
    """All problems of this rank through `cip_conicip_many` (csrc/batch.hip): one handle + HIP stream per problem,
    `in_flight` native interior-point loops at once on the library's own host threads (no Python in the loop)."""
    from . import _lib as L
    from .kkt import KKTSystem
    lib = L.load()
    kw = prs[0].get("kwargs", {})
    opt = _native_options(kw)
    systems, streams = [], []
    try:
        for pr in prs:
            st = torch.cuda.Stream(device=device)
            with torch.cuda.stream(st):
                ks = KKTSystem(pr["Q"], pr["A"], pr.get("G"), pr["cone_dims"], device=device, sparse_q=pr.get("sparse_q", sparse_q))
            ks.set_stream(st.cuda_stream)
            systems.append(ks)
            streams.append(st)
        vec = _Vectors(prs, [(ks.n, ks.m, ks.p) for ks in systems])
        handles = (C.c_void_p * len(prs))(*[ks.h.value for ks in systems])
        with torch.cuda.device(device):
            L.check(lib.cip_conicip_many(handles, len(prs), *vec.args(opt), int(in_flight)))
        return vec.solutions()
    finally:
        for st in streams:
            st.synchronize()
        for ks in systems:
            ks.close()


def lockstep_regularize(on=None):
    """The process-wide switch `cip_set_lockstep_regularize`: True / 1 -- a problem whose factorisation needs the regularised
    LDL' (an LP with a free variable, singular Q with free variables) stays in its lock-step group; False / 0 (the default) --
    it leaves the group and is solved alone afterwards.  None only queries.  Returns the previous value (0 or 1)."""
    from . import _lib as L
    return int(L.load().cip_set_lockstep_regularize(-1 if on is None else int(bool(on))))


def lockstep_ragged(on=None):
    """The process-wide switch `cip_set_lockstep_ragged`: True / 1 -- problems of one shape whose CSR A or CSR Q differ in their
    numbers of non-zeros (or whose CSR Q take different mat-vec forms) share a lock-step group; False / 0 (the default) -- the nnz
    is part of the shape.  None only queries.  Returns the previous value (0 or 1)."""
    from . import _lib as L
    return int(L.load().cip_set_lockstep_ragged(-1 if on is None else int(bool(on))))


def _solve_problems_native(prs, device, in_flight, mode="auto", sparse_q=False, keep_regularized=False, ragged=False):
    """All problems of this rank through the library's batch entry points.
    mode "lockstep": `cip_conicip_lockstep` (csrc/lockstep.hip) -- problems of identical shape advance through the loop
    together, every step one launch with the problem index in the grid; "threads": `cip_conicip_problems`
    (csrc/batch.hip) -- `in_flight` host threads inside the library, each re-loading ONE handle on its own HIP stream
    with the next problem of the queue; "auto": `cip_conicip_mixed` -- every group of problems that share a shape (and
    hold no chip-wide S cone) in lock-step, the others through the threads.  CIP_BATCH=threads|lockstep overrides "auto".
    sparse_q (or a problem's own "sparse_q" key): Q goes over in CSR (cipkkt.kkt.make_problem); the form is part of the shape.
    keep_regularized: `lockstep_regularize(True)` around the native call, the previous setting restored behind it.
    ragged: `lockstep_ragged(True)` around the native call in the same way."""
    from . import _lib as L
    from .kkt import make_problem
    lib = L.load()
    kw = prs[0].get("kwargs", {})
    opt = _native_options(kw)
    k = len(prs)
    with torch.cuda.device(device):
        structs, keep, dims = _problem_array(prs, lambda pr, cd: make_problem(
            pr["Q"], pr["A"], pr.get("G"), cd, kw.get("kktsolver", "schur"), device, sparse_q=pr.get("sparse_q", sparse_q)))
        torch.cuda.current_stream(device).synchronize()     # the staging transposes ran on torch's stream
        vec = _Vectors(prs, dims)
        if mode == "auto":
            mode = os.environ.get("CIP_BATCH", "auto")
        prev = lockstep_regularize(True) if keep_regularized else None
        prev_ragged = lockstep_ragged(True) if ragged else None
        try:
            if mode == "lockstep":
                L.check(lib.cip_conicip_lockstep(k, structs, *vec.args(opt)))
            elif mode == "threads":
                L.check(lib.cip_conicip_problems(k, structs, *vec.args(opt), int(in_flight)))
            else:
                L.check(lib.cip_conicip_mixed(k, structs, *vec.args(opt), int(in_flight)))
        finally:
            if prev_ragged is not None:
                lockstep_ragged(prev_ragged)
            if prev is not None:
                lockstep_regularize(prev)
    return vec.solutions()


def _host_problem(Q, A, G, cone_dims, route="schur"):
    """(cip_problem, keep-alive list) with every matrix a HOST pointer (column-major copies; flags = 0): what the small-problem
    path takes for thousands of instances without a device staging copy each.  A scipy-sparse A goes over as CSR, a
    scipy-sparse Q is densified (as cipkkt.kkt.make_problem does without sparse_q).  Needs no GPU."""
    from . import _lib as L
    from .kkt import _host_csr, _is_sparse, _new_problem
    pr, keep = _new_problem(Q, A, G, cone_dims, route)
    n, m, p = pr.n, pr.m, pr.p

    def dense(M, rows, cols):
        if isinstance(M, torch.Tensor):
            M = M.detach().cpu().numpy()
        a = np.asfortranarray(np.asarray(M.toarray() if _is_sparse(M) else M, dtype=np.float64).reshape(rows, cols))
        keep.append(a)
        return C.c_void_p(a.ctypes.data)

    pr.Q, pr.ldq = dense(Q, n, n), n
    if m > 0 and _is_sparse(A):
        pr.A_rowptr, pr.A_colind, pr.A_val = _host_csr(A, keep)
        pr.A, pr.lda = None, max(m, 1)
    else:
        pr.A, pr.lda = (dense(A, m, n) if m > 0 else None), max(m, 1)
    pr.G, pr.ldg = (dense(G, p, n) if p > 0 else None), max(p, 1)
    pr.flags = 0
    return pr, keep


def small_fits(Q, A, G, cone_dims, route="schur"):
    """Does `cip_conicip_small` -- one workgroup per problem (csrc/small.hip) -- take a problem of this description?  The Schur
    route, dense A, R and Q cones, n + p <= 128, m <= 1024 (`cip_conicip_small_fits`; `small_fits.reason` holds the library's
    message after a False).  Needs the built library, no GPU."""
    from . import _lib as L
    pr, keep = _host_problem(Q, A, G, [(str(t), int(k)) for t, k in cone_dims], route)
    lib = L.load()
    rc = lib.cip_conicip_small_fits(C.byref(pr))
    small_fits.reason = "" if rc == 0 else (lib.cip_last_error() or b"").decode()
    del keep
    return rc == 0


small_fits.reason = ""


def small_stats():
    """`cip_small_stats` of the calling thread's last small-problem call: dict(finished, handed_over, launches, readbacks)."""
    from . import _lib as L
    out = (C.c_int * 4)()
    L.check(L.load().cip_small_stats(out))
    return dict(finished=out[0], handed_over=out[1], launches=out[2], readbacks=out[3])


def solve_small(problems, pointers="host", device=None, **options):
    """Problems of ONE shape (n, m, p, cone list) through `cip_conicip_small`: one workgroup per problem, two launches and one
    read-back per iteration whatever their number.  problems: dicts(Q, c, A, b, cone_dims, G, d) as for `solve_batch`; options: the
    keyword arguments of conicIP (optTol, DTB, infeasTol, refinementThreshold, maxRefinementSteps, maxIters) -- when none is given,
    the first problem's "kwargs".  pointers: "host" (default: the matrices stay numpy arrays, the library uploads them) or "device"
    (staged through cipkkt.kkt.make_problem); the results are the same bits.  A description the path does not take raises CipError
    (CIP_E_UNSUPPORTED, nothing computed); problems whose factorisation needs the regularised LDL' come back from
    `cip_conicip_mixed` (see `small_stats`).  Returns the list of Solutions."""
    from . import _lib as L
    if not problems:
        return []
    lib = L.load()
    kw = options if options else problems[0].get("kwargs", {})
    opt = _native_options(kw)
    route = kw.get("kktsolver", "schur")
    if pointers == "device":
        from .kkt import make_problem
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        structs, keep, dims = _problem_array(problems, lambda pr, cd: make_problem(pr["Q"], pr["A"], pr.get("G"), cd, route, dev))
        torch.cuda.current_stream(dev).synchronize()        # the staging transposes ran on torch's stream
    else:
        structs, keep, dims = _problem_array(problems, lambda pr, cd: _host_problem(pr["Q"], pr["A"], pr.get("G"), cd, route))
    vec = _Vectors(problems, dims)
    L.check(lib.cip_conicip_small(len(problems), structs, *vec.args(opt)))
    return vec.solutions()


def _small_bins(problems, indices):
    """the problems of `indices` binned by shape (n, m, p, cone list); [(fits the small path, [indices])] in order of first appearance"""
    from .kkt import _is_sparse
    bins = {}
    for i in indices:
        pr = problems[i]
        A, G = pr["A"], pr.get("G")
        key = (pr["Q"].shape[0], 0 if A is None else A.shape[0], 0 if G is None else G.shape[0],
               tuple((str(t), int(k)) for t, k in pr["cone_dims"]), bool(A is not None and _is_sparse(A)),
               str(pr.get("kwargs", {}).get("kktsolver", "schur")), bool(pr.get("sparse_q", False)))
        bins.setdefault(key, []).append(i)
    out = []
    for key, idx in bins.items():
        pr = problems[idx[0]]
        fits = not key[-1] and small_fits(pr["Q"], pr["A"], pr.get("G"), pr["cone_dims"], key[-2])
        out.append((fits, idx))
    return out


def solve_batch(problems, solve_fn=None, rank=0, world=1, dist=None, device=None, concurrency=1, native=False,
                reduce_device=None, sparse_q=False, keep_regularized=False, small=False, ragged=False):
    """problems: list of dicts(Q, c, A, b, cone_dims, G, d, kwargs).  Each rank solves its
    shard with `solve_fn` (default: the HIP-backed cipkkt.conicIP) and the statistics are
    reduced over ranks:  SUM(iters, n_factor, n_solve, n_optimal, n_problems), MAX(wall).
    `concurrency` > 1 (default solver only) keeps that many problems in flight on separate
    HIP streams, one Python thread each: a thread builds its problem's handle, runs the native loop
    (`cip_conicip`, GIL released) and frees it, so level-1 setup of one problem overlaps the solve of another
    (n = 2048, 8 problems: 583 KKT solves/s one at a time, 899 with 2 in flight).  `native=True` hands the problems to
    the library's batch entry point `cip_conicip_problems` (host threads inside the library, one re-loaded handle per
    thread: what a C caller uses); `native="handles"` builds all handles first and calls `cip_conicip_many`
    (605-683 KKT solves/s on the same batch: the setup is not overlapped).  `sparse_q=True` (native paths; or a "sparse_q"
    key of a problem dict) hands Q over in CSR.  `keep_regularized=True` (native batch entry points): problems that need the
    regularised factorisation stay in their lock-step group (`lockstep_regularize`).  `ragged=True` (the same entry points): CSR
    matrices of differing numbers of non-zeros share a lock-step group (`lockstep_ragged`).
    `small=True` (default solver only; off by default: today's callers keep today's bits; pass it by keyword): this rank's problems are binned by shape
    (n, m, p, cone list) and every bin `small_fits` accepts goes through `solve_small` -- one workgroup per problem; the other
    problems go where they go without the keyword.
    Returns (local_solutions, stats_dict)."""
    default_solver = solve_fn is None
    if solve_fn is None:
        from .driver import conicIP as solve_fn
    mine = shard_indices(len(problems), rank, world)
    sols = {}
    t0 = time.perf_counter()
    if small and default_solver and mine:
        rest = []
        for fits, idx in _small_bins(problems, mine):
            same = all(problems[i].get("kwargs", {}) == problems[idx[0]].get("kwargs", {}) for i in idx)
            if fits and same and not sparse_q:
                for i, sol in zip(idx, solve_small([problems[i] for i in idx], device=device)):
                    sols[i] = sol
            else:
                rest += idx
        mine = sorted(rest)
    same_opts = all(problems[i].get("kwargs", {}) == problems[mine[0]].get("kwargs", {}) for i in mine) if mine else True
    if default_solver and native and len(mine) > 0 and same_opts:
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        shard = [problems[i] for i in mine]
        if native == "handles":
            out = _solve_many_native(shard, dev, max(1, concurrency), sparse_q=sparse_q)
        else:
            out = _solve_problems_native(shard, dev, max(1, concurrency), native if native in ("lockstep", "threads") else "auto",
                                         sparse_q=sparse_q, keep_regularized=keep_regularized, ragged=ragged)
        for i, sol in zip(mine, out):
            sols[i] = sol
    elif default_solver and concurrency > 1 and len(mine) > 1:
        from concurrent.futures import ThreadPoolExecutor
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        with ThreadPoolExecutor(max_workers=concurrency) as ex:
            futs = {i: ex.submit(_solve_on_stream, problems[i], dev) for i in mine}
            for i, f in futs.items():
                sols[i] = f.result()
    else:
        for i in mine:
            pr = problems[i]
            sols[i] = solve_fn(pr["Q"], pr["c"], pr["A"], pr["b"], pr["cone_dims"], pr.get("G"), pr.get("d"),
                               **pr.get("kwargs", {}))
    wall = time.perf_counter() - t0
    sums = np.array([sum(s.Iter for s in sols.values()),
                     sum(getattr(s, "n_factor", 0) for s in sols.values()),
                     sum(getattr(s, "n_solve", 0) for s in sols.values()),
                     sum(1 for s in sols.values() if s.status == "Optimal"),
                     len(sols)], dtype=np.float64)
    mx = np.array([wall], dtype=np.float64)
    if dist is not None:                 # also with one rank (bench.py's CIP_BENCH_FORCE_DIST exercises RCCL on one GPU)
        # the statistics travel as tensors on `reduce_device` (default: the compute device -- RCCL; "cpu" under gloo)
        tdev = reduce_device if reduce_device is not None else (device if device is not None else "cpu")
        ts = torch.as_tensor(sums, device=tdev)
        tm = torch.as_tensor(mx, device=tdev)
        dist.all_reduce(ts, op=dist.ReduceOp.SUM)
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        sums, mx = ts.cpu().numpy(), tm.cpu().numpy()
    stats = dict(iters=int(sums[0]), n_factor=int(sums[1]), n_solve=int(sums[2]), n_optimal=int(sums[3]),
                 n_problems=int(sums[4]), wall_s=float(mx[0]))
    return sols, stats


def run_config5(rank, world, dist, device, steps, warmup, problems=None, count=64, n=2048, seed=4000, in_flight=4,
                solve_fn=None, barrier=None, reduce_device=None):
    """BASELINE config 5 as a timed job (bench.py --gpus N, N > 1; `--workload c5` on one GPU): `count` independent
    problems, problem i -> rank i mod world, every rank's shard resident in HBM before the timed region; a step is one
    pass over the whole batch (each rank its shard, `in_flight` problems at once through cip_conicip_problems).
    Returns (stats of one pass reduced over ranks, elapsed seconds for `steps` passes = MAX over ranks).
    `problems` / `solve_fn` are injectable (the gloo test runs the sharding and the reduction on CPU)."""
    if problems is None:
        from .workloads import c5_batch
        mine = shard_indices(count, rank, world)
        local = c5_batch(count, n, seed, device=device, indices=mine)
        problems = [None] * count                      # only this rank's shard is materialised
        for i, pr in zip(mine, local):
            problems[i] = pr
    sync = (lambda: torch.cuda.synchronize(device)) if device is not None and str(device) != "cpu" else (lambda: None)
    if barrier is None:
        barrier = (lambda: dist.barrier()) if dist is not None else (lambda: None)

    def one_pass(reduce):
        return solve_batch(problems, solve_fn=solve_fn, rank=rank, world=world, dist=dist if reduce else None,
                           device=device, concurrency=in_flight, native=solve_fn is None, reduce_device=reduce_device)

    for _ in range(warmup):
        one_pass(False)
    sync(); barrier(); sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        one_pass(False)
    sync()
    busy = time.perf_counter() - t0                    # this rank's own time for its shard (before it waits for the others)
    barrier(); sync()
    elapsed = time.perf_counter() - t0
    _, stats = one_pass(True)                          # untimed: the reduced statistics of one pass
    if solve_fn is None:
        release_cached_memory()                        # the lock-step arena (GBs) is not kept beyond the job
    busy_min = busy_max = busy
    if dist is not None:
        dev = reduce_device if reduce_device is not None else (device if device is not None else "cpu")
        t = torch.tensor([elapsed, busy, -busy], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, busy_max, busy_min = float(t[0].item()), float(t[1].item()), -float(t[2].item())
    # load imbalance over the ranks (problems need different iteration counts): per-pass busy time of the fastest / slowest rank
    stats = dict(stats, rank_busy_ms_min=1e3 * busy_min / max(steps, 1), rank_busy_ms_max=1e3 * busy_max / max(steps, 1))
    return stats, elapsed
