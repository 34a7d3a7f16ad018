"""Problem instances for the small-problem batch path (cip_conicip_small; tests/test_gpu_small_batch.py), built without a GPU.

The path's iterates differ from the oracle's in rounding, so a case is only a fair trajectory test when the oracle's iteration
count does not hang on the last bits: `robust(sol, optTol)` says whether, for an :Optimal run, max(rDu, rPr, rCp) is below
optTol / 2 at the last iteration and above 2 optTol at the one before.  The seeds listed here were chosen with it on the CPU
(`python tests/_small_cases.py` prints the check for every listed case; nothing is filtered when the tests run)."""
import numpy as np

OPT_EDGE = 1e-7

# (n, m, p) -> cone list: where a 16-wide tile, the order-128 limit, the m limit and a 64-lane segment boundary can go wrong
EDGE_SHAPES = [
    ((1, 1, 0), [("R", 1)]),
    ((3, 0, 1), []),
    ((15, 16, 0), [("R", 10), ("Q", 1), ("Q", 2), ("Q", 3)]),
    ((16, 17, 1), [("R", 14), ("Q", 3)]),
    ((17, 33, 0), [("R", 30), ("Q", 1), ("Q", 2)]),
    ((127, 130, 1), [("R", 65), ("Q", 65)]),
    ((128, 128, 0), [("R", 64), ("Q", 64)]),
    ((100, 1024, 28), [("R", 756), ("Q", 200), ("Q", 64), ("Q", 3), ("Q", 1)]),
]
# five robust seeds per edge shape (EDGE_SHAPES order), found by scanning 0, 1, 2, ... with robust()
EDGE_SEEDS = {
    (1, 1, 0): [0, 1, 3, 4, 5], (3, 0, 1): [0, 1, 2, 3, 4], (15, 16, 0): [0, 1, 3, 5, 8], (16, 17, 1): [0, 1, 2, 4, 5],
    (17, 33, 0): [0, 1, 2, 3, 4], (127, 130, 1): [0, 3, 4, 5, 7], (128, 128, 0): [1, 2, 6, 7, 10], (100, 1024, 28): [0, 2, 3, 5, 8],
}
# random_mixed(n=60, nq=4, kq=7, p=5) at optTol = 1e-8
MIXED_SEEDS = [0, 1, 2, 7, 8, 9]
# the 64 problems of (64, 128, 8) compared with the lock-step path
LOCKSTEP_SEEDS = [0, 1, 3, 4, 5, 8, 10, 13, 14, 15, 16, 19, 20, 22, 23, 24, 25, 26, 27, 29, 32, 33, 34, 35, 37, 38, 39, 40, 42, 44, 47, 48, 49,
                  50, 51, 52, 53, 54, 56, 61, 62, 66, 67, 68, 70, 71, 72, 75, 77, 79, 82, 84, 85, 86, 90, 94, 95, 96, 97, 99, 101, 102, 103,
                  104]


def cone_problem(n, p, cone_dims, seed, q_scale=1.0):
    """A strictly feasible dense problem (feasible at y = ones) with the given cone list, in the pattern of
    tests/problems.py: random_mixed.  Returns (Q, c, A, b, cone_dims, G, d)."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    Q = q_scale * (M.T @ M / n + 0.1 * np.eye(n))
    c = rng.standard_normal(n)
    rows, rhs = [], []
    one = np.ones(n)
    for t, k in cone_dims:
        Ak = rng.standard_normal((k, n)) * (0.3 if t == "R" else 0.2)
        if t == "R":
            bk = Ak @ one - (rng.random(k) + 0.5)                     # slack s = A 1 - b in (0.5, 1.5)
        else:
            s = rng.standard_normal(k) * 0.3
            s[0] = np.linalg.norm(s[1:]) + 0.5 + rng.random()
            bk = Ak @ one - s
        rows.append(Ak)
        rhs.append(bk)
    m = sum(k for _, k in cone_dims)
    A = np.vstack(rows) if rows else np.zeros((0, n))
    b = np.concatenate(rhs) if rhs else np.zeros(0)
    assert A.shape[0] == m
    G = rng.standard_normal((p, n)) if p else None
    d = G @ one if p else None
    return Q, c, A, b, list(cone_dims), G, d


def as_dict(prob, **kwargs):
    Q, c, A, b, K, G, d = prob[:7]
    dense = lambda M: None if M is None else np.asarray(M.toarray() if hasattr(M, "toarray") else M, dtype=np.float64)
    return dict(Q=dense(Q), c=c, A=dense(A), b=b, cone_dims=K, G=dense(G), d=d, kwargs=kwargs)


def robust(sol, optTol):
    """the oracle's iteration count does not depend on rounding: converged by a factor 2 at the end, unconverged by 2 before"""
    if sol.status != "Optimal":
        return False
    worst = [max(t["rDu"], t["rPr"], t["rCp"]) for t in sol.trace]
    return worst[-1] < optTol / 2 and (len(worst) < 2 or worst[-2] > 2 * optTol)


# ---- different fates in one batch, all of shape n = 6, m = 6 (one R cone), p = 1
def fates():
    """[(name, problem)]: QPs that stop at different iteration counts, an infeasible and an unbounded program, and an LP with a free
    variable (a zero column of A under Q = 0: a zero pivot in the static order, in the manner of the reference's "Miles problem 3")."""
    n = 6
    K = [("R", n)]
    out = []
    for seed, scale in ((26, 1.0), (15, 30.0), (28, 0.02)):           # 5, 8 and 10 iterations, each robust()
        out.append(("qp%d" % seed, cone_problem(n, 1, K, seed, q_scale=scale)))
    rng = np.random.default_rng(0)
    h = rng.standard_normal(n)
    G = np.zeros((1, n)); G[0, 0] = 1.0
    out.append(("infeasible", (np.outer(h, h), np.outer(h, h) @ np.arange(1.0, n + 1), np.eye(n), np.zeros(n), K, G, np.array([-1.0]))))   # y >= 0, y1 = -1
    G = np.zeros((1, n)); G[0, 0], G[0, 1] = 1.0, -1.0
    out.append(("unbounded", (np.zeros((n, n)), np.arange(1.0, n + 1), np.eye(n), np.zeros(n), K, G, np.array([0.0]))))
    A = np.eye(n); A[n - 1, n - 1] = 0.0                      # y6 is free: its row reads 0 >= -1
    b = np.zeros(n); b[n - 1] = -1.0
    out.append(("free_lp", (np.zeros((n, n)), np.array([1.0, 1.0, 1.0, 1.0, 1.0, 3.0]), A, b, K, np.ones((1, n)), np.array([4.0]))))
    return out


if __name__ == "__main__":
    import sys, os, time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import problems as P
    from oracle.conicip import conicIP as oracle

    def scan(make, optTol, want, start=0):
        seeds, s = [], start
        while len(seeds) < want:
            pr = make(s)
            if robust(oracle(*pr[:7], optTol=optTol), optTol):
                seeds.append(s)
            s += 1
        return seeds

    if "scan" in sys.argv:
        for (shape, K) in EDGE_SHAPES:
            n, m, p = shape
            t0 = time.time()
            print(shape, scan(lambda s: cone_problem(n, p, K, 1000 + s), OPT_EDGE, 5), "%.1fs" % (time.time() - t0), flush=True)
        print("mixed", scan(lambda s: P.random_mixed(n=60, nq=4, kq=7, p=5, seed=s), 1e-8, 6))
        print("lockstep", scan(lambda s: cone_problem(64, 8, [("R", 100), ("Q", 28)], 5000 + s), 1e-7, 64))
    for name in ("sphere", "simplex", "combined"):
        print(name, robust(oracle(*getattr(P, name)()[:7], optTol=1e-7, DTB=0.01, maxRefinementSteps=3), 1e-7))
    for (shape, K) in EDGE_SHAPES:
        n, m, p = shape
        print(shape, [robust(oracle(*cone_problem(n, p, K, 1000 + s), optTol=OPT_EDGE), OPT_EDGE) for s in EDGE_SEEDS.get(shape, [])])
    print("mixed", [robust(oracle(*P.random_mixed(n=60, nq=4, kq=7, p=5, seed=s)[:7], optTol=1e-8), 1e-8) for s in MIXED_SEEDS])
    print("lockstep", all(robust(oracle(*cone_problem(64, 8, [("R", 100), ("Q", 28)], 5000 + s), optTol=1e-7), 1e-7) for s in LOCKSTEP_SEEDS))
    for name, pr in fates():
        s = oracle(*pr, optTol=1e-7)
        print(name, s.status, s.Iter, robust(s, 1e-7) if s.status == "Optimal" else "-")
