"""One SHA-256 per line over the raw fp64 bytes of what every form of the S-cone kernels (csrc/sdp.hip, csrc/sdp_large*.hip)
produces, on the smallest orders that reach each form: compare two builds line by line,

    CIPKKT_LIB=/path/to/libcipkkt.so python tools/sdp_forms_digest.py

one process per library.  Asserts nothing.  Inputs come from the portable generator of cipkkt/workloads.py, element-wise
only (no host BLAS product), so the same machine gives the same inputs to both builds.  Per handle: the packed scaling,
lambda, the four apply_F modes, cone_prod, cone_div by lambda and both forms of maxstep.  The forms and what selects them:
  sdp.hip          256 threads up to order 48, 1024 above (sd_threads, by the handle's largest S cone); the one-sided
                   Jacobi keeps both columns in registers while r <= 8 lanes-per-pair
  sdp_large*.hip   (cip_sdp_large_forms.h selects; the max-step's kernels are in sdp_large_eig.hip, the Jacobi's in
                   sdp_large_nt.hip)  order 133 (padded to 256): k_lg_lanczos1 with the certificate (mode 2), alone (1),
                   k_lg_tridiag1 + k_lg_sturm (0), the certificate's fallback on every call (3); 257 and 584 (padded to 512
                   and 1024): k_lg_tridiag with slabs of 32 and of 16 columns; 1025 (padded to 2048): k_tg_symv / k_tg_rank2
  corner handles   a cone of order 132 beside one of order 431 / 432: the small cone decides both max-steps (zero
                   direction, respectively the identity, on the large block)"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + '/conicip.jl_amd'): sys.path.insert(0, p)
import numpy as np, torch, cipkkt
from cipkkt import _lib as L
from cipkkt.workloads import randn_np

F64 = dict(dtype=torch.float64, device="cuda")
lib = L.load()


def line(label, x):
    if isinstance(x, torch.Tensor):
        torch.cuda.synchronize()
        x = x.cpu().numpy()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    print("%s  %s" % (hashlib.sha256(x.tobytes()).hexdigest(), label), flush=True)


def sym_pd(n, seed):
    """symmetric, eigenvalues within 2 +- 1 or so: a scaled Wigner matrix + 2 I"""
    R = randn_np(seed, n, n)
    return (R + R.T) / (2.0 * np.sqrt(2.0 * n)) + 2.0 * np.eye(n)


def vecm(Z):
    iu = np.triu_indices(Z.shape[0])
    x = Z[iu].copy()
    x[iu[0] != iu[1]] *= np.sqrt(2.0)
    return x


def dev(blocks):
    return torch.as_tensor(np.concatenate(blocks), **F64)


def case(label, orders, corner=False):
    """corner: the last cone is the large neighbour of the first -- it takes no part in either max-step"""
    dims = [("S", r * (r + 1) // 2) for r in orders]
    m, n = sum(k for _, k in dims), 4
    seed = 1000 * orders[0] + orders[-1]
    ks = cipkkt.KKTSystem(sym_pd(n, seed), randn_np(seed + 1, m, n), None, dims)
    v = dev([vecm(sym_pd(r, seed + 10 + i)) for i, r in enumerate(orders)])
    s = dev([vecm(sym_pd(r, seed + 20 + i)) for i, r in enumerate(orders)])
    xb = [vecm(sym_pd(r, seed + 30 + i) - 2.0 * np.eye(r)) for i, r in enumerate(orders)]      # indefinite
    x = dev(xb)
    lam, out = torch.zeros(m, **F64), torch.zeros(m, **F64)
    ks.set_scaling_from_iterate(v, s, lam)
    line("%s: packed scaling" % label, ks.get_scaling_packed())
    line("%s: lambda" % label, lam)
    for mode, name in ((L.OP_F, "F"), (L.OP_FT, "F'"), (L.OP_FINV, "F^-1"), (L.OP_FINVT, "F^-T")):
        ks.apply_F(mode, x, out)
        line("%s: apply %s" % (label, name), out)
    ks.cone_prod(x, v, out)
    line("%s: cone_prod" % label, out)
    ks.cone_div(x, lam, out)
    line("%s: cone_div by lambda" % label, out)
    if corner:
        rl = orders[-1]
        d = dev(xb[:-1] + [np.zeros(dims[-1][1])])
        x1 = dev(xb[:-1] + [vecm(np.eye(rl))])
    else:
        d, x1 = x, x
    line("%s: maxstep(v, d)" % label, np.array([ks.maxstep(v, d)]))
    line("%s: maxstep(x, nothing)" % label, np.array([ks.maxstep(x1, None)]))
    ks.close()


for r in (5, 48, 49, 132):
    case("S(%d)" % r, [r])
case("[S(6), S(60)]", [6, 60])
for mode in (2, 1, 0, 3):
    prev = lib.cip_set_sdp_lanczos(mode)
    case("S(133), cip_set_sdp_lanczos %d" % mode, [133])
    lib.cip_set_sdp_lanczos(prev)
for r in (257, 584, 1025):
    case("S(%d)" % r, [r])
for rl in (431, 432):
    case("[S(132), S(%d)]" % rl, [132, rl], corner=True)
