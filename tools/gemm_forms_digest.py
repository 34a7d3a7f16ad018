"""One SHA-256 per line over the raw fp64 bytes of what every form of the fp64 GEMM (csrc/gemm_f64.hip, the single products of
csrc/sdp_large.hip) produces, on the smallest shapes that reach each kernel: compare two builds line by line,

    CIPKKT_LIB=/path/to/libcipkkt.so python tools/gemm_forms_digest.py

one process per library.  Asserts nothing.  Inputs come from the portable generator of cipkkt/workloads.py, element-wise
only (no host BLAS product), so the same machine gives the same inputs to both builds.  Each line names the kernel the
shape is there for; the selection rules are those of gemm_f64.hip (rect_on_quarter_tiles, cip_syrk_split, syrk_split_128),
ldlt.hip (cip_ldlt_outer_block_for, doubling_tiny) and sdp_large.hip (lg_gemm)."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + '/conicip.jl_amd'): sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, torch, cipkkt
from cipkkt import _lib as L
from cipkkt.workloads import randn_np, uniform_np

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


# ---------------------------------------------------------------------------------------------------- cip_gemm_nt_dev
def gemm_nt(M, N, K, lower, what):
    seed = 100 * M + K + lower
    A, B, C0 = randn_np(seed, M, K), randn_np(seed + 1, N, K), randn_np(seed + 2, M, N)
    lda, ldb, ldc = M + 128, N + 256, M + 384
    dA, dB, dC = (torch.full((cols, ld), float("nan"), **F64) for cols, ld in ((K, lda), (K, ldb), (N, ldc)))
    dA[:, :M], dB[:, :N], dC[:, :M] = (torch.as_tensor(np.ascontiguousarray(X.T), **F64) for X in (A, B, C0))
    L.check(lib.cip_gemm_nt_dev(None, M, N, K, -0.75, dA.data_ptr(), lda, dB.data_ptr(), ldb, dC.data_ptr(), ldc, lower))
    line("cip_gemm_nt_dev M %d N %d K %d lower %d (%s): C with its padding" % (M, N, K, lower, what), dC)


gemm_nt(256, 256, 16, 0, "k_gemm_nt_64")
gemm_nt(256, 256, 144, 0, "k_gemm_nt_64")
gemm_nt(2048, 2048, 16, 0, "k_gemm_nt_128")
gemm_nt(256, 256, 144, 1, "k_ldlt_trailing_64<EPI_ACCUM>")

# ---------------------------------------------------------------------------------------- stand-alone LDL' of order 2048
# outer block 512 below order 4096, no wide tail: three trailing updates (k_ldlt_trailing_64<EPI_ACCUM>); solve block 1024:
# doubling of block 0 on k_gemm_nt_64_batched, of block 1 on k_gemm_nt_16_batched.  The in-block updates are k_gemm_nt_64
# launches on the three-launch panel chain only (the one-launch chain carries them inside k_ldlt_panel): first a factor on that chain
N = 2048
nb = C.c_size_t()
L.check(lib.cip_ldlt_workspace_bytes(N, C.byref(nb)))
ws = torch.zeros(nb.value // 8 + 8, **F64)
info = C.c_int(-1)
K0 = torch.as_tensor(sym_pd(N, 7), **F64).t().contiguous()
prev = lib.cip_set_ldlt_fused_chain(0)
Kd = K0.clone()
L.check(lib.cip_ldlt_factor_dev(None, Kd.data_ptr(), N, N, ws.data_ptr(), C.byref(info)))
line("cip_ldlt_factor_dev order 2048, three launches per panel (info %d): the factor" % info.value, Kd)
lib.cip_set_ldlt_fused_chain(prev)
Kd = K0.clone()
L.check(lib.cip_ldlt_factor_dev(None, Kd.data_ptr(), N, N, ws.data_ptr(), C.byref(info)))
line("cip_ldlt_factor_dev order 2048 (info %d): the factor" % info.value, Kd)
x = torch.as_tensor(randn_np(8, N), **F64)
L.check(lib.cip_ldlt_solve_dev(None, Kd.data_ptr(), N, N, ws.data_ptr(), x.data_ptr()))
line("cip_ldlt_solve_dev order 2048: one solve", x)
L.check(lib.cip_ldlt_solve_many_scratch_bytes(N, 8, C.byref(nb)))
scratch = torch.empty(max(nb.value // 8, 1), **F64)
X = torch.as_tensor(randn_np(9, 8, N), **F64)
L.check(lib.cip_ldlt_solve_many_dev(None, Kd.data_ptr(), N, N, ws.data_ptr(), scratch.data_ptr(), X.data_ptr(), N, 8))
line("cip_ldlt_solve_many_dev order 2048: 8 columns", X)
del ws, Kd, X, scratch

# ------------------------------------------------------------ box QP of order 2048, CSR A = I: the lazy-copy trailing update
n = 2048
ks = cipkkt.KKTSystem(sym_pd(n, 11), sp.identity(n, format="csr"), None, [("R", n)])
ks.set_scaling_packed(0.5 + uniform_np(12, n))
ks.factor()
line("box QP order 2048, A = I (k_ldlt_trailing_64<EPI_LAZYC>): K after cip_factor", ks.kkt_matrix())
ks.close()

# --------------------------------------------------------------------------------- dense A, one R cone: the Schur formation
for n, m, what in ((256, 256, "k_syrkq_64"), (256, 4096, "k_syrk_splitk_64 + k_syrk_reduce"), (128, 16384, "k_syrk_splitk_128 + k_syrk_reduce")):
    ks = cipkkt.KKTSystem(sym_pd(n, 20 + n), randn_np(21 + m, m, n), None, [("R", m)])
    ks.set_scaling_packed(0.5 + uniform_np(22 + m, m))
    ks.assemble_only()
    line("dense A n %d m %d (%s): K after cip_assemble_only" % (n, m, what), ks.kkt_matrix())
    ks.close()

# ------------------------------------------------------------------------------------------- large S cones, dense A, n = 4
# order 133 (padded to 256): every product is a single one on k_gemm_nt_small, plain / BVEC / CVEC; order 300 (padded to 512):
# k_gemm_nt_64_batched, with the "lower tiles only" selection in cip_sdp_large_scale_At
for r in (133, 300):
    k = r * (r + 1) // 2
    n = 4
    ks = cipkkt.KKTSystem(sym_pd(n, 30 + r), randn_np(31 + r, k, n), None, [("S", k)])
    v, s = (torch.as_tensor(vecm(sym_pd(r, seed)), **F64) for seed in (32 + r, 33 + r))
    lam = torch.zeros(k, **F64)
    ks.set_scaling_from_iterate(v, s, lam)
    line("S cone order %d: packed scaling after set_scaling_from_iterate" % r, ks.get_scaling_packed())
    line("S cone order %d: lambda" % r, lam)
    xs = torch.as_tensor(vecm(sym_pd(r, 34 + r) - 2.0 * np.eye(r)), **F64)
    out = torch.zeros(k, **F64)
    for mode, name in ((L.OP_F, "F"), (L.OP_FT, "F'"), (L.OP_FINV, "F^-1"), (L.OP_FINVT, "F^-T")):
        ks.apply_F(mode, xs, out)
        line("S cone order %d: apply %s" % (r, name), out)
    line("S cone order %d: maxstep(v, x)" % r, np.array([ks.maxstep(v, xs)]))
    ks.assemble_only()
    line("S cone order %d: K after cip_assemble_only" % r, ks.kkt_matrix())
    ks.close()
