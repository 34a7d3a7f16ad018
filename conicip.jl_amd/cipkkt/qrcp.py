"""The device rank-revealing QR (csrc/qrcp.hip) and the pre-solve's `imcols` on top of it.

`qrcp_hip` is the stand-alone factorisation (cip_qrcp_dev), `imcols_hip` the device counterpart of `preprocess.imcols`
(cip_imcols_dev): same contract, no size limit.  The library wants A' column-major, which is A in row-major order -- the layout
a torch tensor has anyway -- so column blocks [B_1, B_2, ...] are uploaded one by one (sparse blocks as their stored entries)
and concatenated on the device: the wide matrix [Q A' G'] of the dual test never exists densely on the host.  PyTorch is used for
device memory only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .kkt import _is_sparse, _ptr, _require_gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_block(B, device):
    """2-D fp64 tensor on the device from a dense array, a scipy sparse matrix or a tensor"""
    if isinstance(B, torch.Tensor):
        return B.to(dtype=torch.float64, device=device)
    if _is_sparse(B):
        coo = B.tocsr().tocoo()                  # (through CSR: duplicates summed)
        out = torch.zeros(coo.shape, dtype=torch.float64, device=device)
        if coo.nnz:
            i = torch.from_numpy(coo.row.astype(np.int64)).to(device)
            j = torch.from_numpy(coo.col.astype(np.int64)).to(device)
            out[i, j] = torch.from_numpy(coo.data.astype(np.float64)).to(device)
        return out
    return torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64)).to(device)


def _row_major_image(A, device):
    """A (or the column blocks of A) as one contiguous row-major tensor on the device"""
    if isinstance(A, (list, tuple)):
        blocks = [_device_block(B, device) for B in A]
        rows = blocks[0].shape[0]
        if any(B.dim() != 2 or B.shape[0] != rows for B in blocks):
            raise ValueError("imcols_hip: the column blocks must be matrices with the same number of rows")
        return torch.cat(blocks, dim=1).contiguous()
    M = _device_block(A, device)
    if M.dim() != 2:
        raise ValueError("imcols_hip: A must be a matrix")
    return M.contiguous()


def qrcp_hip(M, stop=0.0):
    """Householder QR with column pivoting of M (len x cnt) on the device, stopped at the first step whose largest remaining
    column norm is <= stop.  Returns (factored, tau, piv, rdiag, k): LAPACK geqp3's layout in `factored` (len x cnt; R on and
    above the diagonal, reflector tails below it in the first k columns), tau[k], piv[cnt] (column j of the result is column
    piv[j] of M), rdiag[k] = diag(R), and the number of steps k."""
    _require_gpu()
    lib = L.load()
    M = np.asarray(M, dtype=np.float64)
    if M.ndim != 2:
        raise ValueError("qrcp_hip: M must be a matrix")
    ln, cnt = M.shape
    kmax = min(ln, cnt)
    dev = torch.device("cuda", torch.cuda.current_device())
    Mt = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)           # row-major cnt x len == column-major len x cnt
    nb = C.c_size_t()
    L.check(lib.cip_qrcp_workspace_bytes(ln, cnt, C.byref(nb)))
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dev)
    tau = torch.zeros(max(kmax, 1), dtype=torch.float64, device=dev)
    piv = np.zeros(max(cnt, 1), dtype=np.int32)
    rdiag = np.zeros(max(kmax, 1))
    k = C.c_int(0)
    L.check(lib.cip_qrcp_dev(_stream(), _ptr(Mt), ln, cnt, max(ln, 1), float(stop), _ptr(ws), _ptr(tau),
                             piv.ctypes.data_as(L.c_int_p), rdiag.ctypes.data_as(L.c_double_p), C.byref(k)))
    return np.ascontiguousarray(Mt.cpu().numpy().T), tau.cpu().numpy()[:k.value], piv[:cnt], rdiag[:k.value], k.value


def imcols_hip(A, b, eps=1e-8):
    """`imcols` on the device: (rows, consistent) with the contract of `preprocess.imcols` (src/preprocessor.jl:10-30) and no size
    limit.  A: a dense array, a scipy sparse matrix, a device tensor, or a list of column blocks of any of these kinds."""
    _require_gpu()
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    M = _row_major_image(A, dev)
    cnt, ln = M.shape
    if cnt * ln == 0:
        return [], True
    bd = (b if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64).reshape(-1)))
    bd = bd.to(dtype=torch.float64, device=dev).reshape(-1).contiguous()
    if bd.numel() != cnt:
        raise ValueError("imcols_hip: b has %d entries, A has %d rows" % (bd.numel(), cnt))
    nb = C.c_size_t()
    L.check(lib.cip_imcols_workspace_bytes(ln, cnt, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    rows = np.zeros(cnt, dtype=np.int32)
    nrows, ok = C.c_int(0), C.c_int(0)
    L.check(lib.cip_imcols_dev(_stream(), _ptr(M), ln, cnt, ln, _ptr(bd), float(eps), _ptr(ws), rows.ctypes.data_as(L.c_int_p),
                               C.byref(nrows), C.byref(ok), None))
    if not ok.value:
        return [], False
    return [int(i) for i in rows[:nrows.value]], True
