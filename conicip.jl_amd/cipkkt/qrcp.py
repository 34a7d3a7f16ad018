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


def _as_matrix(B):
    B = np.asarray(B, dtype=np.float64)
    if B.ndim != 2:
        raise ValueError("full_row_rank_hip: every block must be a matrix")
    return B


def _needs_device(B):
    """Does this block put the call into device-pointer mode?  A device tensor does, and so does a host array that is not
    column-major: it is uploaded as it lies and transposed on the device (numpy's strided copy of a row-major 8192 x 8192 block
    was measured at 4.2 s, the upload of the same block at 56 GB/s)."""
    if _is_sparse(B):
        return False
    if isinstance(B, torch.Tensor):
        if B.is_cuda:
            return True
        B = B.detach().numpy()
    return not _as_matrix(B).flags.f_contiguous


def _cert_block(B, on_device, dev, keep):
    """One cip_cert_block for B (n x k).  The library wants B column-major, which is the row-major image of B': the transpose of a
    row-major array (A' of the dual test) is handed over where it lies.  `keep` collects what the pointers refer to."""
    blk = L.CipCertBlock()
    if _is_sparse(B):
        S = B.tocsr().copy()
        S.sum_duplicates()
        rp, ci = S.indptr.astype(np.int32), S.indices.astype(np.int32)
        va = np.ascontiguousarray(S.data, dtype=np.float64)
        keep += [rp, ci, va]
        blk.cols = S.shape[1]
        blk.rowptr, blk.colind, blk.val = rp.ctypes.data, ci.ctypes.data, va.ctypes.data
        return blk, S.shape[0]
    if isinstance(B, torch.Tensor) and not B.is_cuda:
        B = B.detach().numpy()
    if isinstance(B, torch.Tensor):
        if B.dim() != 2:
            raise ValueError("full_row_rank_hip: every block must be a matrix")
        Bt = B.to(torch.float64).t().contiguous()                # k x n row-major (no copy when B is the transpose of one)
    else:
        B = _as_matrix(B)
        if B.flags.f_contiguous:
            Bt = B.T                                             # a view
            if on_device:
                Bt = torch.from_numpy(Bt).to(dev)
        else:
            Bt = torch.from_numpy(np.ascontiguousarray(B)).to(dev).t().contiguous()      # (on_device: _needs_device)
    keep.append(Bt)
    n, k = B.shape
    blk.cols = k
    blk.ld = max(n, 1)
    if n * k:
        blk.dense = Bt.data_ptr() if isinstance(Bt, torch.Tensor) else Bt.ctypes.data
    return blk, n


def full_row_rank_hip(blocks, eps=1e-8):
    """The full-row-rank certificate of `preprocess._full_row_rank` on the device (cip_rowrank_cert): True when M = [B_1 B_2 ...]
    (blocks with n rows each: dense arrays, scipy sparse matrices or device tensors) CERTAINLY has n independent rows by the
    reference's criterion, sigma_min(M) / ||M||_F >= max(100 eps, 1e-6); False = "not certified" (run the QR), never "rank
    deficient".  Sparse blocks stay sparse and device tensors are read where they lie.  Column-major host arrays -- the transposes of
    row-major ones -- are handed over as host pointers and staged by the library panel by panel; a row-major host array moves the
    dense blocks of the call to the device, where it is transposed."""
    _require_gpu()
    lib = L.load()
    blocks = list(blocks)
    dev = torch.device("cuda", torch.cuda.current_device())
    on_device = any(_needs_device(B) for B in blocks)
    keep, arr, rows = [], (L.CipCertBlock * max(len(blocks), 1))(), set()
    for i, B in enumerate(blocks):
        arr[i], n = _cert_block(B, on_device, dev, keep)
        rows.add(n)
    if len(rows) > 1:
        raise ValueError("full_row_rank_hip: the column blocks must have the same number of rows")
    n = rows.pop() if rows else 0
    if on_device:
        torch.cuda.current_stream().synchronize()              # the call works on the null stream: the blocks must be there
    ok = C.c_int(0)
    L.check(lib.cip_rowrank_cert(n, len(blocks), arr, float(eps), (L.FLAG_DEVICE_PTRS | L.FLAG_CSR_HOST) if on_device else 0,
                                 C.byref(ok), None, None))
    del keep
    return bool(ok.value)


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
