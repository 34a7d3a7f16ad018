"""Exact references, rounding bounds and a dispatch model for the HBM-bound vector kernels of csrc/vecops.hip: the column-dot
gemv (k_gemv_t), the symmetric mat-vec from the lower tiles (k_symv_tiles / k_symv_reduce), the CSR mat-vec (k_spmv_csr), the
multi-dot (k_dots1 / k_dots2) and axpby (k_axpby).  No GPU here; tests/test_vec_ref.py checks this module,
tests/test_gpu_vecops.py applies it to the device.

Exact arithmetic.  Veltkamp's splitter cuts a double into hi + lo of at most 26 significant bits each, so the four partial
products of two split doubles are exact doubles (no overflow or underflow at the magnitudes used here) and math.fsum, which
returns the correctly rounded sum of its arguments, gives
    exact_dot(x, y)     the correctly rounded value of sum_i x_i y_i
    exact_fma(a, x, t)  the correctly rounded value of a x + t, per element: what a hardware fused multiply-add returns
(math.fma does not exist in this Python).  Where a matrix is too large for that (the symmetric mat-vec at order 2176) the
reference is formed in numpy.longdouble, whose 64-bit significand leaves 2^-11 u per operation: far inside the bounds below.

Bounds, u = 2^-53.  A mat-vec entry y_j = alpha sum_i M_ij x_i + beta y0_j over k terms: each product is rounded once (or not
at all, where the compiler fuses it), the k terms are added in some order (each term passes through at most k - 1 additions,
whatever the tree), alpha, beta and the last addition round once each.  To first order that is (k + 2) u relative to
|alpha| (|M| |x|)_j + |beta y0_j|; the bound used is twice that,
    |got - want|_j <= 2 (k + 2) u (|alpha| (|M| |x|)_j + |beta y0|_j),
which covers the second-order terms and the reference's own rounding (u |want| for a correctly rounded dot).
For the dots the depth of the kernel's tree is known: a thread adds ceil(len / 8192) products (32 workgroups of 256 threads
stride the vector), then come a 6-level wave sum, two additions over the workgroup's four waves and a 6-level wave sum over
the 32 partial sums.  With k = ceil(len / 8192) + 16 (the products' own rounding included)
    |got - exact| <= k u / (1 - k u) sum_i |x_i y_i|.
The bounds are derived, not measured.

Dispatch model of k_gemv_t's aligned path (even leading dimension, 16-byte aligned matrix and x): lane l starts at i = 2 l
and takes 1024-row trips while i + 897 < rows, 512-row trips while i + 385 < rows, 128-row trips while i + 1 < rows, and the
odd tail if then i < rows.  gemv_trips(rows) returns the per-lane counts; GEMV_ROWS is the row table of the GPU tests, and
tests/test_vec_ref.py asserts that it reaches every class of lane the kernel has."""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SPLITTER = 2.0 ** 27 + 1.0

# row counts of k_gemv_t: around every trip threshold (i + 1, i + 385, i + 897 with i = 2 lane, lane 0 and lane 63), the 1024-row
# trip twice (2049 and up), the odd tail behind each kind of trip (129 / 513 / 1025), more than one kind in one call
GEMV_ROWS = (1, 2, 3, 127, 128, 129, 130, 385, 386, 387, 511, 512, 513, 897, 898, 899, 1023, 1024, 1025, 1026, 1151, 1409, 1537,
             2049, 2561, 2690)
TRIPS = (1024, 512, 128)
_TRIP_REACH = {1024: 897, 512: 385, 128: 1}


def ld_ok():
    """the extended type really is extended (x87: eps = 2^-63)"""
    return np.finfo(LD).eps < 2.0 ** -60


# ------------------------------------------------------------------------------------------------------------ exact arithmetic
def split(a):
    """Veltkamp: a = hi + lo exactly, both with at most 26 significant bits"""
    a = np.asarray(a, dtype=np.float64)
    c = SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def partial_products(x, y):
    """(4, ...) exact doubles whose sum is x * y, elementwise"""
    xh, xl = split(x)
    yh, yl = split(y)
    return np.stack([xh * yh, xh * yl, xl * yh, xl * yl])


def exact_dot(x, y):
    """the correctly rounded sum_i x_i y_i"""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    assert x.shape == y.shape
    return math.fsum(partial_products(x, y).ravel().tolist())


def exact_matvec_t(M, x):
    """y_j = the correctly rounded sum_i M[i, j] x[i] for a dense (rows, cols) array M: what one wave of k_gemv_t computes"""
    M, x = np.asarray(M, dtype=np.float64), np.asarray(x, dtype=np.float64)
    assert M.ndim == 2 and x.shape == (M.shape[0],)
    out = np.zeros(M.shape[1])
    if M.shape[0] == 0:
        return out
    # Dekker's product: p = fl(M x) and e = the sum of the four partial products minus p, which is a double and comes out exactly in
    # this order -- two exact terms per product instead of four, the same correctly rounded sum at half the cost of the fsum
    xh, xl = split(x)
    Mt = np.ascontiguousarray(M.T)
    Mh, Ml = split(Mt)
    P = Mt * x
    E = (((Mh * xh - P) + Mh * xl) + Ml * xh) + Ml * xl
    for j in range(M.shape[1]):
        out[j] = math.fsum(P[j].tolist() + E[j].tolist())
    return out


def exact_csr_matvec(indptr, indices, data, x):
    """row-wise exact dots of a CSR matrix with x; an empty row gives 0"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(len(indptr) - 1)
    for r in range(len(out)):
        a, b = indptr[r], indptr[r + 1]
        if b > a:
            out[r] = exact_dot(data[a:b], x[indices[a:b]])
    return out


def exact_fma(a, x, t):
    """the correctly rounded a * x + t, elementwise (a scalar or an array)"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    P = partial_products(np.broadcast_to(np.float64(a), x.shape), x).reshape(4, -1)
    tt = t.reshape(-1)
    return np.array([math.fsum((P[0, i], P[1, i], P[2, i], P[3, i], tt[i])) for i in range(tt.size)]).reshape(x.shape)


def ld_fma(a, x, t):
    """a * x + t in extended precision, within 2^-64 (1 + 2^-50) of the RESULT even where the sum cancels: the product as p + e
    (Dekker), p + t as s + r (Knuth's two-sum), both exact in doubles, then one extended addition s + (r + e).  A plain extended
    a * x + t is off by 2^-64 |a x| instead, which under cancellation is more than the 2^-10 u |want| a comparison may allow it."""
    assert ld_ok()
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    a = np.broadcast_to(np.float64(a), x.shape)
    ah, al = split(a)
    xh, xl = split(x)
    p = a * x
    e = (((ah * xh - p) + ah * xl) + al * xh) + al * xl
    s = p + t
    bb = s - p
    r = (p - (s - bb)) + (t - bb)
    return s.astype(LD) + (r.astype(LD) + e.astype(LD))


def ld_matvec(alpha, M, x, beta, y0, trans=False):
    """alpha op(M) x + beta y0 in extended precision (beta == 0: y0 is not read)"""
    assert ld_ok()
    Ml = np.asarray(M).astype(LD)
    s = LD(alpha) * ((Ml.T if trans else Ml) @ np.asarray(x).astype(LD))
    return s if beta == 0.0 else s + LD(beta) * np.asarray(y0).astype(LD)


# ------------------------------------------------------------------------------------------------------------ bounds
def matvec_bound(k, alpha, absMx, beta, y0):
    """2 (k + 2) u (|alpha| (|M| |x|) + |beta y0|), entrywise; k a count or an array of counts; beta == 0: no y0 term"""
    tail = np.abs(beta * np.asarray(y0, dtype=np.float64)) if beta != 0.0 else 0.0
    return 2.0 * (np.asarray(k, dtype=np.float64) + 2.0) * U * (abs(alpha) * np.asarray(absMx, dtype=np.float64) + tail)


def dot_depth(length):
    """the longest chain of roundings behind a k_dots1 / k_dots2 result"""
    return -(-int(length) // 8192) + 16


def dot_bound(x, y):
    k = dot_depth(len(x))
    return k * U / (1.0 - k * U) * float(np.abs(np.asarray(x) * np.asarray(y)).sum())


# ------------------------------------------------------------------------------------------------------------ inputs
def graded(rng, shape, decades=4.0):
    """normals times 10^uniform(-decades, decades): entries of every magnitude, so that an entrywise bound means something"""
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-decades, decades, shape)


def orthogonalised(x, y):
    """y minus its component along x (one fp64 Gram-Schmidt step): the dot with x cancels to rounding level"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return y - (float(x @ y) / float(x @ x)) * x


# ------------------------------------------------------------------------------------------------------------ k_gemv_t model
def gemv_trips(rows):
    """per lane of the aligned path: {1024: trips, 512: trips, 128: trips, "tail": 0 / 1, "last": the kind of the lane's last trip
    (None if it made none)} as integer arrays of length 64 (`last` as a list)"""
    out = {t: np.zeros(64, dtype=np.int64) for t in TRIPS}
    tail = np.zeros(64, dtype=np.int64)
    last = [None] * 64
    for lane in range(64):
        i = 2 * lane
        for t in TRIPS:
            while i + _TRIP_REACH[t] < rows:
                out[t][lane] += 1
                last[lane] = t
                i += t
        tail[lane] = 1 if i < rows else 0
    out["tail"], out["last"] = tail, last
    return out
