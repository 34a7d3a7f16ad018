// What the three files of the large S cones share (sdp_large.hip: the map of the whole path, the workspace, the congruences;
// sdp_large_nt.hip: nestod_sdc; sdp_large_eig.hip: maxstep_sdc): the workspace, the coherent accesses, and the host launchers of
// the kernels one file defines and another uses.  Which form a stage runs is cip_sdp_large_forms.h's to say.
#pragma once
#include "cip_handle.h"
#include "cip_sdp_large_forms.h"

#define LG_NPAD 4
// Who owns which words of LargeWs::vec (slots of rp doubles) and LargeWs::ctr (words): the one table; what it does not list is free.
// Both regions are cleared whole: vec at creation, ctr by every NT scaling and every cooperative tridiagonalisation.
enum {                                 // LG_V_SLOTS slots of rp doubles
    LG_V_LAM = 0,                      // the singular values of the NT scaling
    LG_V_DG = 1, LG_V_OF = 2,          // the tridiagonal of side 0: both tridiagonalisations and the side-0 certificate fallback
    LG_V_XBUF = 3, LG_V_PBUF = 5,      // two slots each: xbuf (cooperative tridiagonalisation) / vbuf (stepped form), pbuf of both
    LG_V_SCAL = 7,                     // the stepped form's scalars
    LG_V_DG1 = 9, LG_V_OF1 = 10,       // the tridiagonal of side 1: its certificate fallback
    LG_V_CERT = 11, LG_V_SLOTS = 12    // doubles 2 side, 2 side + 1: the certificate pair of `side`; double 8, as unsigned: fallbacks taken
};
enum {                                 // LG_C_WORDS words
    LG_C_BARRIER = 0,                  // words 0-7: grid-barrier counters (k_lg_tridiag counts in word 0)
    LG_C_SWEEP = 8,                    // words 8-47: the Jacobi's sweep flags, one per sweep
    LG_C_GIVEUP = 128,                 // the cooperative tridiagonalisation's give-up word
    LG_C_STAT = 200, LG_C_GATE = 210, LG_C_WORDS = 256     // + side: stat of the Lanczos max-step, gate of its certificate's fallback
};
// What one side of a max-step pair works in.  Side 0: the max-step's own matrices; side 1: the NT scaling's s-side buffers (Ks, its
// LDL' workspace, Tz / Ts / G as M1 / M2 / M3 -- all idle between scalings).
struct LargeSide {
    double *Kx, *M1, *M2, *M3;
    LdltWorkspace *wx;
    int *stat, *gate;              // words of ctr: steps of the Lanczos max-step, gate of its certificate's fallback
    double *cert;                  // the certificate pair
    double *dg, *of;               // the tridiagonal of the certificate's fallback
};
struct LargeWs {
    int rp = 0;                    // padded order (256, 512, 1024 or 2048)
    int chunk = 64;                // columns of A per batched congruence
    double *base = nullptr;        // one allocation
    double *Kz, *Ks, *Tz, *Ts, *G, *M1, *M2, *M3;      // rp x rp
    double *Rip;                   // nlarge x LG_NPAD x rp x rp: Rinv, Rinv', R, R' of every large cone, zero padded
    double *vec;                   // LG_V_SLOTS x rp, addressed through the accessors below
    double *slot(int v) const { return vec + (size_t)v * rp; }
    double *dg(int side = 0) const { return slot(side ? LG_V_DG1 : LG_V_DG); }
    double *of(int side = 0) const { return slot(side ? LG_V_OF1 : LG_V_OF); }
    double *cert(int side) const { return slot(LG_V_CERT) + 2 * side; }
    unsigned *fallbacks() const { return (unsigned *)(slot(LG_V_CERT) + 8); }
    LargeSide side(int sd) {
        return sd ? LargeSide{Ks, Tz, Ts, G, &ws, (int *)(ctr + LG_C_STAT + 1), (int *)(ctr + LG_C_GATE + 1), cert(1), dg(1), of(1)}
                  : LargeSide{Kz, M1, M2, M3, &wz, (int *)(ctr + LG_C_STAT), (int *)(ctr + LG_C_GATE), cert(0), dg(0), of(0)};
    }
    double *batchX, *batchT;       // chunk x rp x rp each
    // mat(a_i) of every column of A, per large cone, built once per upload (A does not change between the factorisations of a
    // problem): round 4 -- the strided pass over A' was 0.38 ms of every factorisation at order 256, n = 1024
    double *amat = nullptr;        // nlarge x ncols x rp x rp (null when that exceeds 4 GB or the columns do not fit one batch)
    int ncols = 0;
    const double *amat_src[CIP_MAX_LARGE_S] = {};   // the A' the images were built from (null: not built)
    unsigned *ctr;                 // LG_C_WORDS words: barrier counters, sweep flags, gates (table above)
    // round 5: warm start of the one-sided Jacobi (sdp_large_nt.hip: nt_warm_start): the right singular vectors of the previous NT
    // scaling of every large cone, and three work matrices
    double *Vw = nullptr;          // nlarge x rp x rp
    double *G0 = nullptr, *W1 = nullptr, *W2 = nullptr;
    int have_v[CIP_MAX_LARGE_S] = {};
    unsigned long long *vstate = nullptr;   // device, 2 words per large cone: [0] = 1: the stored V may be used; [1]: max |V'V - I| (bit pattern) of the current call
    int *hflag = nullptr, *hflag_dev = nullptr;   // host-mapped: {sweep flag, Cholesky flags, sequence number} of the Jacobi's read-backs
    int hseq = 0;
    LdltWorkspace wz, ws;
    int xz_z = 0, xz_s = 0;        // the upper triangles of their block inverses have been zeroed (they stay zero)
    hipStream_t s2 = nullptr;      // the s-side max-step of a pair runs here, beside the v-side one on the handle's stream
    hipEvent_t efork = nullptr, ejoin = nullptr;
};

__device__ __forceinline__ double lg_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lg_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

static inline dim3 lg_grid(long n) { return dim3((unsigned)((n + 255) / 256)); }
static inline int lg_set_attr(const void *fn, size_t bytes) {
    CIP_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// ---- sdp_large.hip.  The launchers only enqueue: the caller's CIP_HIP_CHECK(hipGetLastError()) stands where it stood.
// X[b] (rp x rp) = mat(x_b) padded with `padval` on the diagonal, b < batch: k_lg_mat
void lg_mat(hipStream_t s, const double *x, long xs, long xb, double *X, int r, int rp, double padval, int batch = 1);
// the order <= 256 products that read B = mat(xv) from, or write C as vecm to, the vector itself: k_gemm_nt_small<true, false> / <false, true>
void lg_gemm_from_vec(hipStream_t s, double *C, const double *A, const double *xv, int rp, int r);
void lg_gemm_to_vec(hipStream_t s, double *outv, const double *A, const double *B, int rp, int r);
// C_b = A_b B_b'  (rp x rp each); stride 0 = operand shared by the batch; tiles: GEMM_TILES_*, which 64-tiles are computed
int lg_gemm(hipStream_t s, double *C, long sC, const double *A, long sA, const double *B, long sB, int rp, int batch, int tiles = GEMM_TILES_ALL);
// ---- sdp_large_eig.hip
void lg_lanczos_stats_print(void);     // CIP_LG_LANCZOS_STATS: k_lg_lanczos1's histogram of step counts, at destroy
