/*
 * libcipkkt -- MI355X (gfx950) native KKT-solve path for ConicIP-style
 * interior-point solvers.  C ABI: plain pointers and sizes only.
 *
 * This is the drop-in boundary for the reference's `kktsolver` plugin hook
 * (reference = MPF-Optimization-Laboratory/ConicIP.jl, paths relative to its
 * root):
 *
 *   level 1  kktsolver(Q, A, G, cone_dims)        src/ConicIP.jl:667
 *   level 2  solve3x3gen(F, F^-T)                 src/ConicIP.jl:682
 *   level 3  solve3x3(x, y, z) -> (a, b, c)       src/ConicIP.jl:688
 *
 * which the reference documents at src/ConicIP.jl:432-466 and
 * docs/src/guides/kkt_solvers.md:84-115, and implements three times in
 * src/kktsolvers.jl (kktsolver_qr :18-58, kktsolver_sparse :180-270,
 * pivot(kktsolver_2x2) :281-349).  The Julia-side `ccall` shim that binds these
 * entry points is shown in INTEGRATION.md.
 *
 * Conventions
 *   - all matrices column-major (Julia / LAPACK), fp64, 0-based C indices
 *   - the m-vector (v, s, lambda, z) is the concatenation of cone blocks in
 *     cone_dims order (src/ConicIP.jl:519-522); a Q block stores the bound t
 *     first; an S block stores `vecm` order (src/ConicIP.jl:128-151)
 *   - every entry point returns 0 on success, a negative CIP_E_* otherwise;
 *     cip_last_error() gives a message.  Nothing falls back to the CPU: when no
 *     HIP device is usable cip_create fails with CIP_E_NODEVICE.
 *   - `*_dev` entry points take DEVICE pointers and enqueue on the handle's
 *     stream without synchronising (except where a host scalar is returned);
 *     the un-suffixed ones take HOST pointers and are synchronous.
 *   - whole problems in, solutions out: cip_conicip (one handle), cip_conicip_lockstep / cip_conicip_mixed (batches, a launch
 *     chain per iteration for groups of up to 64) and cip_conicip_small (batches of problems with n + p <= 128: one workgroup per
 *     problem, two launches per iteration whatever their number).
 */
#ifndef CIPKKT_H
#define CIPKKT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cip_handle cip_handle;

/* cone types: "R", "Q", "S" of cone_dims (src/ConicIP.jl:421-430) */
#define CIP_CONE_R 0
#define CIP_CONE_Q 1
#define CIP_CONE_S 2

/* elimination route */
#define CIP_ROUTE_SCHUR   0  /* pivot on the F'F block first (algebra of src/kktsolvers.jl:316-338), dense LDL' of [S G';G 0] */
#define CIP_ROUTE_FULL3X3 1  /* literal 3x3 assembly (src/kktsolvers.jl:254-256), symmetrised, dense LDL' of order n+p+m */

/* block-operator modes for cip_apply_F_dev (src/blockmatrices.jl:173-200) */
#define CIP_OP_F      0
#define CIP_OP_FT     1
#define CIP_OP_FINV   2
#define CIP_OP_FINVT  3

/* which problem matrix (cip_gemv_dev) */
#define CIP_MAT_Q 0
#define CIP_MAT_A 1
#define CIP_MAT_G 2

/* flags for cip_create_ex */
#define CIP_FLAG_DEVICE_PTRS 1   /* Q/A/G arrays are device pointers */
#define CIP_FLAG_CSR_HOST    2   /* ... except the CSR arrays of A (and of Q), which are host pointers (the library needs them on
                                    the host anyway, to build the CSR of A' and to check Q) */
#define CIP_FLAG_Q_CSR       4   /* Q is given in CSR (Q_rowptr / Q_colind / Q_val); Q itself must be NULL */

#define CIP_OK            0
#define CIP_E_INVALID    -1
#define CIP_E_NODEVICE   -2
#define CIP_E_HIP        -3
#define CIP_E_NOTFACTORED -4
#define CIP_E_SINGULAR   -5   /* zero / non-finite pivot met in the LDL' */
#define CIP_E_UNSUPPORTED -6
#define CIP_E_RETRY      -7   /* nothing is wrong with the input: repeat the call (cip_ldlt_factor_dev: supply K again), or the solves it names */

/* Problem description for cip_create_ex.  A may be given dense (A != NULL) or
 * in CSR (A == NULL, A_rowptr/A_colind/A_val != NULL, 0-based) -- with any mix of cone types (the rows of S cones are expanded
 * into a dense block on the device; R / Q rows stay CSR).  S cones: matrix order r <= 2048 and at most 1024 cones of order >= 133
 * (CIP_E_UNSUPPORTED beyond either; the reference has no limit, src/ConicIP.jl:196-210).
 * Q may be given dense (Q != NULL) or, with CIP_FLAG_Q_CSR, in CSR (Q == NULL; the three Q_* arrays, 0-based, are read only when
 * the flag is set, so a caller compiled against the struct without them is never read past its end).  The CSR Q is the WHOLE
 * symmetric matrix -- both triangles stored, as a SparseMatrixCSC or a scipy matrix holds it; a symmetric CSC is its own CSR --
 * with the columns of a row in any order, no duplicate entries, nnz == 0 for the zero objective.  Level 1 checks it on the host
 * in O(nnz) (device-resident arrays are copied back first, as A's are): rowptr[0] == 0, a monotone row pointer, indices in range,
 * no duplicates, every (i, j) with a stored (j, i) of bit-equal value; a violation is CIP_E_INVALID naming the first offending
 * entry, before any device allocation.  Such a handle holds O(nnz) device memory for Q and every entry point keeps its meaning;
 * the flag together with Q != NULL is CIP_E_INVALID, Q == NULL without it stays CIP_E_INVALID "Q is NULL". */
typedef struct cip_problem {
    int n, m, p;
    int ncones;
    const int *cone_type;      /* ncones entries, CIP_CONE_* */
    const int *cone_dim;       /* ncones entries; for S: vectorised length k = r(r+1)/2 */
    const double *Q;  int ldq; /* n x n */
    const double *A;  int lda; /* m x n dense, or NULL */
    const int *A_rowptr; const int *A_colind; const double *A_val; /* CSR, m+1 / nnz / nnz */
    const double *G;  int ldg; /* p x n (may be NULL when p == 0) */
    int route;                 /* CIP_ROUTE_* */
    int flags;                 /* CIP_FLAG_* */
    const int *Q_rowptr; const int *Q_colind; const double *Q_val; /* CSR of Q, n+1 / nnz / nnz (CIP_FLAG_Q_CSR only) */
} cip_problem;

/* ---- level 1: kktsolver(Q, A, G, cone_dims)  (src/ConicIP.jl:667; src/kktsolvers.jl:18-28, :180-190, :281-285) */
int cip_create(int n, int m, int p, int ncones, const int *cone_type, const int *cone_dim,
               const double *Q, const double *A, const double *G, int route, cip_handle **out);
int cip_create_ex(const cip_problem *prob, cip_handle **out);
/* level 1 again on an existing handle: new Q / A / G of the same shape (n, m, p, cones, route, dense-or-CSR A with the
 * same nnz, dense-or-CSR Q with the same nnz -- else CIP_E_INVALID, the handle stays as it was); keeps every device allocation
 * (hipMalloc / hipFree synchronise the whole device) */
int cip_update_problem(cip_handle *h, const cip_problem *prob);
int cip_destroy(cip_handle *h);
const char *cip_last_error(void);
int cip_set_stream(cip_handle *h, void *hip_stream);

/* ---- level 2: solve3x3gen(F, F^-T)  (src/ConicIP.jl:682; src/kktsolvers.jl:30-35, :250-257, :287-295)
 * The scaling F is handed over in packed form, read off the reference's Block
 * elements (src/ConicIP.jl:189-192, :208, :598):
 *   R cone (k)   : k doubles        diag(F)
 *   Q cone (k)   : 1 + k doubles    beta, w      (F = diag(-beta, beta, ...) + w w')
 *   S cone (k)   : 2 r^2 doubles    R (r x r col-major), then inv(R) (r x r col-major)
 * cip_scaling_packed_len() returns the total length. */
size_t cip_scaling_packed_len(const cip_handle *h);
int cip_set_scaling_packed(cip_handle *h, const double *packedF);       /* host pointer */
int cip_set_scaling_identity(cip_handle *h);                            /* F = I (src/ConicIP.jl:704) */
/* nt_scaling on the device (src/ConicIP.jl:589-605, :165-210): F from (v, s); also
 * writes lambda = F v (src/ConicIP.jl:735) when lambda_out != NULL. */
int cip_set_scaling_from_iterate_dev(cip_handle *h, const double *v, const double *s, double *lambda_out);
int cip_get_scaling_packed(cip_handle *h, double *packedF);             /* host pointer (tests) */
/* assemble + factor the KKT system for the current scaling.  Asynchronous on the handle's stream: nothing waits for
 * the GPU.  The pivot flag is read back into pinned host memory behind the factorisation and resolved by
 * cip_check_factor, by the host-pointer solves (which are synchronous anyway) and by the *_dev solves: those WAIT for
 * the flag until one factorisation of the handle has been seen clean (the factorisation that meets a bad pivot is the
 * first one: LPs, singular Q), afterwards they resolve it only if the read-back has already landed and go ahead
 * speculatively otherwise.  When the resolving call has to redo the factorisation (a bad pivot: the regularised
 * re-factorisation described below; a give-up of the fused panel chain: see cip_debug_chain_giveup) and solves were
 * enqueued speculatively on the first one, it returns CIP_E_RETRY "repeat them": the handle now holds the good factor,
 * repeat those solves (cip_check_factor after cip_factor rules that out).  If the regularised re-factorisation fails too
 * the resolving call returns CIP_E_SINGULAR. */
int cip_factor(cip_handle *h);
/* wait for the factorisation and report its status: CIP_OK or CIP_E_SINGULAR */
int cip_check_factor(cip_handle *h);
/* Static regularisation of the quasi-definite LDL' (K + delta diag(+1.. -1..), delta = rel * max|K_ii|).  Default:
 * rel = 0 and automatic = 1 -- the first factorisation that meets a zero / non-finite / wrong-sign pivot (singular S:
 * LPs, free variables with singular Q; the reference's pivoting LU / QR, src/kktsolvers.jl:24,:231,:295, has no such
 * restriction) is redone with rel = 1e-13 per row (delta_i = rel * max_j |K_ij|), which then stays on; solve3x3 then
 * refines against the true operator (a few extra back-solves) so that callers see the unregularised solution. */
int cip_set_regularization(cip_handle *h, double rel, int automatic);
int cip_get_regularization(cip_handle *h, double *rel, int *times_switched_on);

/* ---- level 3: solve3x3(x, y, z) -> (a, b, c)  (src/ConicIP.jl:688; src/kktsolvers.jl:37-50, :324-330)
 *   Q a + G' b - A' c = x ;  G a = y ;  A a + F'F c = z */
int cip_solve3x3(cip_handle *h, const double *x, const double *y, const double *z,
                 double *a, double *b, double *c);                       /* host pointers */
int cip_solve3x3_dev(cip_handle *h, const double *x, const double *y, const double *z,
                     double *a, double *b, double *c);                   /* device pointers */

/* ---- the 2x2 plugin form  solve2x2(y, w) -> (dy, dw)  (src/ConicIP.jl:450-466; src/kktsolvers.jl:297-302;
 * what `pivot`, src/kktsolvers.jl:316-349, wraps):  [Q + A'(F'F)^-1 A, G'; G, 0][dy; dw] = [y; w].
 * Served by the factor of the Schur route (CIP_E_UNSUPPORTED on the full-3x3 route). */
int cip_solve2x2(cip_handle *h, const double *y, const double *w, double *dy, double *dw);      /* host pointers */
int cip_solve2x2_dev(cip_handle *h, const double *y, const double *w, double *dy, double *dw);  /* device pointers */

/* ---- many right-hand sides for one factor: nrhs calls of solve3x3 / solve2x2 in one.  Blocks are column-major with the
 * leading dimension = their row count: X n x nrhs, Y p x nrhs, Z m x nrhs (A, Bo, C likewise; for solve2x2 Y n x nrhs,
 * W p x nrhs).  The factor is resolved, the calls are speculative and return CIP_E_RETRY, n_solve grows (by nrhs) and C may
 * alias Z exactly as for the single calls; nrhs == 1 gives the single call's bits.  The dense A / A' products and the LDL'
 * sweeps run over 64 columns at a time (L read once per sweep for all of them); a regularised factor is refined per column.
 * nrhs < 0, or a NULL block the single call needs (X, A; Y, Bo when p > 0; Z, C when m > 0): CIP_E_INVALID before anything
 * is enqueued; nrhs == 0: no-op.  cip_solve2x2_many*: CIP_E_UNSUPPORTED on the full-3x3 route. */
int cip_solve3x3_many(cip_handle *h, int nrhs, const double *X, const double *Y, const double *Z,
                      double *A, double *Bo, double *C);                 /* host pointers */
int cip_solve3x3_many_dev(cip_handle *h, int nrhs, const double *X, const double *Y, const double *Z,
                          double *A, double *Bo, double *C);             /* device pointers */
int cip_solve2x2_many(cip_handle *h, int nrhs, const double *Y, const double *W, double *DY, double *DW);      /* host */
int cip_solve2x2_many_dev(cip_handle *h, int nrhs, const double *Y, const double *W, double *DY, double *DW);  /* device */

/* ---- the 4x4 -> 3x3 reduction of solve4x4 (src/ConicIP.jl:684-692), device pointers.
 * r and dz are 4-block vectors (y[n], w[p], v[m], s[m]) stored contiguously.
 * Aliasing: dz may be r itself (an in-place call), and dz may start inside or behind the s block of r (dz >= r + n + p + m):
 * every block of dz is then written after the blocks of r it covers have been read.  Such a call gives the bits of a call with
 * separate buffers; it always takes the element-wise path (with R cones only, separate buffers take two fused kernels that
 * gather r across threads while dz is written -- the same bits, fewer launches).  This holds with R and Q cones and with S cones
 * below order 133 (their kernels stage a cone before they write it), with and without regularisation; it is not promised for
 * larger S cones.  Any other overlap of dz and r is not checked and is undefined: blocks of r would be overwritten before they
 * are read.  lambda must not overlap dz. */
int cip_solve4x4_dev(cip_handle *h, const double *lambda, const double *r, double *dz);

/* ---- block operator / cone algebra on the device (device pointers, length m) */
int cip_apply_F_dev(cip_handle *h, int mode, const double *x, double *out);              /* src/blockmatrices.jl:173-200 */
int cip_cone_prod_dev(cip_handle *h, const double *x, const double *y, double *out);     /* src/ConicIP.jl:637-665 */
int cip_cone_div_dev(cip_handle *h, const double *x, const double *y, double *out);      /* src/ConicIP.jl:607-635: solve y o out = x */
int cip_maxstep_dev(cip_handle *h, const double *x, const double *d, double scale, double *alpha_host); /* src/ConicIP.jl:571-587; d == NULL -> the `nothing` variant; steps along d*scale */
/* the pair the interior-point loop always asks for together (src/ConicIP.jl:708-709, :881-882, :927-928): alpha_host2[0] =
 * maxstep(x1, d1 * scale), alpha_host2[1] = maxstep(x2, d2 * scale), one wait; with S cones of order 133..256 the two sides run
 * side by side on two streams.  Same values as two cip_maxstep_dev calls. */
int cip_maxstep_pair_dev(cip_handle *h, const double *x1, const double *d1, const double *x2, const double *d2, double scale,
                         double *alpha_host2);
int cip_cone_identity_dev(cip_handle *h, double *e);                                     /* src/ConicIP.jl:559-565 */

/* ---- vector helpers for a device-resident driver loop (device pointers) */
int cip_gemv_dev(cip_handle *h, int which, int trans, double alpha, const double *x, double beta, double *y);
/* out_host[i] = dot(x_i[0:len_i], y_i[0:len_i]); pointer arrays live on the host */
int cip_dots_dev(cip_handle *h, int count, const double *const *x, const double *const *y,
                 const int *len, double *out_host);
int cip_axpby_dev(cip_handle *h, int len, double alpha, const double *x, double beta, double *y); /* y = alpha x + beta y */

/* ---- the whole interior-point loop of conicIP (src/ConicIP.jl:468-939) driven natively: every vector stays in
 * HBM, the host sees scalars only.  Same options and defaults as the reference's keyword
 * arguments (src/ConicIP.jl:498-509); a negative infeasTol / refinementThreshold selects the reference's derived
 * default (optTol, optTol/1e7).  c[n], b[m], d[p] and the outputs y[n], w[p], v[m] are host pointers.
 * trace (optional, trace_cap rows of CIP_TRACE_COLS doubles): Iter, mu, rDu, rPr, rCp, pobj, dobj, alpha, sigma. */
#define CIP_STATUS_NONE       0
#define CIP_STATUS_OPTIMAL    1   /* :Optimal    src/ConicIP.jl:786 */
#define CIP_STATUS_INFEASIBLE 2   /* :Infeasible src/ConicIP.jl:815-818 */
#define CIP_STATUS_UNBOUNDED  3   /* :Unbounded  src/ConicIP.jl:847-850 */
#define CIP_STATUS_ABANDONED  4   /* :Abandoned  src/ConicIP.jl:936 */
#define CIP_STATUS_ERROR      5   /* :Error      src/ConicIP.jl:870-873 */
#define CIP_TRACE_COLS 9
typedef struct cip_options {
    double optTol, DTB, infeasTol, refinementThreshold;
    int maxRefinementSteps, maxIters, verbose;
} cip_options;
typedef struct cip_result {          /* src/ConicIP.jl:384-398 (Solution) */
    int status, iter;
    double mu, prFeas, duFeas, muFeas, pobj, dobj;
    int n_factor, n_solve, trace_rows;
    double wall_s;
} cip_result;
int cip_conicip(cip_handle *h, const double *c, const double *b, const double *d, const cip_options *opt,
                double *y, double *w, double *v, cip_result *res, double *trace, int trace_cap);

/* ---- batches of independent problems on one GPU (BASELINE config 5).  A batch is an array of ordinary handles,
 * each on its own HIP stream; cip_batch_handle(b, i) is the "leading problem index": every entry point above works
 * on it.  cip_conicip_many / cip_batch_conicip keep `in_flight` interior-point loops running at once (one host
 * thread each); pointer arrays have one entry per problem (b / d / w / v arrays may be NULL when m or p is 0). */
typedef struct cip_batch cip_batch;
int cip_batch_create(int count, const cip_problem *probs, cip_batch **out);
int cip_batch_destroy(cip_batch *b);
int cip_batch_size(const cip_batch *b);
cip_handle *cip_batch_handle(cip_batch *b, int i);
int cip_batch_conicip(cip_batch *b, const double *const *c, const double *const *bvec, const double *const *d,
                      const cip_options *opt, double *const *y, double *const *w, double *const *v, cip_result *res,
                      int in_flight);
/* problems in, solutions out: `in_flight` host threads, each re-loading ONE handle (cip_update_problem) on its own
 * stream with the next problem of the queue -- level-1 upload of one problem overlaps the loops of the others */
int cip_conicip_problems(int count, const cip_problem *probs, const double *const *c, const double *const *bvec,
                         const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                         double *const *v, cip_result *res, int in_flight);
/* the same, in LOCK-STEP: the problems must have identical shape (n, m, p, cone list, route, dense-or-CSR A, dense-or-CSR Q with the same nnz) and no S
 * cone of matrix order >= 133; they advance through the loop together, every step ONE launch with the problem index in the grid (groups of up
 * to 64).  Results are bit-identical to cip_conicip on each problem run with the same solve block (lock-step handles use
 * min(cip_set_solve_block_max, cip_lockstep_solve_block_for(B)): a standalone handle of order >= 1024 sums its triangular solves in wider blocks unless
 * cip_set_solve_block_max(that value) is called first -- the difference is rounding).  Returns CIP_E_UNSUPPORTED (nothing written) when
 * the batch does not qualify -- fall back to cip_conicip_problems.  A problem whose factorisation meets a zero or wrong-sign pivot in
 * the static order (every LP with a free variable, singular Q with free variables) needs the regularised factorisation.  With
 * cip_set_lockstep_regularize(0), the default, it leaves the group and is solved by the one-problem loop afterwards; with
 * cip_set_lockstep_regularize(1) it stays: the group regularises its matrix and refines its solves under a mask of its own, with
 * the launches and the bits of the one-problem loop.  Either way a problem whose panel chain gave up an in-launch wait leaves.
 * The number of non-zeros of a CSR A or Q, and the mat-vec form a CSR Q's longest row selects, are part of the shape unless
 * cip_set_lockstep_ragged(1) has been called: then problems that differ in them share a group (its slabs are laid out for the
 * group's largest CSR arrays; every problem's Q mat-vec runs in its own form), with the same bits per problem. */
int cip_conicip_lockstep(int count, const cip_problem *probs, const double *const *c, const double *const *bvec,
                         const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                         double *const *v, cip_result *res);
/* ANY mix of problems: those that share a shape with at least one other problem of the batch (and qualify for lock-step)
 * advance together, shape group by shape group; the others go through cip_conicip_problems' thread pool (`in_flight`
 * threads).  Per problem the result is that of the entry point it went through; cip_lockstep_stats adds up over the groups.
 * The bins follow cip_conicip_lockstep's notion of shape: with cip_set_lockstep_ragged(1) CSR matrices of differing numbers of
 * non-zeros fall into one bin, with 0 (the default) each number is a bin of its own.
 * (The reference solves one problem per conicIP call, src/ConicIP.jl:472-480: a batch is N independent calls.) */
int cip_conicip_mixed(int count, const cip_problem *probs, const double *const *c, const double *const *bvec,
                      const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                      double *const *v, cip_result *res, int in_flight);
/* the arena of the last lock-step group is kept for the next call (allocation of several GB is slow); this frees it */
int cip_release_cached_memory(void);
/* diagnostics of the calling thread's last cip_conicip_lockstep: {groups, problems, problems that left their group} */
int cip_lockstep_stats(int *out3);
/* 1: problems that need the regularised factorisation stay in their lock-step group (see cip_conicip_lockstep); 0 (default): they
 * leave it.  Process-wide; returns the previous value; any other argument only queries. */
int cip_set_lockstep_regularize(int on);
/* 1: problems of one shape (n, m, p, cone list, route, dense-or-CSR A, dense-or-CSR Q) whose CSR matrices differ in their
 * numbers of non-zeros, or whose CSR Q take different mat-vec forms, share a lock-step group; 0 (default): they do not
 * (cip_conicip_lockstep: CIP_E_UNSUPPORTED, nothing written; cip_conicip_mixed: thread pool).  Process-wide; returns the
 * previous value; any other argument only queries. */
int cip_set_lockstep_ragged(int on);
/* the calling thread's last cip_conicip_lockstep / cip_conicip_mixed: how many problems were switched to the regularised factorisation
 * inside their group (summed over the groups, like cip_lockstep_stats; its third entry counts only the problems that still left) */
int cip_lockstep_regularized(int *count);
/* a lock-step call of at least 2 x 8 problems of one shape runs as k groups (default 2) SIDE BY SIDE, each on its own host thread and stream (the
 * groups fill each other's launch-latency gaps; per problem nothing changes: same kernels, same solve block, same bits).  k = 1: one
 * group after the other (the form up to round 5).  Also CIP_LOCKSTEP_SPLIT.  Process-wide; returns the previous value (k < 1: query).
 * With k > 1 a call that cip_conicip_lockstep refuses with CIP_E_UNSUPPORTED for a slab-layout reason found inside a group (CSR arrays
 * in device memory with differing numbers of non-zeros, with cip_set_lockstep_ragged(0) only: with 1 such arrays share a group) may
 * already have written other groups' results. */
int cip_set_lockstep_split(int k);
int cip_conicip_many(cip_handle *const *handles, int count, const double *const *c, const double *const *bvec,
                     const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                     double *const *v, cip_result *res, int in_flight);

/* ---- batches of SMALL problems, one workgroup per problem (csrc/small.hip).  Every entry point above pays a launch chain per
 * interior-point iteration whatever the problem size (cip_conicip_lockstep: 97 launches and 3 host read-backs per iteration of an
 * 8-problem shard, groups of at most 64).  Here a problem whose KKT matrix of order n + p <= CIP_SMALL_MAX_N fits the LDS of one
 * compute unit is one 256-thread workgroup: per iteration the call issues at most 2 launches and 1 host read-back WHATEVER count is,
 * plus 2 launches (upload gather, initial point) and 1 read-back (the iterates) per call; cip_small_stats reports what ran.
 * Taken: the Schur route; dense Q, A and G, as host or device pointers as `flags` says (the same for every problem of a call); R and Q
 * cones of any dimension; n + p <= CIP_SMALL_MAX_N, m <= CIP_SMALL_MAX_M; m == 0 and p == 0; all problems of a call of one n, m, p and
 * cone list; any count >= 0 (0: no-op).  Anything else (an S cone, a CSR A, CIP_FLAG_Q_CSR, the full 3x3 route, a larger problem,
 * differing shapes): CIP_E_UNSUPPORTED with cip_last_error() naming the rule, nothing written and nothing allocated.  Argument errors
 * (a NULL array or vector, bad dimensions, cones that do not cover m, a leading dimension below its row count): CIP_E_INVALID before
 * any allocation.
 * The algorithm, the options and every field of cip_result are cip_conicip's (same loop, same verdicts: the per-iteration verdict is
 * the one host function every loop of the library calls; n_factor and n_solve as cip_conicip counts them; wall_s: the call's wall
 * time; verbose prints nothing per problem); the iterates differ from the other paths' in rounding only.  A problem's bits do not
 * depend on count, on its index in the batch or on the run.  The call owns its stream and its device memory, is synchronous and
 * frees everything on every path.
 * A problem whose factorisation meets a zero, non-finite or wrong-sign pivot (positive expected on the first n, negative on the last p:
 * LPs, singular Q with free variables) cannot be finished by the kernels -- there is no regularised factor in them: after the loop
 * all such problems are solved from the start by cip_conicip_mixed, and their results are that call's, bit for bit.
 * When it pays, as measured on one MI355X against cip_conicip_mixed on the same problems (dense QPs, m = 2n, wall time with the
 * upload; DESIGN_LOG.md, "Small problems, one workgroup each"): at n <= 64 from the smallest count measured on (64 problems: 2.3 to
 * 4.1 times the problems per second; 8192 problems: 26 times at n = 16, 7 to 8 times at n = 64); at n = 120 from about a thousand
 * problems on (1024: 1.5 to 1.9 times, 8192: 2.1 to 2.5 times) -- with 64 problems of n = 120 it is level or LOSES (0.8 to 1.1 times):
 * 64 workgroups leave most of the chip idle. */
#define CIP_SMALL_MAX_N 128    /* n + p */
#define CIP_SMALL_MAX_M 1024
/* CIP_OK when cip_conicip_small takes a problem of this description, else CIP_E_UNSUPPORTED (or CIP_E_INVALID) with cip_last_error()
 * naming the rule; no device is touched */
int cip_conicip_small_fits(const cip_problem *prob);
/* arguments and results as cip_conicip_lockstep */
int cip_conicip_small(int count, const cip_problem *probs, const double *const *c, const double *const *bvec,
                      const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                      double *const *v, cip_result *res);
/* of the calling thread's last cip_conicip_small: {problems finished by the kernels, problems handed to cip_conicip_mixed, kernel
 * launches, host read-backs} */
int cip_small_stats(int *out4);
/* HIP-event timing of the step kernel (k_small_step) for the calling thread's cip_conicip_small calls: enable = 1 / 0 switches it on /
 * off (any other value only queries); out2 (may be NULL) = {step launches timed, their total ms} of the last call.  Returns the
 * previous setting. */
int cip_small_step_time(int enable, double *out2);

/* ---- dense symmetric LDL' building blocks (device pointers), usable on their own.
 * K is N x N column-major with leading dimension ld >= N; only the lower triangle is
 * referenced.  N and ld must be multiples of 128 (pad with an identity block); K, workspace and rhs non-NULL -- else
 * CIP_E_INVALID before anything is enqueued.  Rows N..ld-1 of K are never touched.
 * cip_ldlt_factor_dev waits for the factorisation and stores its first bad pivot in *info_host (0: none; 1-based column;
 * info_host may be NULL); it returns CIP_E_RETRY when an in-launch wait of the fused panel chain gave up (see
 * cip_debug_chain_giveup): K then holds a partial factor and must be supplied again.
 * After a factorisation K holds L strictly below the diagonal, D on it and L' above it OUTSIDE the 128 x 128 diagonal blocks;
 * the upper triangle of the diagonal blocks is undefined.  The workspace size covers either mode of cip_set_solve_fused; the
 * mode in force at cip_ldlt_factor_dev must still be in force at its cip_ldlt_solve_dev calls, and the solve-block limit
 * (cip_set_solve_block_max) must not change between the sizing call, the factorisation and its solves. */
int cip_ldlt_workspace_bytes(int N, size_t *bytes);
int cip_ldlt_factor_dev(void *hip_stream, double *K, int N, int ld, void *workspace, int *info_host);
int cip_ldlt_solve_dev(void *hip_stream, const double *K, int N, int ld, const void *workspace, double *rhs);
/* nrhs right-hand sides at once: B is N x nrhs (leading dimension ldb >= N), solved in place; rows N..ldb-1 are never touched.
 * scratch: device memory of cip_ldlt_solve_many_scratch_bytes(N, nrhs) bytes (at most 64 columns' worth, whatever nrhs).
 * Same rules as cip_ldlt_solve_dev, plus nrhs >= 0, ldb >= N, and B, scratch non-NULL when nrhs > 0 -- else CIP_E_INVALID
 * before anything is enqueued; nrhs == 0: no-op.  nrhs == 1 is cip_ldlt_solve_dev (same bits); otherwise every column gets the
 * same bits whatever nrhs and the other columns are (fp64 MFMA products, fixed reduction order). */
int cip_ldlt_solve_many_scratch_bytes(int N, int nrhs, size_t *bytes);
int cip_ldlt_solve_many_dev(void *hip_stream, const double *K, int N, int ld, const void *workspace,
                            void *scratch, double *B, int ldb, int nrhs);
/* C(lower or full) += alpha * A * B'   (A: M x K, B: N x K, all column-major; M,N % 128 == 0, K % 16 == 0, K > 0;
 * lda >= M, ldb >= N, ldc >= M; A, B, C non-NULL; lower_only needs M == N and leaves the 128 x 128 tiles above the diagonal
 * untouched -- else CIP_E_INVALID before anything is enqueued) */
int cip_gemm_nt_dev(void *hip_stream, int M, int N, int K, double alpha,
                    const double *A, int lda, const double *B, int ldb, double *C, int ldc, int lower_only);

/* ---- rank-revealing (column-pivoted) Householder QR and the pre-solve's `imcols` on top of it (device pointers), usable on
 * their own.  M is len x cnt column-major with leading dimension ld.  Argument rules: len, cnt >= 0; ld >= max(len, 1); stop, eps
 * >= 0 and finite; M, workspace (and b, rows_host for cip_imcols_dev) non-NULL when len * cnt > 0; k_host / nrows_host /
 * consistent_host non-NULL -- else CIP_E_INVALID before anything is enqueued; len * cnt == 0: no-op with k = 0 (no rows,
 * consistent).  A NaN or Inf entry (or one whose square overflows): CIP_E_INVALID "non-finite entry".  Both calls wait for their
 * result.  The same input gives the same bits on every run.
 * workspace for cip_qrcp_dev / cip_imcols_dev (the latter includes a working copy of M) */
int cip_qrcp_workspace_bytes(int len, int cnt, size_t *bytes);
int cip_imcols_workspace_bytes(int len, int cnt, size_t *bytes);
/* M is overwritten with LAPACK geqp3's result layout: columns physically permuted, R on and above the diagonal, the reflector
 * tails (leading 1 implicit) below it in the first k columns; rows len..ld-1 are never read or written.  Column j of the result
 * is column piv_host[j] of the input (0-based).  The factorisation stops at the first step whose largest remaining column norm
 * is <= stop (every later |R_jj| would be): *k_host = steps done, columns k.. then hold the updated, unfactored remainder.
 * piv_host[cnt], rdiag_host[min(len,cnt)] (the diagonal of R, first *k_host entries valid), tau_dev[min(len,cnt)] (device) may
 * be NULL.  16-byte accesses when ld is even and M 16-byte aligned; same bits either way. */
int cip_qrcp_dev(void *hip_stream, double *M, int len, int cnt, int ld, double stop, void *workspace,
                 double *tau_dev, int *piv_host, double *rdiag_host, int *k_host);
/* imcols of the reference (src/preprocessor.jl:10-28) for the rows of A (cnt rows of length len), handed over as
 * M = A' column-major -- i.e. A in row-major order; M and b (device, cnt entries) are NOT modified.  A is scaled by 1 / ||A||_F,
 * the QR runs with stop = eps on a working copy, the rows whose |R_jj| > eps are kept, x = A[R,:] \ b[R] is the minimum-norm
 * solution Q1 R1^-T b_R with one refinement step, and the system counts as consistent when ||A x - b||_inf < eps over all rows.
 * rows_host[cnt]: sorted 0-based kept rows, *nrows_host of them (also when inconsistent); *consistent_host 0/1; *resid_host =
 * ||A x - b||_inf of the scaled system (may be NULL).  An empty or all-zero A: no rows, consistent (the reference's empty-R
 * branch). */
int cip_imcols_dev(void *hip_stream, const double *M, int len, int cnt, int ld, const double *b, double eps,
                   void *workspace, int *rows_host, int *nrows_host, int *consistent_host, double *resid_host);

/* ---- the pre-solve's full-row-rank certificate (cipkkt/preprocess.py: _full_row_rank) on the device, in one self-contained call.
 * M = [B_1 B_2 ...] has n rows and is handed over as column blocks.  *certified = 1: M CERTAINLY has n independent rows by the
 * reference's criterion (src/preprocessor.jl:19-23), sigma_min(M) / ||M||_F >= thr = max(100 eps, 1e-6); 0: not certified -- the
 * caller runs the rank-revealing QR; it never means "rank deficient".  The n x n Gram matrix sum B_i B_i' is formed on the device
 * (dense blocks through the fp64 MFMA GEMM, CSR blocks entry by entry: O(nnz), never densified), tau I is subtracted, tau =
 * (thr^2 + 2 (L + n) 2^-53) ||M||_F^2 with L the number of columns of M, and the unpivoted LDL' must have only positive pivots
 * (Sylvester).  Rounding can only cost a certificate, never grant one.  *fro2 = ||M||_F^2 (a fixed-order sum), *shift = tau; either
 * may be NULL; the same input gives the same bits on every run.
 * flags: CIP_FLAG_DEVICE_PTRS -- the dense blocks are device pointers; the CSR arrays are host pointers unless it is set without
 * CIP_FLAG_CSR_HOST.  The call owns its device memory and its streams: it works on the null stream, waits for its result and frees
 * everything on every path.
 * Argument rules, each CIP_E_INVALID naming the block and the entry before any device allocation: n, nblocks, cols >= 0; eps finite
 * and >= 0; certified non-NULL; a block with cols > 0 (and n > 0) has exactly one of the two forms, a dense one with ld >= n; CSR:
 * rowptr[0] == 0, a monotone row pointer, indices in [0, cols), no entry stored twice (checked on the host in O(nnz); device-resident
 * arrays are copied back first).  n == 0 or no column at all: not certified, fro2 = 0, CIP_OK.  A NaN or Inf entry (or a sum of
 * squares that overflows): CIP_E_INVALID "non-finite entry".  An all-zero M: not certified. */
/* one column block B of M = [B_1 B_2 ...]; every block has n rows */
typedef struct cip_cert_block {
    int cols;
    const double *dense; int ld;      /* column-major n x cols, ld >= max(n,1); or NULL for a CSR block */
    const int *rowptr; const int *colind; const double *val;   /* CSR of B: n+1 / nnz / nnz, 0-based */
} cip_cert_block;
int cip_rowrank_cert(int n, int nblocks, const cip_cert_block *blocks, double eps, int flags,
                     int *certified, double *fro2, double *shift);

/* ---- introspection (tests, bench) */
int cip_kkt_order(const cip_handle *h, int *N, int *N_padded);
int cip_get_kkt_matrix(cip_handle *h, double *K_host /* N_padded^2 */); /* assembled (before cip_factor) or factored */
int cip_assemble_only(cip_handle *h);                                   /* level-2 assembly without the factorisation */
/* stats: [0] factor calls, [1] solve calls, [2] last factor ms (assemble), [3] last factor ms (ldlt), [4] flops of last ldlt */
int cip_stats(cip_handle *h, double *out8);
int cip_set_timing(cip_handle *h, int enabled);
int cip_set_ldlt_outer_block(int nbo);    /* 0 = automatic (896 from order 4096 on, else 512); returns the knob's value */
/* tuning knob: widest block of the triangular solves' block-step form (128, 256, 512 or 1024; 0 = query).  Applies to
 * handles created afterwards; returns the previous value.  Lock-step batches use min(this, cip_lockstep_solve_block_for(B)) for their handles. */
int cip_set_solve_block_max(int b);
/* block steps of the triangular sweeps (also CIP_SOLVE_FUSED): 0 (default) = two launches per step (block product, then the
 * update of everything below / above); 1 = ONE launch per block step for solve blocks of at most 512 columns -- the neighbour
 * blocks X_J L_{J,J-1} / L_{J+1,J} X_J are formed with the block inverses at factorisation time, so a step depends on the
 * previous step's result only (sweeps 20 % faster, factorisation dearer: pays from about six solves per factorisation on);
 * 2 = for every block width.  Applies to handles created afterwards; the two forms differ in rounding.  On graded factors
 * (|L| up to 1e6) the one-launch form is the less accurate one: the pre-multiplied neighbours put |L_JJ||inv L_JJ| in front of
 * L_{J,J-1}, and the residual against the factor was measured at 30 to 1.4e4 times the substitution bound u |L||D||L'||x| and
 * 1.1e-14 to 1.4e-14 norm-wise, where the two-launch form stays at 1 to 3 times and below 3e-15 (DESIGN_LOG.md, "The LDL'
 * and its solves on graded matrices").  Returns the previous mode (other values: query). */
int cip_set_solve_fused(int mode);
/* the solve-block limit cip_conicip_lockstep gives the handles of a call of B problems in all (512 for B <= 8, else 256 -- chosen
 * from the size of the whole call, so the groups of 64 it is cut into all use the same one; never more than
 * cip_set_solve_block_max's value; CIP_LOCKSTEP_SOLVE_BLOCK overrides): a one-problem run with this limit
 * reproduces the call's iterates bit for bit */
int cip_lockstep_solve_block_for(int B);
/* panel chain of the serial schedule (also CIP_FUSE_DIAG, where any value but 0 selects 3): 3 (default) = one launch per
 * 128-column panel -- diagonal kernel, the previous panel's in-block update and this panel's TRSM, the TRSM following the
 * diagonal kernel micro-panel by micro-panel through a stage counter; 0 = three launches per panel.  Same factor bit for bit.
 * Process-wide; accepts 0 and 3, any other value only queries; returns the previous setting. */
int cip_set_ldlt_fused_chain(int on);
/* The fused panel chain waits INSIDE a launch for workgroups of the same launch (bounded: 2e9 ticks of the s_memtime counter, which
 * counts shader clock cycles -- about 0.8 s at the 2.4 GHz peak clock, longer at a lower clock -- then the factorisation reports
 * that the wait gave up).  On a GPU shared with other processes the
 * hardware scheduler can keep a launch's workgroups apart for longer than the wait expects (seen with eight processes on one MI355X).
 * Every path that runs the fused chain either falls back or reports it: a handle redoes the factorisation with the three-launch
 * chain -- no in-launch wait, same bits -- and keeps that chain (solves enqueued speculatively on the first one: CIP_E_RETRY, repeat
 * them); a problem of a lock-step group leaves the group and is solved alone; cip_ldlt_factor_dev returns CIP_E_RETRY; the
 * factorisations inside large S cones (order >= 133) always run on the three-launch chain.
 * TEST HOOK: the next `count` factorisations of the process that run the fused chain (directly or as the replay of a recorded
 * graph that holds it) report such a give-up.  n < 0: query; else n = count + 65536 * skip (+ kind bits): the `count` ones after
 * the next `skip` (count < 65536, skip < 4096).  Kind bits:
 *   + 2^28  they report a wrong-sign pivot at column 1 instead of a give-up
 *   + 2^29  POISON: besides the give-up, the factor is left as a real give-up can leave it -- the strictly-lower 64 x 64 block
 *           K[64:128, 0:64] is multiplied by 1 + 2^-20 (inside the N x N lower triangle at every order) and the solves follow
 *           it -- so that whoever ignores the give-up computes a measurably wrong answer
 *   + 2^30  the first factorisation on the three-launch chain after each give-up of the hook reports a wrong-sign pivot at
 *           column 1 (the redo meets a bad pivot)
 * Returns the previous count. */
int cip_debug_chain_giveup(int n);
/* how many factorisations of this handle were redone on the three-launch chain after such a give-up (-1: NULL handle) */
int cip_get_chain_fallbacks(cip_handle *h);
/* solve preparation (block inverses for the triangular sweeps, mirror image of L) of every solve block whose columns are final,
 * on a side stream beside the last panels of the factorisation instead of behind it (also CIP_SIDE_PREP; CIP_SIDE_PREP_FROM =
 * columns before the end from which it forks, default 2048).  1 (default) on, 0 off.  Same bits.  Returns the previous setting. */
int cip_set_ldlt_side_prep(int on);
/* Schur route, CSR A with one entry per row, R cones, no equalities, order a multiple of 128 (the box-QP family): cip_factor
 * copies only the first outer block's columns of Q into K; the first trailing update of the LDL' reads the rest from Q
 * itself (also CIP_LAZY_COPY=0).  Same factor bit for bit.  1 (default) on, 0 off; returns the previous setting. */
int cip_set_lazy_copy(int on);
/* S cones of order 133..256: the max-step's extreme eigenvalue (the reference's eigmin / eigmax, src/ConicIP.jl:272-303) by
   Lanczos (1: the plain three-term recurrence, stopped at the first convergence of the extreme Ritz value; CIP_LG_LANCZOS_REORTH=1
   adds full reorthogonalisation, the form until round 6) or by a full tridiagonalisation + Sturm multisection (0); < 0 only
   reads.  Returns the previous setting.  Same eigenvalue to ~1e-11 relative either way; for A/B runs and tests.
   2 (DEFAULT): Lanczos + INERTIA CERTIFICATE -- a Krylov method started from a fixed vector can in principle settle on an interior
   eigenvalue (no component along the extreme eigenvector); mode 2 checks with an LDL' of theta' I - A (theta' = theta + 1e-9 |T|)
   that no eigenvalue lies beyond the returned one and recomputes the verdict by the tridiagonalisation when the check fails
   (0.09 ms per iteration of config 4, 1 %; also CIP_LG_LANCZOS=2).  cip_sdp_lanczos_fallbacks: how often that happened on this handle.
   3 (self-test): as 2 with the bound on the wrong side of theta, so that every certificate fails and every verdict is the fallback's. */
int cip_set_sdp_lanczos(int on);
/* (S cones of order >= 133, NT scaling, src/ConicIP.jl:196-210: the one-sided Jacobi of svd(Lz'Ls) runs as one launch per phase.  Rounds
   3-5 also offered one persistent launch with in-launch block hand-offs behind cip_set_sdp_jacobi_stepped; that form was measured to
   come out with other bits about once in 800 / 4000 / 40000 scalings at order 1024 / 512 / 256, the cause was never found, and round 6
   REMOVED it together with its switch: no public knob of this library documents nondeterminism.) */
int cip_sdp_lanczos_fallbacks(cip_handle *h, int *count);
/* HIP-event timing of the LDL' trailing-update launches (bench.py roofline): enable, then read
 * out3 = [launches, total ms, total algorithmic flops (r(r+1)K per launch)].  enabled = 1: every launch of every factorisation;
 * enabled = k > 1: of every k-th factorisation, starting with the next one (an event pair costs the chain ~8 us: a sampled
 * profile perturbs the timed region a k-th as much); 0: off (drops the totals) */
int cip_profile_trailing(cip_handle *h, int enabled);
int cip_profile_get(cip_handle *h, double *out3);
/* the same for every factorisation the CALLING THREAD enqueues on handles without a profile of their own (the handles of
 * cip_conicip_lockstep live inside the call): flops count every live problem of a lock-step launch */
int cip_profile_trailing_thread(int enabled);
int cip_profile_thread_get(double *out3);
/* the same event-pair timing for the dominant kernels of the other configurations, per calling thread: slot 0 = the trailing
 * update (as above), 1 = Schur formation S = Q + (A'F^-1)(A'F^-1)' with a dense A (m n^2 flop per call; src/kktsolvers.jl:33-34,
 * :290), 2 = the one-sided Jacobi of a large S cone's NT scaling (src/ConicIP.jl:204; latency-bound, flops reported as 0) */
#define CIP_PROFILE_TRAILING 0
#define CIP_PROFILE_SYRK     1
#define CIP_PROFILE_JACOBI   2
int cip_profile_kernel_thread(int slot, int enabled);
int cip_profile_kernel_thread_get(int slot, double *out3);

#ifdef __cplusplus
}
#endif
#endif /* CIPKKT_H */
