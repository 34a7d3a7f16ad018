// The opaque handle behind the C ABI (one KKT system, resident on one GPU).
#pragma once
#include "cip_internal.h"
#include <vector>

struct cip_handle {
    int n = 0, m = 0, p = 0, ncones = 0, route = 0;
    int N = 0, Npad = 0;            // KKT order for the route, and padded to a multiple of 128
    int npad = 0, mpad = 0;         // n rounded up to 128, m rounded up to 16 (>= 16)
    int nq = 0, nqpad = 0;          // number of Q cones, rounded up to 16 (>= 16)
    hipStream_t stream = nullptr;
    int device = 0;
    // Device memory of the handle.  Every creation-time buffer is a member of ONE block, laid out by one function (api.hip:
    // cip_handle_layout) that is walked twice: over a null base it sizes the block, over the block it carves.  An ordinary handle
    // allocates its block; a handle of a lock-step batch borrows its slab of the batch's arena, where the same walk puts problem
    // z's buffers at problem 0's addresses + z * stride.  Buffers of first use (ref, c2x2, many, many_stage, drv) are allocations
    // of their own -- except in a slab, whose layout holds those the group needs (CIP_EXTRA_*).
    std::vector<void *> owned;      // every pointer cip_handle_alloc got from hipMalloc (the block, first-use buffers): what destruction frees
    bool in_slab = false;           // the block is a slab of a lock-step arena: not the handle's to free
    int ldlt_fused = 0;             // cip_ldlt_fused_for(Npad) when the handle was planned: both walks lay out the same LDL' workspace

    // ---- problem data, device resident for the lifetime of the handle (level 1)
    double *Q = nullptr;            // n x n, ld n            (dense Q only)
    // CSR Q (CIP_FLAG_Q_CSR): the whole symmetric matrix, columns of a row ascending (level 1 sorts them), no dense image and no
    // symv tables.  Q_wave: the mat-vec form chosen at level 1 from the longest row (api.hip: cip_mul_Q)
    bool Q_sparse = false;
    int Q_nnz = 0, Q_wave = 0;
    int *Q_rp = nullptr, *Q_ci = nullptr; double *Q_v = nullptr;
    double *symv_ws = nullptr;      // partial-sum tables of the symmetric mat-vec (n a multiple of 128, n >= 2048), else null
    bool A_sparse = false;
    bool A_one_per_row = false;     // CSR A with at most one entry per row (A = I, bound constraints): A'(F'F)^-1 A is diagonal for R cones
    double *kdiag = nullptr;        // n doubles: the Schur route's diagonal of K beyond the first outer block when the copy of Q is lazy
    int s4_fused = -1;              // solve4x4 takes the fused element-wise path (cip_all_r and CIP_S4_FUSED); -1: not looked at yet
    double *A = nullptr;            // m x n, ld m            (dense A only)
    double *At = nullptr;           // npad x mpad, ld npad   (dense A only; zero padded)  At[i + r*npad] = A[r,i]
    int A_nnz = 0;
    int *A_rp = nullptr, *A_ci = nullptr; double *A_v = nullptr;   // CSR of A  (m rows)
    int *T_rp = nullptr, *T_ci = nullptr; double *T_v = nullptr;   // CSR of A' (n rows)
    int *row_cone = nullptr;        // m ints: cone index of every row of A
    // CSR A with S cones (round 4): the rows of the S cones as a dense transposed block, and its scaled image (Schur route)
    double *AtS = nullptr, *WtS = nullptr; int mS = 0, mSpad = 0;     // npad x mSpad each, ld npad; cone c's rows at columns [aoff, aoff + dim)
    double *G = nullptr;            // p x n, ld p
    double *Gt = nullptr;           // n x p, ld n

    // host staging of the small tables and of the CSR arrays: asynchronous uploads read them after the call has returned
    std::vector<int> st_rp, st_ci, st_trp, st_tci, st_rowcone, st_sidx, st_small, st_bigq, st_ritems, st_packq;
    std::vector<double> st_av, st_tv;
    std::vector<int> st_qrp, st_qci; std::vector<double> st_qv;
    bool staging_live = false;

    // ---- cones / scaling (level 2 input)
    std::vector<ConeDesc> h_cones;
    std::vector<WorkItem> h_items;
    ConeSet cs = {};

    // ---- KKT matrix + factor (level 2 output)
    double *K = nullptr; long ldk = 0;
    double *Wt = nullptr;           // npad x mpad   At * F^-1           (dense-A Schur route)
    double *syrk_ws = nullptr; int syrk_n = 1, syrk_len = 0;   // split-K images of the Schur formation (few output tiles, long K: config 4)
    double *Gm = nullptr;           // npad x nqpad  rank-1 columns of the Q cones (sparse-A Schur route)
    void *ws_base = nullptr; LdltWorkspace ws = {};
    struct LdltSide *ldlt_side = nullptr;   // side stream + events of the overlapped solve preparation (ldlt.hip), created on first use
    bool assembled = false, factored = false;
    // static regularisation K + delta diag(+1 .. -1 ..), delta = reg_rel * max|K_ii|: 0 until a factorisation meets a
    // bad pivot (auto_reg), then kept for the lifetime of the handle; the loops' iterative refinement absorbs it
    double reg_rel = 0.0;
    bool auto_reg = true;
    int n_regularized = 0;
    int n_chain_fallbacks = 0;     // factorisations redone with the three-launch chain after an in-launch wait of the fused one gave up
    int x_zeroed = 0;               // block-inverse storage zero-initialised
    // pivot flag of the last factorisation: read back asynchronously into pinned host memory, resolved lazily
    // (api.hip: cip_factor_resolve) so that cip_factor never waits for the GPU
    int *info_host = nullptr;
    int info_seq = 0;                 // sequence number of the last factorisation's flag read-back (info_host[4] == info_seq: landed)
    bool info_pending = false;
    int spec_solves = 0;            // solves enqueued while the flag was still in flight
    // true once a factorisation of this handle has been resolved clean (or the regularised mode is on): until then the
    // *_dev solves WAIT for the pivot flag instead of going ahead speculatively -- the factorisation that meets a bad
    // pivot is almost always the first one (LPs, singular Q with free variables), and a caller doing factor -> solve*_dev
    // must not get rc 0 and a solution of a broken factor
    bool pivots_verified = false;

    // ---- scratch
    double *rhs = nullptr;          // Npad
    double *mt1 = nullptr, *mt2 = nullptr, *mt3 = nullptr;   // m-vectors
    double *nt1 = nullptr;          // n-vector
    double *pt1 = nullptr;          // p-vector
    double *dot_scratch = nullptr;
    double *stage = nullptr;        // device staging for the host-pointer entry points (StageView, one column)
    double *ref = nullptr;          // right-hand side / residual / correction of the refinement inside solve3x3 (regularised factor only)
    double *c2x2 = nullptr;         // m-vector: discarded third component of a regularised 2x2 solve
    // many right-hand sides (cip_solve3x3_many*), allocated on first use, sized for chunks of 64 columns: the Npad x 64 right-hand
    // side block, two m x 64 blocks (t, u of the Schur route), the Bs x 64 scratch of the sweeps; host staging of the host-pointer calls
    double *many = nullptr, *many_stage = nullptr;
    double *drv = nullptr;          // vectors of the native interior-point loop (cip_conicip), allocated on first use

    // ---- hipGraphs of the two launch-bound inner loops of small systems (opt-in, CIP_GRAPH=1; graph_run below)
    hipGraphExec_t gx_factor = nullptr, gx_solve = nullptr;
    // what the recorded factorisation baked in besides the handle's fixed pointers: where the first trailing update reads
    // its C operand (ws.lazyC: Q while the copy is lazy, else null).  A replay under another state would read stale data
    // (ADVICE r3): factor_enqueue drops the graph and records a new one when it differs.
    const double *gx_factor_lazyC = nullptr;
    int gx_factor_unfused = 0;     // ws.unfused when gx_factor was recorded
    bool gx_factor_fused = false;  // gx_factor holds a fused panel chain (the give-up test hook fires on its replays)
    int graph_state = 0;            // 0 undecided, 1 in use, -1 off (null stream, large system, capture failed, CIP_GRAPH=0)

    // ---- stats
    double n_factor = 0, n_solve = 0, ms_assemble = 0, ms_ldlt = 0, flops_ldlt = 0;
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
};

int cip_lazy_copy_set(int on);       // assemble.hip
int cip_scatter_AtS(cip_handle *h);   // assemble.hip: CSR A with S cones: their rows of A' as a dense block (h->AtS)
int cip_assemble(cip_handle *h, bool lazy_ok = false);     // assemble.hip; lazy_ok: the caller factors right away (see assemble_schur)
// Relative size of the automatic regularisation.  Miles problem 3 under the reference's 10 scalings (test/runtests.jl:
// 618-637), iterations to :Optimal (oracle: 15 16 16 15 21 29 30 | 20 29 32): 1e-9 -> one false :Unbounded; 1e-11 -> 11 16 16
// 15 21 26 24 | 20 28 27; 1e-13 -> 16 16 16 15 21 29 29 | 21 29 32.  The refinement inside solve3x3 is what makes the
// small value work.  CIP_AUTO_REG overrides (api.hip: cip_factor_resolve; lockstep.hip: GroupLoop).
#define CIP_AUTO_REG 1e-13

// assemble.hip: the assembled K of every problem of the thread's mask becomes K + E, E_ii = +-rel * max_j |K_ij| (what cip_assemble does
// behind the assembly while h->reg_rel > 0; a lock-step group calls it under the mask of its regularised problems)
int cip_regularize(cip_handle *h, double rel);
int cip_mul_Q(cip_handle *h, double alpha, const double *x, double beta, double *y, bool symv = true);   // api.hip: y = alpha Q x + beta y, dense or CSR Q
int cip_mul_A(cip_handle *h, double alpha, const double *x, double beta, double *y);    // solve.hip: y = alpha A x + beta y (m), dense or CSR A
int cip_mul_At(cip_handle *h, double alpha, const double *x, double beta, double *y);   // solve.hip: y = alpha A' x + beta y (n)
inline bool cip_all_r(const cip_handle *h) { return h->m > 0 && h->nq == 0 && !h->cs.has_S; }   // every cone is an R cone: F = diag(packed scaling)
int cip_handle_alloc(cip_handle *h, void **out, size_t bytes);      // api.hip: an allocation of the handle's own
// api.hip, level 1 in parts (a lock-step group sizes its slabs from problem 0's plan before anything exists on the device):
// the host half; the layout of the device block (null base: its size); the device half inside a slab.
// extras: what an ordinary handle allocates on first use and a lock-step handle holds in its slab, in this order
#define CIP_EXTRA_DRIVER 1u         // h->drv: the vectors of the interior-point loop (cip_driver_bytes)
#define CIP_EXTRA_REFINE 2u         // h->ref, h->c2x2: the refined solves of a regularised factor
int cip_plan(const struct cip_problem *pr, hipStream_t stream, cip_handle **out);
// Entries the layout reserves for the index / value arrays of a CSR A (and of its transpose) and of a CSR Q.  NULL: the handle's own
// numbers of non-zeros -- every ordinary handle, whose layout keeps its bytes.  A ragged lock-step group passes its largest ones, so that
// every problem's arrays sit at problem 0's offsets; a handle uploads and checks (cip_update_problem) its own nnz, and the tail above
// it is never read: every kernel walks the row pointers.
struct CipCsrCap { size_t A_nnz, Q_nnz; };
size_t cip_handle_layout(CipLayout L, cip_handle *h, unsigned extras, const CipCsrCap *cap = nullptr);
int cip_create_in_slab(cip_handle *h, const struct cip_problem *pr, char *slab, size_t cap, unsigned extras, const CipCsrCap *csr_cap = nullptr);
// What a branch of the host code asks about the CSR CONTENT of "the problem": inside a lock-step group, whose host code runs once on
// problem 0's handle, a statement about every live problem of the group (the thread's mask); else about the handle.
inline bool cip_grp_A_one_per_row(const cip_handle *h) {     // every one of them has at most one entry per row
    return cip_in_batch() ? (cip_tl_bz.mask & ~cip_tl_bz.a_one_per_row) == 0 : h->A_one_per_row;
}
inline bool cip_grp_Q_nonempty(const cip_handle *h) {        // at least one of them stores an entry
    return cip_in_batch() ? (cip_tl_bz.mask & cip_tl_bz.q_nonempty) != 0 : h->Q_nnz > 0;
}
size_t cip_driver_bytes(const cip_handle *h);                        // driver.hip: vectors of the interior-point loop
// api.hip: resolve the pivot flag of the last factorisation (wait = false: only if its read-back has already landed)
int cip_factor_resolve(cip_handle *h, bool wait);

// api.hip: roctx ranges (no-ops when the marker library is not present)
void cip_range_push(const char *name);
void cip_range_pop(void);
struct CipRange { explicit CipRange(const char *n) { cip_range_push(n); } ~CipRange() { cip_range_pop(); } };

// ---- views of the handle's packed scratch buffers (8-byte granular, the staging view 16); each layout function sizes the allocation and
// carves for every user
#define CIP_MANY_CHUNK 64
struct Vec3 { double *x, *y, *z; };            // an (n, p, m) triple of k columns each
inline Vec3 cip_take3(CipLayout &L, const cip_handle *h, size_t k = 1, size_t g = 8) { return Vec3{L.take<double>(h->n * k, g), L.take<double>(h->p * k, g), L.take<double>(h->m * k, g)}; }
// h->stage (cap = 1), h->many_stage (cap = CIP_MANY_CHUNK): an input and an output triple of `cap` columns each; a chunk of fewer
// columns uses the front of every block, so the layout is one and the same for every chunk.  16-byte granular: the blocks stand in for a
// device caller's vectors, and the mat-vecs sum in another order (vecops.hip: k_gemv_t) when theirs is not 16-byte aligned -- the
// refined solve of a regularised factor multiplies by its own outputs
struct StageView { Vec3 in, out; };
inline size_t stage_layout(CipLayout L, const cip_handle *h, size_t cap, StageView *v) {
    v->in = cip_take3(L, h, cap, 16);
    v->out = cip_take3(L, h, cap, 16);
    return L.bytes();
}
// h->ref: right-hand side, residual and correction of the refined solve, 8 spare doubles behind each
struct RefView { Vec3 rhs, res, cor; };
inline size_t ref_layout(CipLayout L, const cip_handle *h, RefView *v) {
    for (Vec3 *b : {&v->rhs, &v->res, &v->cor}) { *b = cip_take3(L, h); L.take<double>(8, 8); }
    return L.bytes();
}
// h->many, CIP_MANY_CHUNK columns each: the Npad-row right-hand sides R, the m-row blocks T and U of the Schur route, the sweeps' scratch S
struct ManyView { double *R, *T, *U, *S; };
inline size_t many_layout(CipLayout L, const cip_handle *h, ManyView *v) {
    const size_t c = CIP_MANY_CHUNK;
    *v = ManyView{L.take<double>(c * h->Npad, 8), L.take<double>(c * h->m, 8), L.take<double>(c * h->m, 8), L.take<double>(c * h->ws.Bs, 8)};
    return L.bytes();
}

// ---- hipGraph replay of a handle's fixed launch sequences (api.hip: the factorisation; solve.hip: the triangular sweeps): `enqueue`
// runs as it is, or -- where api.hip's cip_graph_wanted says so -- is recorded once into *exec (cip_launch) and replayed
bool cip_graph_wanted(cip_handle *h);
template <class F>
static int graph_run(cip_handle *h, hipGraphExec_t *exec, F &&enqueue, bool *replayed = nullptr) {
    if (cip_in_batch() || !cip_graph_wanted(h) || h->timing || h->ws.prof) return enqueue();
    if (!*exec) {
        CipGraphBuilder b = {nullptr, nullptr, false, true};
        if (hipGraphCreate(&b.graph, 0) != hipSuccess) { (void)hipGetLastError(); h->graph_state = -1; return enqueue(); }
        cip_tl_builder = &b;
        const int rc = enqueue();                // records kernel nodes, launches nothing
        cip_tl_builder = nullptr;
        hipError_t ei = hipErrorUnknown;
        if (rc == 0 && b.ok && b.have_last) ei = hipGraphInstantiate(exec, b.graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(b.graph);
        if (ei != hipSuccess) { (void)hipGetLastError(); *exec = nullptr; h->graph_state = -1; return enqueue(); }
    }
    CIP_HIP_CHECK(hipGraphLaunch(*exec, h->stream));
    if (replayed) *replayed = true;
    return 0;
}
