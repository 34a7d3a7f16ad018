// Lock-step batches: B independent problems of IDENTICAL shape (n, m, p, cone list, route, dense / CSR A with the same
// number of non-zeros, dense / CSR Q with the same number of non-zeros -- or, with cip_set_lockstep_ragged(1), any numbers: see
// lockstep_group) advance through the interior-point loop of src/ConicIP.jl:468-939 together, every step of the
// loop ONE launch whose grid carries the problem index in blockIdx.z (BASELINE config 5: 64 dense QPs of n = 2048;
// SURVEY 7.4(5) "batch dimension").
//
// Why: a small system is a chain of tiny dependent launches (n = 2048: ~1500 launches and 16.8 ms of serial kernel time
// per problem, 30 % of it the single-workgroup diagonal kernel).  Host threads with one stream each (batch.hip) keep only
// ~3.4 kernels executing at once -- the streams are launch-latency-bound and share four hardware queues.  In lock-step
// the diagonal kernel of 64 problems is one launch of 64 workgroups, the TRSM one launch of 64 x 30, and the host pays
// one launch and one read-back per step for all of them.
//
// How: the device block of problem z's handle is slab z of one arena, carved by the walk that sized it (api.hip: cip_handle_layout),
// so that problem z's pointers are problem 0's + z * stride.  The library's host code then runs ONCE, on problem 0's
// handle, under a thread-local batch context (cip_internal.h: cip_launch_b appends {stride, mask} to every launch and
// multiplies grid.z by B; kernels shift their pointer arguments and drop out when their problem's mask bit is clear).
// The iteration is cip_conicip's own (driver.hip: Loop::run); the kernels, their grids in x / y and their arithmetic are
// those of the one-problem path: results are bit-identical to cip_conicip on each problem (tests/test_gpu_lockstep.py).
// Per-problem control flow is the mask: problems that have reached a final status stop taking part; the refinement loop
// runs on the subset that still needs it.  What differs is the policy on pivot flags (GroupLoop below): a problem whose
// factorisation meets a bad pivot (it would switch to the regularised factorisation: LPs, singular Q with free
// variables) is taken out of the lock-step group and solved afterwards by cip_conicip on its own handle -- or, with
// cip_set_lockstep_regularize(1), switched to the regularised factorisation INSIDE its group: the group keeps a mask of
// its regularised problems, regularises their K behind the assembly and refines their solves (solve.hip: cip_solve3x3_dev).
//
// Not supported in lock-step (the caller falls back to the thread pool of batch.hip): S cones of order >= 133 (their
// chip-wide kernels own one workspace), problems of differing shape.
#include "cip_driver.h"
#include "cip_batch_front.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace cipdrv;

thread_local CipBatchCtx cip_tl_bz = {1, 0, 1ull, nullptr, nullptr, 0ull};

namespace {

struct BatchScope {           // activates the batch context for the calling thread; restores on exit
    CipBatchCtx saved;
    explicit BatchScope(const CipBatchCtx &c) : saved(cip_tl_bz) { cip_tl_bz = c; }
    ~BatchScope() { cip_tl_bz = saved; }
};

// the four pivot-flag words of a factorisation into slots 32..35 of the problem's row of the gather buffer (slots 0..31
// carry the dot products: the flags come back with the same device-to-host copy)
#define INFO_SLOT 32
#ifndef CIP_LOCKSTEP_SPLIT_MIN_DEFAULT
#define CIP_LOCKSTEP_SPLIT_MIN_DEFAULT 8    // smallest group a split may produce (2 x 4 problems side by side LOSE: 15.3 -> 16 ms per pass)
#endif
#ifndef CIP_LOCKSTEP_SPLIT_DEFAULT
#define CIP_LOCKSTEP_SPLIT_DEFAULT 2        // (round 6, measured: see cip_conicip_lockstep)
#endif
__global__ void k_gather_info(const int *info, double *gather, CipBatch cb) {
    CIP_BATCH_GUARD(cb);
    CIP_BO1(cb, info);
    if (threadIdx.x < 4) gather[blockIdx.z * CIP_GATHER + INFO_SLOT + threadIdx.x] = (double)info[threadIdx.x];
}

static thread_local bool g_stats_accumulate = false;     // cip_conicip_mixed: the groups' statistics add up
// cip_set_lockstep_ragged: 1 = the nnz of a CSR A / Q and a CSR Q's mat-vec form are not part of the shape (process-wide; a call reads it once)
std::atomic<int> g_ragged{0};
// ragged: the numbers of non-zeros of CSR matrices do not count (dense beside CSR still does)
bool same_shape(const cip_problem &a, const cip_problem &b, bool ragged) {
    if (!same_dims(a, b) || a.route != b.route || (a.A == nullptr) != (b.A == nullptr)) return false;
    // CSR A: the slab layout depends on the number of non-zeros -- part of the shape when the row pointers can be read here
    // (host memory); device-resident row pointers are caught by the slab-layout check of lockstep_group instead
    auto host_rowptr = [](const cip_problem &q) {
        return q.A == nullptr && q.m > 0 && q.A_rowptr && ((q.flags & CIP_FLAG_CSR_HOST) || !(q.flags & CIP_FLAG_DEVICE_PTRS));
    };
    if (!ragged && host_rowptr(a) && host_rowptr(b) && a.A_rowptr[a.m] != b.A_rowptr[b.m]) return false;
    // Q: dense or CSR, and a CSR Q's number of non-zeros under the same rule
    if ((a.flags & CIP_FLAG_Q_CSR) != (b.flags & CIP_FLAG_Q_CSR)) return false;
    auto host_q_rowptr = [](const cip_problem &q) {
        return (q.flags & CIP_FLAG_Q_CSR) && q.Q_rowptr && ((q.flags & CIP_FLAG_CSR_HOST) || !(q.flags & CIP_FLAG_DEVICE_PTRS));
    };
    if (!ragged && host_q_rowptr(a) && host_q_rowptr(b) && a.Q_rowptr[a.n] != b.Q_rowptr[b.n]) return false;
    return true;
}

// Up to four arenas are kept between calls (a bench or a service solves batch after batch of the same shape, possibly from several
// host threads at once; hipMalloc / hipFree of several GB cost up to 0.6 s and synchronise the device).
// cip_release_cached_memory() frees them.
struct ArenaCache {
    std::mutex mu;
    struct Slot { char *ptr; size_t bytes; int device; };
    std::vector<Slot> slots;
} g_cache;
// *cap: the allocation's true size (a recycled arena may be larger than asked for; it goes back into the cache with that size)
int arena_acquire(size_t bytes, char **out, size_t *cap) {
    int dev = 0;
    CIP_HIP_CHECK(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lk(g_cache.mu);
        int best = -1;                                       // the smallest cached arena that fits
        for (int i = 0; i < (int)g_cache.slots.size(); ++i) {
            const auto &sl = g_cache.slots[i];
            if (sl.device == dev && sl.bytes >= bytes && (best < 0 || sl.bytes < g_cache.slots[best].bytes)) best = i;
        }
        if (best >= 0) {
            *out = g_cache.slots[best].ptr; *cap = g_cache.slots[best].bytes;
            g_cache.slots.erase(g_cache.slots.begin() + best);
            return 0;
        }
        // nothing fits: the cached arenas of this device make room (a larger batch follows a smaller one)
        for (int i = (int)g_cache.slots.size() - 1; i >= 0; --i)
            if (g_cache.slots[i].device == dev) { (void)hipFree(g_cache.slots[i].ptr); g_cache.slots.erase(g_cache.slots.begin() + i); }
    }
    CIP_HIP_CHECK(hipMalloc((void **)out, bytes));
    *cap = bytes;
    return 0;
}
void arena_release(char *ptr, size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_cache.mu);
    if (g_cache.slots.size() >= 4) {                         // full: the smallest one goes
        int small = 0;
        for (int i = 1; i < (int)g_cache.slots.size(); ++i) if (g_cache.slots[i].bytes < g_cache.slots[small].bytes) small = i;
        (void)hipFree(g_cache.slots[small].ptr);
        g_cache.slots.erase(g_cache.slots.begin() + small);
    }
    g_cache.slots.push_back({ptr, bytes, dev});
}
struct Group {
    int B = 0;
    char *arena = nullptr; size_t arena_bytes = 0;
    size_t stride = 0;
    double *gather_dev = nullptr, *gather_host = nullptr;
    hipStream_t stream = nullptr;
    std::vector<cip_handle *> h;
    ~Group() {
        for (cip_handle *x : h) if (x) cip_destroy(x);
        if (stream) (void)hipStreamDestroy(stream);
        if (arena) arena_release(arena, arena_bytes);      // the handles' stream was drained by cip_destroy
        if (gather_host) (void)hipHostFree(gather_host);
    }
};

// groups, problems, problems that left their group, problems regularised inside their group (last call of this thread)
#define N_STATS 4
thread_local int g_last_stats[N_STATS] = {0, 0, 0, 0};
// cip_set_lockstep_regularize: 1 = a problem whose factorisation meets a bad pivot stays in its group (process-wide; a group reads it once)
std::atomic<int> g_keep_regularized{0};

// The group's policy on pivot flags: assembly + LDL' of every problem of the mask, the four flag words of each problem copied
// into its row of the gather buffer (they ride on the next read-back, normally the dots'), and the problems whose fused panel
// chain gave up an in-launch wait taken out of the group (ejected: solved alone afterwards).  A problem that met a bad pivot is
// ejected too (keep == false), or joins `reg` (keep): the group's problems on the regularised factorisation, for good -- what
// cip_factor_resolve (api.hip) does to one handle, per problem of the group.  `reg` lives with the group: the side-by-side groups of
// a split call have their own.  A group of ONE problem is no batch for the kernels (no mask): there bit 0 of `reg` is the
// handle's own reg_rel, which cip_assemble and the solves read as they do for a stand-alone handle.
struct GroupLoop final : Loop {
    Group &G;
    std::vector<char> ejected;
    const bool keep;
    const double rel;
    unsigned long long reg = 0;
    GroupLoop(Group &g, bool keep_) : Loop(g.h[0], g.B), G(g), ejected(g.B, 0), keep(keep_), rel(cip_env_double("CIP_AUTO_REG", CIP_AUTO_REG)) {}
    // assembly, regularisation of the regularised ones, LDL': the problems of mk (the thread's mask on entry, and again on return)
    int factor_under(unsigned long long mk) {
        int rc;
        const unsigned long long rg = mk & reg;
        h->assembled = h->factored = false;
        if (!cip_in_batch()) {
            h->reg_rel = rg ? rel : 0.0;
            if ((rc = cip_assemble(h, true))) return rc;
        } else {
            // (a regularised matrix cannot take the lazy copy, and the copy is per launch: nobody takes it while one of them is in)
            h->reg_rel = 0.0;
            if ((rc = cip_assemble(h, rg == 0))) return rc;
            if (rg) {
                cip_tl_bz.mask = rg;
                rc = cip_regularize(h, rel);
                cip_tl_bz.mask = mk;
                if (rc) return rc;
            }
        }
        if ((rc = cip_ldlt_factor(h->stream, h->K, h->Npad, h->ldk, h->ws))) return rc;
        h->factored = true; h->info_pending = false;
        return 0;
    }
    int factor() override { return factor_under(cip_tl_bz.mask); }
    int ride_pivots() override {       // (under the mask the factorisation ran under)
        cip_launch_b(k_gather_info, dim3(1), dim3(64), 0, h->stream, (const int *)h->ws.info, G.gather_dev);
        CIP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    int fetch() {
        CIP_HIP_CHECK(hipMemcpyAsync(G.gather_host, G.gather_dev, sizeof(double) * (size_t)B * CIP_GATHER, hipMemcpyDeviceToHost, h->stream));
        return cip_wait(h->stream);
    }
    const double *flags(int z) const { return G.gather_host + (size_t)z * CIP_GATHER + INFO_SLOT; }
    // what every factorisation's flags may say, bad pivots aside.  Returns > 0: the problem has left the group
    int common_flags(int z) {
        const double *gi = flags(z);
        if (gi[1] != 0.0) { cip_set_error("LDL': a triangular sweep bailed out (problem %d)", z); return -1; }
        // gi[3]: an in-launch wait of the fused panel launch gave up -- a GPU shared with other processes can keep a launch's
        // workgroups off the chip for longer than the bound.  The problem leaves the group like one with a bad pivot and is
        // solved alone afterwards, on the three-launch chain (no in-launch wait, same bits)
        if (gi[3] != 0.0) {
            G.h[z]->ws.unfused = 1; G.h[z]->n_chain_fallbacks += 1; h->ws.unfused = 1;      // (h: the group's launches follow problem 0's workspace -- three launches per panel from here on)
            eject(z);
            return 1;
        }
        return 0;
    }
    void eject(int z) { ejected[z] = 1; active &= ~(1ull << z); reg &= ~(1ull << z); publish(); }
    void publish() { cip_tl_bz.reg_mask = reg; }
    // a regularised factor: a wrong-sign pivot -- |d| ~ delta, rounding decides its sign -- is harmless (the refined solves work
    // against the true operator); a zero / non-finite one ends the problem with :Error, as it does alone (driver.hip: OneProblem)
    void regularised_flags(int z) {
        if (flags(z)[2] == 0.0) return;
        outcome[z].status = CIP_STATUS_ERROR;
        active &= ~(1ull << z);
    }
    int take_pivots(bool fresh) override {
        // (a group of ONE problem is no batch for the kernels: its dot products do not go through the gather buffer)
        int rc;
        if ((!fresh || !cip_in_batch()) && (rc = fetch())) return rc;
        unsigned long long joining = 0;
        for (int z = 0; z < B; ++z) {
            if (!((active >> z) & 1ull)) continue;
            if ((rc = common_flags(z)) < 0) return CIP_E_HIP;
            if (rc > 0) continue;
            if ((reg >> z) & 1ull) regularised_flags(z);
            else if (flags(z)[0] != 0.0) { if (keep) joining |= 1ull << z; else eject(z); }
        }
        if (!joining) return 0;
        // the problems that have just met their first bad pivot: assembly, regularisation and LDL' again, for them alone, and their
        // flags back.  No solve has been enqueued on the factorisation being replaced (Loop::run takes the flags first), and the redo
        // is not a factorisation of its own in n_factor -- as for one problem (api.hip: cip_factor_resolve)
        reg |= joining; publish();
        const unsigned long long mk = cip_tl_bz.mask;
        cip_tl_bz.mask = joining;
        rc = factor_under(joining);
        if (!rc) rc = ride_pivots();
        if (!rc) rc = fetch();
        cip_tl_bz.mask = mk;
        if (rc) return rc;
        for (int z = 0; z < B; ++z) {
            if (!((joining >> z) & 1ull)) continue;
            if ((rc = common_flags(z)) < 0) return CIP_E_HIP;
            if (rc == 0) regularised_flags(z);
        }
        return 0;
    }
};

}   // namespace

// Solve-block limit of a lock-step call's handles, chosen from the size of the WHOLE call (count), not per group of 64: every
// problem of one cip_conicip_lockstep call is solved with the same block, so a problem's bits do not depend on which group
// it lands in (72 problems = 64 + 8: both groups take 256).  Never above the process-wide limit.
extern "C" int cip_lockstep_solve_block_for(int B) {
    // groups of up to 8 problems: 512 (the sweeps are launch chains on a mostly idle chip: half the block steps; 8 problems of
    // order 2048, 256 / 512 / 1024: 16.75 / 16.55 / 17.8 ms per pass); larger groups: 256 (the doubling GEMMs of a wider
    // block are real work for 64 problems).  CIP_LOCKSTEP_SOLVE_BLOCK overrides both.
    const int want = cip_env_int("CIP_LOCKSTEP_SOLVE_BLOCK", B <= 8 ? 512 : 256), glob = cip_solve_block_max_set(0);
    return want < glob ? want : glob;
}
// One lock-step group (B <= CIP_BATCH_MAX problems of the same shape).  Returns 0 and fills res / y / w / v of every
// problem, or an error code (nothing meaningful written).
// ragged (cip_set_lockstep_ragged(1), read by the call): the CSR matrices of the group's problems may differ in their numbers of
// non-zeros.  Every problem is planned first (host work; CSR arrays in device memory cost the read-back of rowptr[m] they always did),
// the slab is laid out for the group's largest A_nnz and Q_nnz, and every handle is carved with those capacities: problem z's arrays
// sit at problem 0's offsets + z * stride, each handle uploads its own nnz, the tail above it is never read (every kernel walks the
// row pointers).  What the host code, run once on problem 0's handle, would read from problem 0's CSR content becomes a statement
// about the group (CipBatchCtx: a_one_per_row, q_nonempty, q_wave) -- also for groups of equal nnz, where the patterns still differ.
static int lockstep_group(int B, int call_count, bool ragged, const cip_problem *probs, const double *const *c, const double *const *b,
                          const double *const *d, const cip_options *opt_in, double *const *y, double *const *w,
                          double *const *v, cip_result *res) {
    const auto t_start = std::chrono::steady_clock::now();
    static const bool timing = cip_env_set("CIP_LOCKSTEP_TIMING");
    auto since = [&]() { return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    double t_plan = 0, t_arena = 0, t_create = 0, t_loop = 0;
    const cip_options o = resolve_options(opt_in);
    const int n = probs[0].n, m = probs[0].m, p = probs[0].p;
    struct ExitTimer {            // reports what the destructors behind it (handles, arena) cost
        bool on; std::chrono::steady_clock::time_point t0;
        ~ExitTimer() { if (on) fprintf(stderr, "lockstep group: tear-down %.2f ms\n", 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); }
    };
    ExitTimer exit_timer{false, std::chrono::steady_clock::now()};
    Group G;
    G.B = B;
    int rc;
    CIP_HIP_CHECK(hipStreamCreateWithFlags(&G.stream, hipStreamNonBlocking));
    // solve-block limit of the group's handles (see ldlt.hip: cip_solve_block)
    struct SolveBlockScope {
        int saved;
        explicit SolveBlockScope(int B_) : saved(cip_tl_solve_block_max) { cip_tl_solve_block_max = cip_lockstep_solve_block_for(B_); }
        ~SolveBlockScope() { cip_tl_solve_block_max = saved; }
    } solve_block_scope(call_count);
    // ---- slab size: the walk that will carve problem 0's slab, over a null base (under the group's solve-block limit, like the carve)
    const bool keep_reg = g_keep_regularized.load() != 0;            // (read once: the group's slab and its policy must agree)
    // the loop's vectors, and what a regularised factor's refined solves would allocate on first use: part of every slab
    const unsigned extras = CIP_EXTRA_DRIVER | (keep_reg ? CIP_EXTRA_REFINE : 0u);
    G.h.assign(B, nullptr);
    CipCsrCap cap = {0, 0};
    for (int z = 0; z < B; ++z) {
        if ((rc = cip_plan(&probs[z], G.stream, &G.h[z]))) return rc;
        if (z == 0 && G.h[0]->cs.nlarge > 0) return refuse_chipwide_s_cone();      // (the backstop: has_chipwide_s_cone looked at the description)
        cap.A_nnz = std::max(cap.A_nnz, (size_t)G.h[z]->A_nnz);
        cap.Q_nnz = std::max(cap.Q_nnz, (size_t)G.h[z]->Q_nnz);
    }
    const CipCsrCap *csr_cap = ragged ? &cap : nullptr;      // (not ragged: every handle's own nnz, which must then agree with problem 0's)
    const size_t slab = cip_handle_layout(nullptr, G.h[0], extras, csr_cap);
    t_plan = since();
    G.stride = slab_stride(slab);
    const size_t gather_bytes = sizeof(double) * (size_t)B * CIP_GATHER;
    G.arena_bytes = G.stride * (size_t)B + gather_bytes;
    if ((rc = arena_acquire(G.arena_bytes, &G.arena, &G.arena_bytes))) return rc;
    G.gather_dev = (double *)(G.arena + G.stride * (size_t)B);
    CIP_HIP_CHECK(hipHostMalloc((void **)&G.gather_host, gather_bytes, hipHostMallocDefault));
    t_arena = since();
    // (refused before anything is carved or uploaded.  Device-resident CSR arrays with another number of non-zeros: same_shape could not look)
    for (int z = 1; z < B; ++z) {
        if (cip_handle_layout(nullptr, G.h[z], extras, csr_cap) != slab) {
            cip_set_error("lock-step batch: problem %d does not fit problem 0's slab layout", z);
            return CIP_E_UNSUPPORTED;
        }
        // not ragged: the group's Q mat-vec is one form for all, a CSR Q whose longest row asks for the other one (other bits) cannot follow
        if (!ragged && G.h[z]->Q_wave != G.h[0]->Q_wave) {
            cip_set_error("lock-step batch: the CSR Q of problem %d takes another mat-vec form than problem 0's", z);
            return CIP_E_UNSUPPORTED;
        }
    }
    CipBatchCtx ctx = {B, (long)G.stride, full_mask(B), G.gather_dev, G.gather_host, 0ull};
    for (int z = 0; z < B; ++z) {
        cip_handle *hz = G.h[z];
        if ((rc = cip_create_in_slab(hz, &probs[z], G.arena + G.stride * (size_t)z, G.stride, extras, csr_cap))) return rc;
        if (hz->A_one_per_row) ctx.a_one_per_row |= 1ull << z;
        if (hz->Q_nnz > 0) ctx.q_nonempty |= 1ull << z;
        if (hz->Q_wave) ctx.q_wave |= 1ull << z;
    }
    t_create = since();
    hipStream_t s = G.stream;
    BatchScope scope(ctx);
    GroupLoop L(G, keep_reg);
    if ((rc = L.run(c, b, d, o, res, nullptr, 0))) return rc;
    if (timing) { (void)hipStreamSynchronize(s); t_loop = since(); }
    // ---- results of the lock-step problems
    const Vec4 &zv = L.V.z;
    for (int z = 0; z < B; ++z) {
        if (L.ejected[z]) continue;
        const size_t off = G.stride * (size_t)z;
        CIP_HIP_CHECK(hipMemcpyAsync(y[z], (char *)zv.y + off, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        if (p > 0) CIP_HIP_CHECK(hipMemcpyAsync(w[z], (char *)zv.w + off, sizeof(double) * p, hipMemcpyDeviceToHost, s));
        if (m > 0) CIP_HIP_CHECK(hipMemcpyAsync(v[z], (char *)zv.v + off, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    }
    CIP_HIP_CHECK(hipStreamSynchronize(s));
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    if (timing)
        fprintf(stderr, "lockstep group B=%d n=%d: plan %.2f ms, arena %.2f, create %.2f, loop %.2f (%d iterations), download %.2f; slab %.1f MB\n",
                B, n, t_plan, t_arena - t_plan, t_create - t_arena, t_loop - t_create, L.iters, 1e3 * wall - t_loop, G.stride / 1048576.0);
    for (int z = 0; z < B; ++z) {
        if (L.ejected[z]) continue;
        apply_certificate(L.outcome[z], n, m, p, y[z], p > 0 ? w[z] : nullptr, m > 0 ? v[z] : nullptr);
        res[z].wall_s = wall;            // the group's wall time: the problems finished together
    }
    g_last_stats[0] += 1; g_last_stats[1] += B;
    for (int z = 0; z < B; ++z) g_last_stats[2] += L.ejected[z] ? 1 : 0;
    g_last_stats[3] += __builtin_popcountll(L.reg);                  // (a problem that left the group afterwards is no longer in it)
    exit_timer.on = timing; exit_timer.t0 = std::chrono::steady_clock::now();
    // ---- problems that left the group: the one-problem loop on their own handle (regularised factorisation and all)
    {
        BatchScope single(CipBatchCtx{1, 0, 1ull, nullptr, nullptr, 0ull});
        for (int z = 0; z < B; ++z) {
            if (!L.ejected[z]) continue;
            cip_handle *hz = G.h[z];
            hz->assembled = hz->factored = false; hz->info_pending = false; hz->reg_rel = 0.0; hz->n_regularized = 0;
            if ((rc = cip_conicip(hz, c[z], m > 0 ? b[z] : nullptr, p > 0 ? d[z] : nullptr, opt_in, y[z], p > 0 ? w[z] : nullptr,
                                  m > 0 ? v[z] : nullptr, &res[z], nullptr, 0)))
                return rc;
        }
    }
    return 0;
}

// groups of a large lock-step call that run side by side (see cip_conicip_lockstep); k < 1 only reads; returns the previous value
static CipKnob g_lockstep_split{[] { const int v = cip_env_int("CIP_LOCKSTEP_SPLIT", CIP_LOCKSTEP_SPLIT_DEFAULT); return v < 1 ? 1 : (v > 8 ? 8 : v); }};
int cip_lockstep_split_set(int k) { return g_lockstep_split.set(k, [](int v) { return v >= 1 && v <= 8; }); }
extern "C" int cip_set_lockstep_split(int k) { return cip_lockstep_split_set(k); }

// Problems in, solutions out, in lock-step groups of up to 64.  CIP_E_UNSUPPORTED (nothing written): the problems differ
// in shape or hold S cones -- use cip_conicip_problems.
extern "C" int cip_conicip_lockstep(int count, const cip_problem *probs, const double *const *c, const double *const *b,
                                    const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                                    double *const *v, cip_result *res) {
    CIP_TRY(check_batch_call("cip_conicip_lockstep", {count, probs, nullptr, c, b, d, opt, y, w, v, res}, CHECK_PROBLEM0));
    if (count == 0) return 0;
    const bool ragged = g_ragged.load() != 0;                  // (read once: the shape check and every group's slab must agree)
    for (int i = 1; i < count; ++i)
        if (!same_shape(probs[0], probs[i], ragged)) { cip_set_error("lock-step batch: problem %d differs in shape from problem 0", i); return CIP_E_UNSUPPORTED; }
    if (has_chipwide_s_cone(probs[0])) return refuse_chipwide_s_cone();
    if (cip_tl_builder) { cip_set_error("lock-step batch inside a graph recording"); return CIP_E_INVALID; }
    if (!g_stats_accumulate) for (int &q : g_last_stats) q = 0;
    auto range = [&](int i0, int i1) -> int {                // groups of up to 64 over [i0, i1), one after the other, on the calling thread
        for (int g0 = i0; g0 < i1; g0 += CIP_BATCH_MAX) {
            const int B = (i1 - g0 < CIP_BATCH_MAX) ? (i1 - g0) : CIP_BATCH_MAX;
            const int rc = lockstep_group(B, count, ragged, probs + g0, c + g0, b ? b + g0 : nullptr, d ? d + g0 : nullptr, opt, y + g0,
                                          w ? w + g0 : nullptr, v ? v + g0 : nullptr, res + g0);
            if (rc) return rc;
        }
        return 0;
    };
    // Round 6: a large call as TWO (CIP_LOCKSTEP_SPLIT = k: k) lock-step groups side by side, each driven by its own host thread on its
    // own stream.  A group's loop alternates latency-bound launch chains (the panel chain, the triangular sweeps: most of the chip idle)
    // with throughput-bound ones (trailing updates, symv) and three host round trips per iteration; two groups fill each other's
    // gaps.  Measured first with two PROCESSES sharing one GPU (round 5: 64 problems of order 2048, 8819 against 7971 KKT solves/s for
    // one rank); this is the same overlap inside one process.  Per problem nothing changes: the solve block follows the size of the
    // whole call, every kernel is the group-size-independent code the bit-identity tests pin (tests/test_gpu_lockstep.py).
    // Measured (profiles/r6/lockstep_split.txt, problems of order 2048, ms per pass, one group -> two side by side): 64 problems 77.3-79.4 ->
    // 72.4-74.4 (8000 -> 8500-8650 KKT solves/s), 32: 44.9 -> 40.4-41.5, 24: 32.5 -> 30.8-31.7, 16: 25.2 -> 23.7-24.4; 8 problems as
    // 2 x 4 LOSE (15.3 -> 15.5-16.9: each panel launch owns whole CUs -- 160 KB of LDS per workgroup -- and two latency-bound chains only
    // get in each other's way), as do three or four groups (64 as 4 x 16: 77.2-78.8).  Hence: two groups, none smaller than 8.
    int nsplit = cip_lockstep_split_set(0);
    static const int split_min = [] { const int k = cip_env_int("CIP_LOCKSTEP_SPLIT_MIN", CIP_LOCKSTEP_SPLIT_MIN_DEFAULT); return k < 1 ? 1 : k; }();
    while (nsplit > 1 && count / nsplit < split_min) --nsplit;
    if (nsplit <= 1) return range(0, count);
    int device = 0;
    CIP_HIP_CHECK(hipGetDevice(&device));
    std::vector<int> rcs(nsplit, 0);
    std::vector<std::string> errs(nsplit);
    std::vector<int> st(N_STATS * (size_t)nsplit, 0);
    std::vector<std::thread> th;
    const int per = (count + nsplit - 1) / nsplit;
    for (int t = 0; t < nsplit; ++t)
        th.emplace_back([&, t] {
            (void)hipSetDevice(device);
            for (int &q : g_last_stats) q = 0;
            const int i0 = t * per, i1 = (t + 1) * per < count ? (t + 1) * per : count;
            rcs[t] = i0 < i1 ? range(i0, i1) : 0;
            if (rcs[t]) errs[t] = cip_last_error();
            for (int q = 0; q < N_STATS; ++q) st[N_STATS * t + q] = g_last_stats[q];
        });
    for (auto &x : th) x.join();
    for (int t = 0; t < nsplit; ++t)
        for (int q = 0; q < N_STATS; ++q) g_last_stats[q] += st[N_STATS * t + q];
    for (int t = 0; t < nsplit; ++t)
        if (rcs[t]) { cip_set_error("%s", errs[t].c_str()); return rcs[t]; }
    return 0;
}

// Any mix of problems.  The ones that share a shape with at least one other problem of the batch (and qualify for
// lock-step: no chip-wide S cone) advance together, shape group by shape group in order of first appearance; the rest go
// through the thread pool (`in_flight` threads).  Results per problem are those of cip_conicip_lockstep / cip_conicip_problems.
extern "C" int cip_conicip_mixed(int count, const cip_problem *probs, const double *const *c, const double *const *b,
                                 const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                                 double *const *v, cip_result *res, int in_flight) {
    const BatchCall call = {count, probs, nullptr, c, b, d, opt, y, w, v, res};
    CIP_TRY(check_batch_call("cip_conicip_mixed", call, CHECK_EVERY));
    if (count == 0) return 0;
    const bool ragged = g_ragged.load() != 0;
    std::vector<std::vector<int>> bins;                         // bins[k][0] is the representative
    for (int i = 0; i < count; ++i) {
        size_t k = 0;
        for (; k < bins.size(); ++k)
            if (same_shape(probs[bins[k][0]], probs[i], ragged)) break;
        if (k == bins.size()) bins.emplace_back();
        bins[k].push_back(i);
    }
    for (int &q : g_last_stats) q = 0;
    struct Acc { Acc() { g_stats_accumulate = true; } ~Acc() { g_stats_accumulate = false; } } acc;
    std::vector<int> rest;
    auto run = [&](const std::vector<int> &idx, bool lock) -> int {
        SubBatch sub(call, idx);
        const BatchCall g = sub.view();
        const int rc = lock ? cip_conicip_lockstep(g.count, g.probs, g.c, g.b, g.d, g.opt, g.y, g.w, g.v, g.res)
                            : cip_conicip_problems(g.count, g.probs, g.c, g.b, g.d, g.opt, g.y, g.w, g.v, g.res, in_flight);
        if (rc == 0 || !lock) sub.scatter();                    // the thread pool writes a status for every problem it reached
        return rc;
    };
    for (const auto &bin : bins) {
        if (bin.size() < 2 || has_chipwide_s_cone(probs[bin[0]])) { rest.insert(rest.end(), bin.begin(), bin.end()); continue; }
        const int rc = run(bin, true);
        // a bin that turns out not to qualify (same shape, yet a different slab layout: CSR arrays in device memory with differing
        // numbers of non-zeros, or a CSR Q of another mat-vec form -- neither with cip_set_lockstep_ragged(1)) has written nothing: its problems join the thread pool's share instead of failing the batch
        if (rc == CIP_E_UNSUPPORTED) { rest.insert(rest.end(), bin.begin(), bin.end()); continue; }
        if (rc) return rc;
    }
    if (!rest.empty()) {
        std::sort(rest.begin(), rest.end());
        const int rc = run(rest, false);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int cip_release_cached_memory(void) {
    std::lock_guard<std::mutex> lk(g_cache.mu);
    for (auto &sl : g_cache.slots) (void)hipFree(sl.ptr);
    g_cache.slots.clear();
    return 0;
}

// diagnostics of the calling thread's last cip_conicip_lockstep: {groups, problems, problems that left their group}
extern "C" int cip_lockstep_stats(int *out3) {
    if (!out3) return CIP_E_INVALID;
    for (int i = 0; i < 3; ++i) out3[i] = g_last_stats[i];
    return 0;
}

// 1: a problem whose factorisation meets a bad pivot is switched to the regularised factorisation inside its lock-step group; 0 (default):
// it leaves the group and is solved alone.  Process-wide; any other argument only queries.  Returns the previous value
extern "C" int cip_set_lockstep_regularize(int on) {
    const int prev = g_keep_regularized.load();
    if (on == 0 || on == 1) g_keep_regularized.store(on);
    return prev;
}
// 1: problems whose CSR matrices differ in their numbers of non-zeros (or whose CSR Q take different mat-vec forms) share a lock-step
// group; 0 (default): the nnz is part of the shape.  Process-wide; any other argument only queries.  Returns the previous value
extern "C" int cip_set_lockstep_ragged(int on) {
    const int prev = g_ragged.load();
    if (on == 0 || on == 1) g_ragged.store(on);
    return prev;
}
// the calling thread's last cip_conicip_lockstep / cip_conicip_mixed: problems switched to the regularised factorisation inside their group
extern "C" int cip_lockstep_regularized(int *count) {
    if (!count) return CIP_E_INVALID;
    *count = g_last_stats[3];
    return 0;
}
