// What the batch entry points (batch.hip, lockstep.hip, small.hip) do in front of and behind the interior-point loop, once: the call
// as a struct, the null-argument rules, the gather of a sub-batch, the shape rule, the chip-wide S cone test, the slab stride, the
// fresh result and the worker pool.  Host code only.
#pragma once
#include "cip_internal.h"
#include "../../include/cipkkt.h"
#include <atomic>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

namespace cipdrv {

struct BatchCall {                 // what every batch entry point receives (cip_conicip_many: handles instead of probs)
    int count;
    const cip_problem *probs; cip_handle *const *handles;
    const double *const *c, *const *b, *const *d; const cip_options *opt;
    double *const *y, *const *w, *const *v; cip_result *res;
};

// How far an entry point looks: the arrays; problem 0's b / v and d / w arrays ("null argument" too); every problem's vectors, a
// missing array among them ("null vector for problem i").  A level does not repeat the one before it beyond the arrays: cip_conicip_small
// asks for one after the other, around its own checks.
enum CheckLevel { CHECK_ARRAYS, CHECK_PROBLEM0, CHECK_EVERY };
inline int check_batch_call(const char *who, const BatchCall &k, CheckLevel level) {
    bool bad = k.count < 0 || (k.count > 0 && ((!k.probs && !k.handles) || !k.c || !k.y || !k.res));
    if (!bad && k.count > 0 && level == CHECK_PROBLEM0) bad = (k.probs[0].m > 0 && (!k.b || !k.v)) || (k.probs[0].p > 0 && (!k.d || !k.w));
    if (bad) { cip_set_error("%s: null argument", who); return CIP_E_INVALID; }
    for (int i = 0; level == CHECK_EVERY && i < k.count; ++i) {
        const cip_problem &q = k.probs[i];
        if ((q.m > 0 && (!k.b || !k.v || !k.b[i] || !k.v[i])) || (q.p > 0 && (!k.d || !k.w || !k.d[i] || !k.w[i])) || !k.c[i] || !k.y[i]) {
            cip_set_error("%s: null vector for problem %d", who, i);
            return CIP_E_INVALID;
        }
    }
    return 0;
}

// The problems idx[0], idx[1], ... of a call as a call of their own: view() goes to the nested entry point, scatter() writes its
// results back to the outer call's res -- when the caller says so.
struct SubBatch {
    const BatchCall &from;
    const std::vector<int> &idx;
    std::vector<cip_problem> gp;
    std::vector<const double *> gc, gb, gd;
    std::vector<double *> gy, gw, gv;
    std::vector<cip_result> gr;
    SubBatch(const BatchCall &k, const std::vector<int> &ix)
        : from(k), idx(ix), gp(ix.size()), gc(ix.size()), gb(ix.size()), gd(ix.size()), gy(ix.size()), gw(ix.size()), gv(ix.size()), gr(ix.size()) {
        for (size_t j = 0; j < idx.size(); ++j) {
            const int i = idx[j];
            gp[j] = k.probs[i]; gc[j] = k.c[i]; gy[j] = k.y[i];
            gb[j] = k.b ? k.b[i] : nullptr; gv[j] = k.v ? k.v[i] : nullptr;
            gd[j] = k.d ? k.d[i] : nullptr; gw[j] = k.w ? k.w[i] : nullptr;
        }
    }
    BatchCall view() { return {(int)idx.size(), gp.data(), nullptr, gc.data(), gb.data(), gd.data(), from.opt, gy.data(), gw.data(), gv.data(), gr.data()}; }
    void scatter() const { for (size_t j = 0; j < idx.size(); ++j) from.res[idx[j]] = gr[j]; }
};

// The shape every batch path compares: dimensions, cone list, host or device pointers.  (Lock-step adds the route and the matrix
// forms: lockstep.hip, same_shape; the small path has pinned those for every problem before it compares: small.hip, small_check.)
inline bool same_dims(const cip_problem &a, const cip_problem &b) {
    if (a.n != b.n || a.m != b.m || a.p != b.p || a.ncones != b.ncones || (a.flags & CIP_FLAG_DEVICE_PTRS) != (b.flags & CIP_FLAG_DEVICE_PTRS)) return false;
    for (int c = 0; c < a.ncones; ++c)
        if (a.cone_type[c] != b.cone_type[c] || a.cone_dim[c] != b.cone_dim[c]) return false;
    return true;
}

// S cones of order >= CIP_LARGE_S_MIN take chip-wide kernels with a single workspace (sdp_large.hip): no lock-step group holds one
inline bool has_chipwide_s_cone(const cip_problem &q) {
    for (int c = 0; c < q.ncones; ++c)
        if (q.cone_type[c] == CIP_CONE_S && q.cone_dim[c] >= CIP_LARGE_S_MIN * (CIP_LARGE_S_MIN + 1) / 2) return true;
    return false;
}
inline int refuse_chipwide_s_cone() { cip_set_error("lock-step batch: S cones of order >= %d are not supported", CIP_LARGE_S_MIN); return CIP_E_UNSUPPORTED; }

// The stride of an arena's per-problem slabs: an odd number of 256-byte granules, so that the same buffer of consecutive problems
// does not land on the same HBM channel
inline size_t slab_stride(size_t bytes) {
    size_t gran = (bytes + 255) / 256;
    if ((gran & 1) == 0) ++gran;
    return gran * 256;
}

inline cip_result fresh_result() {             // what a loop starts every problem's result from
    cip_result r = cip_result{};
    r.prFeas = r.duFeas = r.muFeas = INFINITY; r.pobj = INFINITY; r.dobj = -INFINITY;
    return r;
}

// The worker pool of batch.hip: up to `in_flight` threads -- the calling thread is the first, so that what the library keeps per thread
// (cip_last_error, statistics, profile) is the caller's after the call -- take the problems 0 .. count - 1 from one counter.
// per_thread_setup() makes a thread's state (its destructor is the tear-down), per_problem(state, i) solves problem i and returns its
// code.  A failed problem gets CIP_STATUS_ERROR and the others are still solved; the first failure's code and text are the call's.
template <typename Setup, typename PerProblem>
int run_pool(const BatchCall &k, int in_flight, Setup per_thread_setup, PerProblem per_problem) {
    if (in_flight < 1) in_flight = 1;
    if (in_flight > k.count) in_flight = k.count;
    std::atomic<int> next(0), first_rc(0);
    std::string first_err;
    std::atomic<bool> have_err(false);
    auto worker = [&]() {
        auto state = per_thread_setup();
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= k.count) return;
            const int rc = per_problem(state, i);
            if (rc != 0) {
                k.res[i].status = CIP_STATUS_ERROR;
                bool expected = false;
                if (have_err.compare_exchange_strong(expected, true)) { first_rc = rc; first_err = cip_last_error(); }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < in_flight; ++t) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
    if (have_err) { cip_set_error("problem failed: %s", first_err.c_str()); return first_rc; }
    return 0;
}

}   // namespace cipdrv
