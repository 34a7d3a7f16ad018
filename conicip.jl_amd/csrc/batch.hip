// Batches of independent problems on one GPU (BASELINE config 5; SURVEY 8b "cip_batch_*", 8e).
// A single KKT system never leaves its GPU and independent problems share nothing, so a batch is an array of
// ordinary handles -- each with its own HIP stream -- plus a host-thread pool that keeps `in_flight` interior-point
// loops running at once: a small system (n ~ 2048) is a chain of tiny dependent launches that leaves most of the
// chip idle, several of them on different streams fill it (measured from Python threads: 481 -> 658 KKT solves/s).
// Per-problem work uses the normal entry points on cip_batch_handle(b, i) (the "leading problem index").
#include "cip_handle.h"
#include "cip_batch_front.h"
#include <string>
#include <vector>

using namespace cipdrv;

struct cip_batch {
    std::vector<cip_handle *> h;
    std::vector<hipStream_t> streams;
};

// problem i of a call through the one-problem loop on handle h
static int solve_one(const BatchCall &k, cip_handle *h, int i) {
    return cip_conicip(h, k.c[i], k.b ? k.b[i] : nullptr, k.d ? k.d[i] : nullptr, k.opt, k.y[i], k.w ? k.w[i] : nullptr,
                       k.v ? k.v[i] : nullptr, &k.res[i], nullptr, 0);
}

extern "C" int cip_conicip_many(cip_handle *const *handles, int count, const double *const *c, const double *const *b,
                                const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                                double *const *v, cip_result *res, int in_flight) {
    const BatchCall k = {count, nullptr, handles, c, b, d, opt, y, w, v, res};
    CIP_TRY(check_batch_call("cip_conicip_many", k, CHECK_ARRAYS));
    if (count == 0) return 0;
    return run_pool(k, in_flight, [] { return 0; }, [&](int, int i) { return solve_one(k, handles[i], i); });
}

// Problems in, solutions out: `in_flight` worker threads, each with ONE handle on its own stream that is re-loaded
// (cip_update_problem: no hipMalloc / hipFree, which synchronise the device) for every problem of the same shape it
// takes from the queue -- so the level-1 upload of one problem overlaps the interior-point loops of the others, and a
// batch of small systems, each a chain of tiny dependent launches, fills the chip.
extern "C" int cip_conicip_problems(int count, const cip_problem *probs, const double *const *c, const double *const *b,
                                    const double *const *d, const cip_options *opt, double *const *y, double *const *w,
                                    double *const *v, cip_result *res, int in_flight) {
    const BatchCall k = {count, probs, nullptr, c, b, d, opt, y, w, v, res};
    CIP_TRY(check_batch_call("cip_conicip_problems", k, CHECK_ARRAYS));
    if (count == 0) return 0;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { cip_set_error("no HIP device"); return CIP_E_NODEVICE; }
    struct Worker {                // a thread's handle and stream
        cip_handle *h = nullptr;
        hipStream_t st = nullptr;
        explicit Worker(int dev) { (void)hipSetDevice(dev); if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr; }
        Worker(const Worker &) = delete;
        ~Worker() { if (h) cip_destroy(h); if (st) (void)hipStreamDestroy(st); }
    };
    return run_pool(k, in_flight, [&] { return Worker(device); }, [&](Worker &t, int i) {
        int rc = 0;
        // (refused for another shape -- another Q form, dense or CSR, or another nnz of a CSR Q or A included: new handle)
        if (t.h && cip_update_problem(t.h, &probs[i]) != 0) { cip_destroy(t.h); t.h = nullptr; }     // other shape: new handle
        if (!t.h) {
            rc = cip_create_ex(&probs[i], &t.h);
            if (rc == 0 && t.st) rc = cip_set_stream(t.h, t.st);
        }
        return rc ? rc : solve_one(k, t.h, i);
    });
}

extern "C" int cip_batch_create(int count, const cip_problem *probs, cip_batch **out) {
    if (count < 0 || (count > 0 && !probs) || !out) { cip_set_error("cip_batch_create: bad argument"); return CIP_E_INVALID; }
    cip_batch *b = new (std::nothrow) cip_batch();
    if (!b) { cip_set_error("out of host memory"); return CIP_E_INVALID; }
    *out = nullptr;
    for (int i = 0; i < count; ++i) {
        cip_handle *h = nullptr;
        int rc = cip_create_ex(&probs[i], &h);
        hipStream_t s = nullptr;
        if (rc == 0 && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { cip_set_error("hipStreamCreate failed"); rc = CIP_E_HIP; }
        if (rc == 0) rc = cip_set_stream(h, s);
        if (rc != 0) {
            if (h) cip_destroy(h);
            if (s) (void)hipStreamDestroy(s);
            const std::string msg = cip_last_error();
            cip_batch_destroy(b);
            cip_set_error("problem %d: %s", i, msg.c_str());
            return rc;
        }
        b->h.push_back(h);
        b->streams.push_back(s);
    }
    *out = b;
    return 0;
}
extern "C" int cip_batch_destroy(cip_batch *b) {
    if (!b) return 0;
    for (size_t i = 0; i < b->h.size(); ++i) {
        (void)hipStreamSynchronize(b->streams[i]);
        cip_destroy(b->h[i]);
        (void)hipStreamDestroy(b->streams[i]);
    }
    delete b;
    return 0;
}
extern "C" int cip_batch_size(const cip_batch *b) { return b ? (int)b->h.size() : 0; }
extern "C" cip_handle *cip_batch_handle(cip_batch *b, int i) { return (b && i >= 0 && i < (int)b->h.size()) ? b->h[i] : nullptr; }
extern "C" int cip_batch_conicip(cip_batch *b, const double *const *c, const double *const *bb, const double *const *d,
                                 const cip_options *opt, double *const *y, double *const *w, double *const *v, cip_result *res,
                                 int in_flight) {
    if (!b) { cip_set_error("cip_batch_conicip: null batch"); return CIP_E_INVALID; }
    return cip_conicip_many(b->h.data(), (int)b->h.size(), c, bb, d, opt, y, w, v, res, in_flight);
}
