// snesimage_amd/csrc/group_host.inc — one process driving several GPUs: candidate sharding with RCCL inside the library.
// (`bench.py` and snesimage_amd/distributed.py use one process per GPU and let torch.distributed issue the collective;
// this is the same step for a host that owns all devices itself, e.g. the reference's single Rust process.)
// A group borrows one context per device, all holding the same image and state.  A step is snesimage_step_begin on every
// member (rank r scores candidates k = r mod N), ONE grouped ncclAllReduce(min) over the N error vectors on the
// members' streams, and snesimage_step_commit on every member: all palettes stay bit-identical (SURVEY §8e).
// librccl is opened at run time, on the first group: the library itself does not link against it.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

// One host thread per member: a phase of a step is ~20 kernel launches per device, and issued from one thread the members
// would start one after the other (N x ~0.1 ms of enqueueing before the last device has anything to do).
struct GroupWorkers {
    struct Slot { std::function<int32_t()> job; int32_t rc = 0; std::string err; bool busy = false; };
    std::vector<std::thread> th; std::vector<Slot> slot;
    std::mutex m; std::condition_variable cv_go, cv_done; bool quit = false;
    void start(size_t n) {
        slot.resize(n);
        for (size_t i = 0; i < n; i++) th.emplace_back([this, i] {
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                cv_go.wait(lk, [&] { return quit || slot[i].busy; });
                if (quit) return;
                auto job = slot[i].job;
                lk.unlock();
                const int32_t rc = job();
                std::string e = rc != SNES_OK ? g_err : std::string(); // the message lives in this thread's g_err
                lk.lock();
                slot[i].rc = rc; slot[i].err = e; slot[i].busy = false;
                cv_done.notify_all();
            }
        });
    }
    // job(r) on member r's thread, all at once; the first failure's code and message are the caller's
    int32_t run(const std::function<int32_t(uint32_t)> &job) {
        { std::lock_guard<std::mutex> lk(m); for (size_t i = 0; i < slot.size(); i++) { slot[i].job = [job, i] { return job((uint32_t)i); }; slot[i].busy = true; } }
        cv_go.notify_all();
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { for (auto &s : slot) if (s.busy) return false; return true; });
        for (auto &s : slot) if (s.rc != SNES_OK) return fail(s.rc, s.err);
        return SNES_OK;
    }
    void stop() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv_go.notify_all();
        for (auto &t : th) t.join();
        th.clear();
    }
};

struct snesimage_group {
    std::vector<snesimage_ctx *> ctx; // a member destroyed under the group is replaced by nullptr and the group retired (dead)
    bool dead = false;
    std::vector<ncclComm_t> comm;
    std::vector<double *> d_err;
    uint32_t err_cap = 0;
    GroupWorkers workers;
};

namespace {

struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
} g_rccl;

int32_t rccl_load() {
    if (g_rccl.lib) return SNES_OK;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so"}) { h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) return fail(SNES_ERR_UNSUPPORTED, std::string("cannot open librccl: ") + dlerror());
    RcclApi a; a.lib = h;
    a.CommInitAll = (decltype(a.CommInitAll))dlsym(h, "ncclCommInitAll");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
    a.GroupStart = (decltype(a.GroupStart))dlsym(h, "ncclGroupStart");
    a.GroupEnd = (decltype(a.GroupEnd))dlsym(h, "ncclGroupEnd");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!a.CommInitAll || !a.CommDestroy || !a.AllReduce || !a.GroupStart || !a.GroupEnd || !a.GetErrorString) return fail(SNES_ERR_UNSUPPORTED, "librccl lacks an expected symbol");
    g_rccl = a;
    return SNES_OK;
}
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return fail(SNES_ERR_HIP, std::string("RCCL: ") + g_rccl.GetErrorString(r_)); } while (0)

} // namespace

extern "C" {

int32_t snesimage_group_create(snesimage_ctx **ctxs, uint32_t n, snesimage_group **out) {
    if (!ctxs || !out || n == 0) return fail(SNES_ERR_ARG, "null pointer or empty group");
    *out = nullptr;
    std::vector<int> devs;
    for (uint32_t i = 0; i < n; i++) {
        snesimage_ctx *c = ctxs[i];
        if (!c) return fail(SNES_ERR_ARG, "null context in group");
        if (c->group) return fail(SNES_ERR_STATE, "context already belongs to a group");
        if (c->backdrop) return fail(SNES_ERR_UNSUPPORTED, kBackdropRefused);
        if (c->od_L > 1) return fail(SNES_ERR_ARG, kLevelsRefused);
        if (blocked(c)) return fail(SNES_ERR_UNSUPPORTED, kBlockedRefused);
        if (c->W != ctxs[0]->W || c->H != ctxs[0]->H || c->sub_count != ctxs[0]->sub_count || c->sub_size != ctxs[0]->sub_size || c->dither != ctxs[0]->dither ||
            c->perceptual != ctxs[0]->perceptual)
            return fail(SNES_ERR_ARG, "contexts of a group must hold the same image geometry, palette geometry and flags");
        if (!ordered_tables_equal(c, ctxs[0])) return fail(SNES_ERR_ARG, "contexts of a group must share their ordered-dither table");
        for (int d : devs) if (d == c->device) return fail(SNES_ERR_ARG, "a group takes one context per device");
        devs.push_back(c->device);
    }
    CHECK(rccl_load());
    std::unique_ptr<snesimage_group> g(new snesimage_group());
    g->ctx.assign(ctxs, ctxs + n);
    g->comm.resize(n);
    g->d_err.assign(n, nullptr);
    NCCLCHK(g_rccl.CommInitAll(g->comm.data(), (int)n, devs.data()));
    for (auto *c : g->ctx) c->group = g.get();
    g->workers.start(n);
    *out = g.release();
    return SNES_OK;
}

// a member context is being destroyed while it belongs to a group: the group is retired, the other members are their own again
void group_forget(snesimage_group *g, snesimage_ctx *c) {
    for (auto *&m : g->ctx) { if (m) { m->group = nullptr; m->pend = false; } if (m == c) m = nullptr; }
    g->dead = true;
}

void snesimage_group_destroy(snesimage_group *g) {
    if (!g) return;
    g->workers.stop();
    for (size_t r = 0; r < g->ctx.size(); r++) {
        if (g->ctx[r]) {
            (void)hipSetDevice(g->ctx[r]->device);
            (void)hipStreamSynchronize(g->ctx[r]->stream);
            g->ctx[r]->group = nullptr;
        }
        if (g->comm[r]) (void)g_rccl.CommDestroy(g->comm[r]);
        if (g->d_err[r]) (void)hipFree(g->d_err[r]);
    }
    delete g;
}

// One optimizer call (lib.rs:191-328 + 906-910) with its candidates sharded over the group's devices.
int32_t snesimage_group_step(snesimage_group *g, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_total, double *best_error,
                             uint8_t *best_rgb5) {
    if (!g) return fail(SNES_ERR_ARG, "null group");
    if (g->dead) return fail(SNES_ERR_STATE, "a member context of this group was destroyed");
    const uint32_t N = (uint32_t)g->ctx.size();
    const uint32_t n = method_count(method, n_total);
    if (n > g->err_cap) {
        g->err_cap = 0; // released below: a failed grow must not leave the old capacity behind
        for (uint32_t r = 0; r < N; r++) {
            HIPCHK(hipSetDevice(g->ctx[r]->device));
            HIPCHK(hipStreamSynchronize(g->ctx[r]->stream));
            if (g->d_err[r]) { HIPCHK(hipFree(g->d_err[r])); g->d_err[r] = nullptr; }
            HIPCHK(hipMalloc(&g->d_err[r], sizeof(double) * n));
        }
        g->err_cap = n;
    }
    // A failure part-way leaves no member with a half-finished step (pend) and never leaves an RCCL group open.
    auto abandon = [&](int32_t rc) { for (auto *c : g->ctx) c->pend = false; return rc; };
    { const int32_t rc = g->workers.run([&](uint32_t r) { return snesimage_step_begin(g->ctx[r], method, palette, index, channel, seed, step_id, n_total, r, N, g->d_err[r]); });
      if (rc != SNES_OK) return abandon(rc); }
    NCCLCHK(g_rccl.GroupStart());
    int32_t rc = SNES_OK;
    for (uint32_t r = 0; r < N && rc == SNES_OK; r++) {
        const hipError_t he = hipSetDevice(g->ctx[r]->device);
        if (he != hipSuccess) { rc = fail(SNES_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he)); break; }
        const ncclResult_t nr = g_rccl.AllReduce(g->d_err[r], g->d_err[r], n, ncclDouble, ncclMin, g->comm[r], g->ctx[r]->stream);
        if (nr != ncclSuccess) rc = fail(SNES_ERR_HIP, std::string("RCCL: ") + g_rccl.GetErrorString(nr));
    }
    { const ncclResult_t nr = g_rccl.GroupEnd(); // closed on the error path as well
      if (nr != ncclSuccess && rc == SNES_OK) rc = fail(SNES_ERR_HIP, std::string("RCCL: ") + g_rccl.GetErrorString(nr)); }
    if (rc != SNES_OK) return abandon(rc);
    rc = g->workers.run([&](uint32_t r) { return snesimage_step_commit(g->ctx[r], g->d_err[r]); });
    if (rc != SNES_OK) return abandon(rc);
    if (best_error || best_rgb5) return snesimage_last_step(g->ctx[0], best_error, best_rgb5, nullptr);
    return SNES_OK;
}

// One grouped all-reduce(min) of the first `count` doubles of every member's error vector, on the members' streams.
static int32_t group_allreduce_min(snesimage_group *g, size_t count) {
    const uint32_t N = (uint32_t)g->ctx.size();
    NCCLCHK(g_rccl.GroupStart());
    int32_t rc = SNES_OK;
    for (uint32_t r = 0; r < N && rc == SNES_OK; r++) {
        const hipError_t he = hipSetDevice(g->ctx[r]->device);
        if (he != hipSuccess) { rc = fail(SNES_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he)); break; }
        const ncclResult_t nr = g_rccl.AllReduce(g->d_err[r], g->d_err[r], count, ncclDouble, ncclMin, g->comm[r], g->ctx[r]->stream);
        if (nr != ncclSuccess) rc = fail(SNES_ERR_HIP, std::string("RCCL: ") + g_rccl.GetErrorString(nr));
    }
    { const ncclResult_t nr = g_rccl.GroupEnd(); // closed on the error path as well
      if (nr != ncclSuccess && rc == SNES_OK) rc = fail(SNES_ERR_HIP, std::string("RCCL: ") + g_rccl.GetErrorString(nr)); }
    return rc;
}

// snesimage_run_slots over the group: the calls of every window are dealt to the members (runs of six consecutive calls, round
// robin: every call its own base image, its own candidates), ONE grouped all-reduce(min) over the window's error vector, then every
// member commits the same decisions in the same order: the palettes stay bit-identical on all devices and the trajectory
// is the reference's, call for call (lib.rs:888-933).  Configurations the windows do not cover fall back to
// snesimage_group_step per call.
int32_t snesimage_group_run_slots(snesimage_group *g, uint32_t n_calls, uint64_t seed, uint64_t first_step_id, uint32_t *palette, uint32_t *index, uint32_t *channel, uint32_t *step,
                                  uint32_t n_random, uint32_t window, snesimage_call_result *log, snesimage_run_stats *stats) {
    if (!g || !palette || !index || !channel || !step) return fail(SNES_ERR_ARG, "null pointer");
    if (g->dead) return fail(SNES_ERR_STATE, "a member context of this group was destroyed");
    const uint32_t N = (uint32_t)g->ctx.size();
    snesimage_ctx *c0 = g->ctx[0];
    const int nes = c0->nes ? 1 : 0;
    snesimage_run_stats S{};
    uint32_t done = 0, method = 0;
    bool windows = window != 1 && n_random <= 64;
    for (auto *c : g->ctx) windows = windows && window_capable(c);
    const uint32_t cap_calls = window_max() * N > (uint32_t)snes::kMaxWindow ? (uint32_t)snes::kMaxWindow : window_max() * N;
    if (windows && (size_t)cap_calls * 64 > g->err_cap) {
        g->err_cap = 0;
        for (uint32_t r = 0; r < N; r++) {
            HIPCHK(hipSetDevice(g->ctx[r]->device));
            HIPCHK(hipStreamSynchronize(g->ctx[r]->stream));
            if (g->d_err[r]) { HIPCHK(hipFree(g->d_err[r])); g->d_err[r] = nullptr; }
            HIPCHK(hipMalloc(&g->d_err[r], sizeof(double) * cap_calls * 64));
        }
        g->err_cap = cap_calls * 64;
    }
    uint32_t adapt = kWindowMin * N; WindowPolicy policy;
    std::vector<uint32_t> taken(N), stride(N), used(N), acc(N);
    auto abandon = [&](int32_t rc) { for (auto *c : g->ctx) c->win_pend = false; return rc; };
    while (done < n_calls) {
        // (as snesimage_run_slots: a first call that starts from a palette_map which is not optimize() of the palette — the state
        // recalculate_palettes leaves — is stepped alone; every call leaves the members synced, so the windows start with the next)
        bool synced = true;
        for (auto *c : g->ctx) synced = synced && c->map_synced;
        if (!windows || !synced) { // one call, its candidates sharded (snesimage_group_step)
            uint32_t p = *palette, i = *index, ch = *channel;
            snesimage_schedule_next(c0->sub_count, c0->sub_size, nes, palette, index, channel, step, &method);
            CHECK(snesimage_group_step(g, method, p, i, ch, seed, first_step_id + done, n_random, nullptr, nullptr));
            snes::StepResult r;
            HIPCHK(hipSetDevice(c0->device));
            HIPCHK(hipMemcpyAsync(&r, c0->d_last, sizeof(r), hipMemcpyDeviceToHost, c0->stream));
            HIPCHK(hipStreamSynchronize(c0->stream));
            if (log) { log[done].error = r.error; log[done].best_k = r.best_k; memcpy(log[done].rgb5, r.rgb5, 3); log[done].changed = r.changed; }
            const uint32_t n = method_count(method, n_random);
            S.calls++; S.windows++; S.scored += n; S.useful += n; if (r.changed) S.accepted++;
            done++;
            continue;
        }
        uint32_t K = window ? window : adapt;
        if (K > n_calls - done) K = n_calls - done;
        if (K > cap_calls) K = cap_calls;
        int32_t rc = g->workers.run([&](uint32_t r) { return snesimage_slots_begin(g->ctx[r], K, seed, first_step_id + done, *palette, *index, *channel, *step, n_random, r, N, g->d_err[r], &taken[r], &stride[r]); });
        if (rc != SNES_OK) return abandon(rc);
        rc = group_allreduce_min(g, (size_t)taken[0] * stride[0]);
        if (rc != SNES_OK) return abandon(rc);
        rc = g->workers.run([&](uint32_t r) { return snesimage_slots_commit(g->ctx[r], g->d_err[r], &used[r], &acc[r], r == 0 && log ? log + done : nullptr); });
        if (rc != SNES_OK) return abandon(rc);
        for (uint32_t r = 1; r < N; r++) if (used[r] != used[0] || acc[r] != acc[0]) return fail(SNES_ERR_STATE, "the members of the group disagree on a window's outcome: their states have diverged");
        for (uint32_t j = 0; j < used[0]; j++) snesimage_schedule_next(c0->sub_count, c0->sub_size, nes, palette, index, channel, step, &method);
        S.calls += used[0]; S.windows++; S.scored += (uint64_t)taken[0] * stride[0]; S.useful += (uint64_t)used[0] * stride[0]; S.accepted += acc[0];
        done += used[0];
        adapt = policy.next(used[0], acc[0], kWindowMin * N, cap_calls, N, taken[0]);
    }
    if (stats) *stats = S;
    return SNES_OK;
}

} // extern "C"
