// snesimage_amd/csrc/shared_window_host.inc — slot windows for a set (DESIGN §5b): snesimage_run_slots' speculation
// (window_host.inc) on one palette shared by F images (shared_host.inc).  Included by capi.hip after window_host.inc,
// whose records, slot contexts and size policy it reuses.
//
// A window scores the coming K calls of the schedule for every member against the current palette in ONE set of the
// batched launches: F * K "images", a slot context per (member, call) — its own pack, base image B and candidate
// storage; the member's source pyramid and its copy of the shared palette tables (window_make_child on the member).
// Every member of call j scores the one candidate list of key (seed, first_step_id + j).  ksw_commit (kernels_shared.hpp)
// sums the members' errors in member order, walks the calls in schedule order and applies the first one that accepts to
// every member; the calls behind it were scored against a palette that no longer exists and are run again.  Results
// equal snesimage_schedule_next + snesimage_shared_step per call bit for bit, whatever K.
//
// One window is in flight at a time: the host waits for a window's result before it builds the next (the single-image
// path's window-ahead is not built here).  B's sweeps run on a side stream beside the candidates' first stages.

struct snesimage_shared_window {
    std::vector<std::vector<snesimage_ctx *>> child; // [member][group]: slot contexts, grow-only
    WindowRec rec;                     // the window in flight (its argument blob holds K call records + F * K argument blocks)
    uint32_t cap = 0;                  // calls the record's arrays hold
    int *d_dead = nullptr;             // never raised (no window is enqueued ahead): kw_gen_candidates reads it
    hipStream_t side = nullptr; bool use_side = true;
    uint32_t adapt = 0;                // next window's size when the caller leaves it to the library (0: not yet chosen)
    WindowPolicy policy;
    // guided windows (shared_guided_window_host.inc) size themselves: a guided run between two scheduled runs leaves the launch sets of those as they were
    uint32_t g_adapt = 0; WindowPolicy g_policy;
    struct snesimage_sharedguidewin *g_work = nullptr; // ... and their generator's workspace, made by the first guided window
};

// A window whose calls are not the scheduler's (WindowGen for a set): the caller of shared_window_run names the slot order and
// writes the candidate lists itself.  next: the slot behind (*palette, *index); generate: n candidates for each of the window's K
// calls (r.h_slots / r.d_slots: their slots) into r.d_cand and the first K * n errors preset to +inf, on the set's stream, where
// kw_gen_candidates runs.
struct SharedWindowGen {
    uint32_t n;
    void (*next)(const snesimage_ctx *c0, uint32_t *palette, uint32_t *index);
    int32_t (*generate)(snesimage_shared *s, WindowRec &r, uint32_t K, uint32_t n);
};

namespace {

void shared_guided_window_free(snesimage_sharedguidewin *g);

void shared_window_free(snesimage_shared_window *w) {
    if (!w) return;
    shared_guided_window_free(w->g_work);
    for (auto &m : w->child) for (auto *k : m) window_release_child(k);
    if (w->side) { (void)hipStreamSynchronize(w->side); (void)hipStreamDestroy(w->side); }
    window_rec_free(w->rec);
    for (auto &e : w->rec.ev) if (e) (void)hipEventDestroy(e);
    if (w->rec.done) (void)hipEventDestroy(w->rec.done);
    dfree(w->d_dead);
    delete w;
}

// Calls a window of this set may hold: F * K slot contexts stay within SNES_WINDOW_MAX, what a single image's windows take.
uint32_t shared_window_kmax(snesimage_shared *s) { return window_max() / (uint32_t)members(s).size(); }

size_t shared_blob_bytes(uint32_t cap, uint32_t F) { return window_slots_bytes(cap) + sizeof(snes::BatchArgs) * (size_t)cap * F; }

// grow-only: the record's arrays for windows of K calls, `own` slot contexts per member.  A failed allocation leaves what
// was there (or nothing: cap = 0, fewer slot contexts) and the set usable.
int32_t shared_window_reserve(snesimage_shared *s, uint32_t K, uint32_t own) {
    auto &M = members(s);
    const uint32_t F = (uint32_t)M.size();
    if (!s->win) { s->win = new snesimage_shared_window(); s->win->child.resize(F); if (const char *e = getenv("SNES_WINDOW_SIDE")) s->win->use_side = atoi(e) != 0; }
    snesimage_shared_window *w = s->win;
    hipStream_t st = s->b->stream;
    if (!w->d_dead) {
        HIPCHK(dmalloc(&w->d_dead, sizeof(int)));
        HIPCHK(hipMemsetAsync(w->d_dead, 0, sizeof(int), st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (!w->side) HIPCHK(hipStreamCreateWithFlags(&w->side, hipStreamNonBlocking));
    for (int i = 0; i < 4; i++) if (!w->rec.ev[i]) HIPCHK(hipEventCreateWithFlags(&w->rec.ev[i], hipEventDisableTiming));
    if (!w->rec.done) HIPCHK(hipEventCreateWithFlags(&w->rec.done, hipEventDisableTiming));
    if (K > w->cap) {
        HIPCHK(hipStreamSynchronize(st));
        w->cap = 0;
        uint32_t cap = 8; while (cap < K) cap *= 2;
        WindowRec &r = w->rec;
        window_rec_free(r);
        HIPCHK(hipHostMalloc(&r.h_blob, shared_blob_bytes(cap, F)));
        HIPCHK(hipHostMalloc(&r.h_log, sizeof(snes::StepResult) * cap));
        HIPCHK(hipHostMalloc(&r.h_res, sizeof(snes::WindowResult)));
        HIPCHK(dmalloc(&r.d_blob, shared_blob_bytes(cap, F)));
        HIPCHK(dmalloc(&r.d_log, sizeof(snes::StepResult) * cap));
        HIPCHK(dmalloc(&r.d_res, sizeof(snes::WindowResult)));
        HIPCHK(dmalloc(&r.d_cand, 3 * 64 * (size_t)cap));
        HIPCHK(dmalloc(&r.d_errs, sizeof(double) * 64 * (size_t)cap * F));
        w->cap = cap;
    }
    for (uint32_t i = 0; i < F; i++)
        while (w->child[i].size() < own) {
            snesimage_ctx *k = nullptr;
            CHECK(window_make_child(M[i], &k)); // (sparse_alloc ends with a synchronisation of the member's stream: the context may be used on the set's at once)
            w->child[i].push_back(k);
        }
    return SNES_OK;
}

// What a window takes for granted in every member, then the set's stream behind whatever that queued on the members' own.
int32_t shared_window_prepare(snesimage_shared *s) {
    hipStream_t st = s->b->stream;
    for (auto *c : members(s)) {
        CHECK(ensure_tables(c));
        CHECK(ensure_source(c));
        CHECK(ensure_incumbent(c));
        if (c->dither) CHECK(run_prep(c, 1, -1, -1)); // the member's slot contexts read this pack
        if (!c->ev_own) HIPCHK(hipEventCreateWithFlags(&c->ev_own, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_own, c->stream));
        HIPCHK(hipStreamWaitEvent(st, c->ev_own, 0));
    }
    return SNES_OK;
}

// One window: at most n_slots calls from the scheduler state on, cut where the method changes; scored, committed, its
// result awaited.  *taken calls were scored, *used of them took effect, the last of them changed the palette if *acc.
// gen: the calls are the next n_slots slots of the caller's order instead, each of gen->n candidates that gen->generate writes;
// they are committed by the random method's rule.
int32_t shared_window_run(snesimage_shared *s, uint32_t n_slots, uint64_t seed, uint64_t first_step_id, uint32_t palette, uint32_t index, uint32_t channel, uint32_t step, uint32_t n_random,
                          snesimage_call_result *log, uint32_t *taken, uint32_t *stride, uint32_t *used, uint32_t *acc, const SharedWindowGen *gen = nullptr) {
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const uint32_t F = (uint32_t)M.size();
    struct Call { uint32_t method, palette, index, channel; } calls[snes::kMaxWindow];
    uint32_t K = 0;
    { uint32_t p = palette, i = index, ch = channel, st = step, m = 0, m0 = 0;
      while (K < n_slots) {
          const uint32_t cp = p, ci = i, cc = ch;
          if (s->backdrop && cp == c0->sub_count) break; // a window ends in front of a backdrop call (snesimage_shared_run_slots steps it on its own)
          if (gen) { gen->next(c0, &p, &i); calls[K++] = Call{SNES_METHOD_RANDOM, cp, ci, 0u}; continue; } // the caller's slot order
          ctx_schedule_next(c0, c0->nes ? 1 : 0, &p, &i, &ch, &st, &m); // (a backdrop set: snesimage_schedule_next_backdrop)
          if (K == 0) m0 = m; else if (m != m0) break;
          calls[K++] = Call{m, cp, ci, cc};
      } }
    const uint32_t method = calls[0].method, n = gen ? gen->n : method_count(method, n_random);
    if (n > 64) return fail(SNES_ERR_ARG, "a slot window holds at most 64 candidates per call");
    // groups: a call, or the consecutive channel calls of one entry behind one base image (window_enqueue's merge rule)
    struct Group { uint32_t j0, len; } groups[snes::kMaxWindow];
    uint32_t G = 0;
    for (uint32_t j = 0; j < K;) {
        uint32_t len = 1;
        while (j + len < K && n * (len + 1) <= kMemberCand && calls[j + len].palette == calls[j].palette && calls[j + len].index == calls[j].index) len++;
        groups[G++] = Group{j, len};
        j += len;
    }
    CHECK(shared_window_reserve(s, K, G));
    CHECK(shared_window_prepare(s));
    snesimage_shared_window *w = s->win;
    WindowRec &r = w->rec;
    hipStream_t st = s->b->stream;
    const size_t args_off = window_slots_bytes(K);
    r.h_slots = reinterpret_cast<snes::WindowSlot *>(r.h_blob); r.d_slots = reinterpret_cast<snes::WindowSlot *>(r.d_blob);
    r.h_args = reinterpret_cast<snes::BatchArgs *>(r.h_blob + args_off); r.d_args = reinterpret_cast<snes::BatchArgs *>(r.d_blob + args_off);
    for (uint32_t j = 0; j < K; j++) {
        snes::WindowSlot &sl = r.h_slots[j];
        sl.method = (int)calls[j].method; sl.n = (int)n; sl.slot = (int)(calls[j].palette * c0->sub_size + calls[j].index); sl.channel = (int)calls[j].channel;
        sl.nes = method == SNES_METHOD_NES ? 1 : 0; sl.member = -1; sl.cand0 = 0; sl.pad = 0;
        sl.key = mix64(seed ^ ((first_step_id + j) * 0x9E3779B97F4A7C15ull) ^ 0xD1B54A32D192ED03ull);
    }
    uint32_t n_max = 0;
    for (uint32_t g = 0; g < G; g++) {
        const uint32_t j0 = groups[g].j0, len = groups[g].len;
        for (uint32_t l = 0; l < len; l++) { r.h_slots[j0 + l].member = (int)g; r.h_slots[j0 + l].cand0 = (int)(l * n); }
        if (n * len > n_max) n_max = n * len;
        for (uint32_t i = 0; i < F; i++) { // member-major: member i's groups follow each other
            snes::BatchArgs &a = r.h_args[(size_t)i * G + g];
            CHECK(fill_batch_args(a, w->child[i][g], n * len, method, calls[j0].palette, calls[j0].index, calls[j0].channel, r.h_slots[j0].key));
            a.dead_base = 1;
            a.cand = r.d_cand + 3 * (size_t)j0 * n;                 // one list per call, read by every member
            a.errors = r.d_errs + ((size_t)i * K + j0) * n;         // errors[(i * K + j) * n + k]
        }
    }
    HIPCHK(hipMemcpyAsync(r.d_blob, r.h_blob, args_off + sizeof(snes::BatchArgs) * (size_t)F * G, hipMemcpyHostToDevice, st));
    if (gen) CHECK(gen->generate(s, r, K, n)); // the caller's lists in the random candidates' place
    else hipLaunchKernelGGL(kw_gen_candidates, dim3((n + 63) / 64, K), dim3(64), 0, st, r.d_slots, c0->d_colors, r.d_cand, r.d_errs, (int)n, (const int *)w->d_dead, 1);
    BatchSide bs{w->use_side ? w->side : nullptr, r.ev[0], r.ev[1], r.ev[2], r.ev[3], false};
    CHECK(enqueue_batched_scoring(st, r.d_args, F * G, n_max, w->child[0][0], &bs, nullptr));
    hipLaunchKernelGGL(ksw_commit, dim3(1), dim3(1024), 0, st, r.d_slots, (int)K, (int)n, (int)F, (int)G, r.d_args, r.d_errs, r.d_cand, s->d_joint, r.d_res, r.d_log);
    if (c0->dither) hipLaunchKernelGGL(ksw_take_map, dim3(F), dim3(1024), 0, st, r.d_args, (int)G, r.d_slots, r.d_res, r.d_log, (int)c0->npx); // lib.rs:237: the winner's own resumed run, per member
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(r.h_res, r.d_res, sizeof(snes::WindowResult), hipMemcpyDeviceToHost, st));
    if (log) HIPCHK(hipMemcpyAsync(r.h_log, r.d_log, sizeof(snes::StepResult) * K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(r.done, st));
    s->b->busy = true;
    for (size_t i = 0; i < M.size(); i++) { // what a set call leaves behind in a member (batch_call); the map of the committed state is owed
        snesimage_ctx *c = M[i];
        c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
        c->map_pending = !c->dither; c->map_synced = true; c->inc_valid = true; c->best_valid = false;
        s->epoch[i] = c->epoch;
    }
    HIPCHK(hipEventSynchronize(r.done));
    const uint32_t done = (uint32_t)r.h_res->consumed;
    if (log) for (uint32_t j = 0; j < done; j++) { log[j].error = r.h_log[j].error; log[j].best_k = r.h_log[j].best_k; memcpy(log[j].rgb5, r.h_log[j].rgb5, 3); log[j].changed = r.h_log[j].changed; }
    *taken = K; *stride = n; *used = done; *acc = (uint32_t)r.h_res->accepted;
    return SNES_OK;
}

} // namespace

extern "C" {

// Storage for windows of up to n_slots calls now rather than on first use: F slot contexts per call (~0.3 GB each), at
// most SNES_WINDOW_MAX in all.
int32_t snesimage_shared_slots_reserve(snesimage_shared *s, uint32_t n_slots) {
    CHECK(shared_enter(s));
    const uint32_t kmax = shared_window_kmax(s);
    if (kmax < 2) return SNES_OK; // such a set steps call by call: nothing to reserve
    if (n_slots > kmax) n_slots = kmax;
    if (n_slots == 0) n_slots = 1;
    return shared_window_reserve(s, n_slots, n_slots);
}

// The reference's loop on the set for n_calls calls from scheduler state (*palette, *index, *channel, *step): equivalent,
// bit for bit, to snesimage_schedule_next + snesimage_shared_step per call.  window = calls scored per launch set
// (0: chosen by the library, 1: call by call).
int32_t snesimage_shared_run_slots(snesimage_shared *s, uint32_t n_calls, uint64_t seed, uint64_t first_step_id, uint32_t *palette, uint32_t *index, uint32_t *channel, uint32_t *step,
                                   uint32_t n_random, uint32_t window, snesimage_call_result *log, snesimage_run_stats *stats) {
    if (!s || !palette || !index || !channel || !step) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s));
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    CHECK(check_slot(c0, *palette, *index));
    if (*channel > 2) return fail(SNES_ERR_ARG, "bad channel");
    snesimage_run_stats S{};
    const int nes = c0->nes ? 1 : 0;
    const uint32_t F = (uint32_t)M.size(), kmax = shared_window_kmax(s);
    const bool windows = window != 1 && n_random <= 64 && kmax >= 2; // (more members than slot contexts: call by call)
    uint32_t done = 0, method = 0;
    while (done < n_calls) {
        bool synced = true;
        for (auto *c : M) synced = synced && c->map_synced;
        uint32_t K = 1;
        if (windows && synced) {
            if (!s->win || !s->win->adapt) { CHECK(shared_window_reserve(s, 1, 0)); s->win->adapt = kmax < kWindowMin ? kmax : kWindowMin; }
            K = window ? window : s->win->adapt;
            if (K > n_calls - done) K = n_calls - done;
            if (K > kmax) K = kmax;
        }
        uint32_t taken = 1, used = 1, acc = 0, n = 0;
        const bool tied = s->backdrop && *palette == c0->sub_count; // a backdrop call: no window's, and nothing the size policy learns from
        if (!windows || !synced || (window == 0 && K == 1 && s->win->adapt == 1) || tied) {
            // One call on its own: what the windows do not cover (a backdrop call among it: DESIGN §5c''), a first call that starts
            // from a palette_map which is not optimize() of the palette, and a phase in which the size policy finds one call per
            // launch set fastest
            uint32_t p = *palette, i = *index, ch = *channel, m = 0, st = *step;
            ctx_schedule_next(c0, nes, &p, &i, &ch, &st, &m);
            CHECK(snesimage_shared_step_async(s, m, *palette, *index, *channel, seed, first_step_id + done, n_random));
            snesimage_call_result r;
            CHECK(snesimage_shared_last_step(s, &r));
            if (log) log[done] = r;
            n = method_count(m, n_random);
            acc = (nes ? r.changed != 0 : r.best_k >= 0) ? 1 : 0; // (what a window reports: a candidate accepted; NES: the colour changed)
        } else {
            CHECK(shared_window_run(s, K, seed, first_step_id + done, *palette, *index, *channel, *step, n_random, log ? log + done : nullptr, &taken, &n, &used, &acc));
        }
        for (uint32_t j = 0; j < used; j++) ctx_schedule_next(c0, nes, palette, index, channel, step, &method);
        done += used;
        S.calls += used; S.windows++; S.scored += (uint64_t)taken * n; S.useful += (uint64_t)used * n; S.accepted += acc;
        if (windows && synced && !tied) s->win->adapt = s->win->policy.next(used, acc, 1, kmax, 1, taken, (double)F);
    }
    if (stats) *stats = S;
    return SNES_OK;
}

} // extern "C"
