// snesimage_amd/csrc/shared_guided_window_host.inc — guided calls of a set through the slot windows:
// snesimage_shared_guided_run_slots (definition: include/snesimage_hip.h; kernels: kernels_guide_set_window.hpp; DESIGN 5f'''').
//
// A rejected guided set call changes nothing that a shortlist or a score reads (the palette, tile_palettes, the targets, and the
// maps the palette implies), so a guided window of a set IS the set's scheduled window (shared_window_run) — the same slot
// contexts per (member, call), batched scoring, ksw_commit with the random method's rule, ksw_take_map for --dither — whose
// candidate lists are written by the generator instead of kw_gen_candidates (shared_window_run's `gen` argument).  The window's
// generator forms one table per subpalette and one correction per call instead of one full table per call.  One window is in
// flight at a time.  Included by capi.hip behind shared_guide_host.inc, shared_window_host.inc and guided_window_host.inc.

struct snesimage_sharedguidewin { // the generator's workspace of a set's guided windows
    uint32_t cap = 0, subs = 0, G = 0;      // calls and distinct subpalettes a window may hold; global tiles of the set
    snes::GuidePixel *shared = nullptr;      // [subs][G * 64]: a subpalette's population as (rgb8 of T, a)
    snes::GuideOwnPixel *own = nullptr;      // [cap][G * 64]: a call's own pixels (j* == its entry) as (rgb8 of T, a, b)
    unsigned long long *tab = nullptr;       // the counts (32 bits each: subs shared, cap own; cap words in all), then the window's tables A, then its tables D
    int *d_plan = nullptr, *h_plan = nullptr; // per call the number of its subpalette among the window's (h_plan: pinned; one window is in flight)
};

namespace {

void shared_guided_window_free(snesimage_sharedguidewin *g) {
    if (!g) return;
    dfree(g->shared); dfree(g->own); dfree(g->tab); dfree(g->d_plan);
    if (g->h_plan) (void)hipHostFree(g->h_plan);
    delete g;
}

// The workspace for shared_window_kmax calls: all or nothing (four device allocations).
int32_t sgw_alloc(snesimage_shared *s) {
    snesimage_shared_window *w = s->win;
    if (w->g_work) return SNES_OK;
    const snesimage_ctx *c0 = members(s)[0];
    snesimage_sharedguidewin n;
    n.cap = shared_window_kmax(s); n.subs = n.cap < c0->sub_count ? n.cap : c0->sub_count; n.G = (uint32_t)members(s).size() * sg_ntile(s);
    const size_t list = (size_t)n.G * 64;
    if (dmalloc(&n.shared, sizeof(snes::GuidePixel) * list * n.subs) != hipSuccess || dmalloc(&n.own, sizeof(snes::GuideOwnPixel) * list * n.cap) != hipSuccess ||
        dmalloc(&n.tab, sizeof(unsigned long long) * (n.cap + (size_t)snes::kGuideColors * (n.subs + n.cap))) != hipSuccess || dmalloc(&n.d_plan, sizeof(int) * n.cap) != hipSuccess ||
        hipHostMalloc(&n.h_plan, sizeof(int) * n.cap) != hipSuccess) {
        dfree(n.shared); dfree(n.own); dfree(n.tab); dfree(n.d_plan);
        return fail(SNES_ERR_HIP, "out of device memory for the workspace of the set's guided windows");
    }
    w->g_work = new snesimage_sharedguidewin(n);
    return SNES_OK;
}

// The tables of the K calls whose records are r.h_slots / r.d_slots, on the set's stream: A of every distinct subpalette, D of
// every call.  *A, *D: where they are (call j reads A + plan[j] * 32,768 and D + j * 32,768); *subs: the distinct subpalettes.
int32_t sgw_tables(snesimage_shared *s, WindowRec &r, uint32_t K, unsigned long long **A, unsigned long long **D, uint32_t *subs) {
    snesimage_shared_window *w = s->win;
    snesimage_sharedguidewin *g = w->g_work;
    const snesimage_ctx *c0 = members(s)[0];
    hipStream_t st = s->b->stream;
    const uint32_t ntile = sg_ntile(s);
    uint32_t nsub = 0;
    for (uint32_t j = 0; j < K; j++) { // the window's subpalettes, numbered in the order of their first call
        const int p = r.h_slots[j].slot / (int)c0->sub_size;
        int q = -1;
        for (uint32_t e = 0; e < j && q < 0; e++) if (r.h_slots[e].slot / (int)c0->sub_size == p) q = g->h_plan[e];
        g->h_plan[j] = q < 0 ? (int)nsub++ : q;
    }
    unsigned int *shared_counts = reinterpret_cast<unsigned int *>(g->tab), *own_counts = shared_counts + g->subs;
    unsigned long long *tabA = g->tab + g->cap, *tabD = tabA + (size_t)snes::kGuideColors * nsub;
    HIPCHK(hipMemcpyAsync(g->d_plan, g->h_plan, sizeof(int) * K, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(g->tab, 0, sizeof(unsigned long long) * (g->cap + (size_t)snes::kGuideColors * (nsub + K)), st)); // the counts and the window's tables: once per window
    const uint32_t slices = (g->G * 64 + snes::kGuideSlice - 1) / snes::kGuideSlice; // the host does not know the counts: the largest list, every tile
    hipLaunchKernelGGL(ksgw_gather_shared, dim3(g->G), dim3(64), 0, st, (const snes::WindowSlot *)r.d_slots, (const int *)g->d_plan, (int)K, (const snes::GuideMember *)s->guide->d_mem, (const uint8_t *)c0->d_colors,
                       (int)ntile, (int)g->G, (int)c0->W, (int)c0->sub_size, g->shared, shared_counts, (const int *)w->d_dead, 1);
    hipLaunchKernelGGL(kw_guide_cost, dim3(snes::kGuideColors / 256, slices, nsub), dim3(256), 0, st, (const snes::GuidePixel *)g->shared, (const unsigned int *)shared_counts, (int)g->G, tabA, (const int *)w->d_dead, 1);
    hipLaunchKernelGGL(ksgw_gather_own, dim3(g->G, K), dim3(64), 0, st, (const snes::WindowSlot *)r.d_slots, (const snes::GuideMember *)s->guide->d_mem, (const uint8_t *)c0->d_colors, (int)ntile, (int)g->G, (int)c0->W,
                       (int)c0->sub_size, g->own, own_counts, (const int *)w->d_dead, 1);
    hipLaunchKernelGGL(ksgw_cost_diff, dim3(snes::kGuideColors / 256, slices < 8 ? slices : 8, K), dim3(256), 0, st, (const snes::GuideOwnPixel *)g->own, (const unsigned int *)own_counts, (int)g->G, tabD,
                       (const int *)w->d_dead, 1);
    HIPCHK(hipGetLastError());
    *A = tabA; *D = tabD; *subs = nsub;
    return SNES_OK;
}

// The shortlists of the window's K calls into r.d_cand, the errors kw_gen_candidates presets preset to +inf.
int32_t sgw_generate(snesimage_shared *s, WindowRec &r, uint32_t K, uint32_t k) {
    unsigned long long *A = nullptr, *D = nullptr; uint32_t subs = 0;
    CHECK(sgw_tables(s, r, K, &A, &D, &subs));
    hipLaunchKernelGGL(ksgw_select, dim3(K), dim3(1024), 0, s->b->stream, (const snes::WindowSlot *)r.d_slots, (const int *)s->win->g_work->d_plan, (const unsigned long long *)A, (const unsigned long long *)D,
                       (const uint8_t *)members(s)[0]->d_colors, (int)k, r.d_cand, r.d_errs, (const int *)s->win->d_dead, 1);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

} // namespace

extern "C" {

// snesimage_shared_run_slots' loop with the guided sweep's slot order in the scheduler's place and sg_step_async in snesimage_shared_step_async's.
int32_t snesimage_shared_guided_run_slots(snesimage_shared *s, uint32_t n_calls, uint32_t k, uint32_t *palette, uint32_t *index, uint32_t window, snesimage_call_result *log, snesimage_run_stats *stats) {
    if (!s || !palette || !index) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s));
    CHECK(sg_check(s, *palette, *index, k));
    if (k == 0) k = 16;
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const uint32_t F = (uint32_t)M.size(), kmax = shared_window_kmax(s);
    const bool windows = window != 1 && kmax >= 2 && s->guide_proxy == SNES_GUIDE_REDMEAN; // (more members than slot contexts, and the CIELAB proxy, which has no batched generator: call by call)
    if (windows && n_calls) { // the workspace first: a refusal leaves the set as it was
        CHECK(sg_ready(s, k));
        CHECK(shared_window_reserve(s, 1, 0));
        CHECK(sgw_alloc(s));
        if (!s->win->g_adapt) s->win->g_adapt = kmax < kWindowMin ? kmax : kWindowMin;
    }
    const SharedWindowGen gen{k, guided_next_slot, sgw_generate};
    if (s->guide_capture) { s->guide_captured.assign((size_t)n_calls * k * 3, 0xffu); s->guide_captured_k = k; }
    snesimage_run_stats S{};
    hipStream_t st = s->b->stream;
    uint32_t done = 0;
    while (done < n_calls) {
        bool synced = true;
        for (auto *c : M) synced = synced && c->map_synced;
        const bool tied = s->backdrop && *palette == c0->sub_count;
        if (!windows || !synced || tied || (window == 0 && s->win->g_adapt == 1)) {
            // One call on its own: what the windows do not cover, the tied slot, a first call from maps that are not optimize() of the
            // palette, and a phase in which the size policy finds one call per launch set fastest
            CHECK(sg_step_async(s, *palette, *index, k));
            snesimage_call_result r;
            CHECK(snesimage_shared_last_step(s, &r));
            if (s->guide_capture) { // (the list the scorers read: every member holds it)
                HIPCHK(hipMemcpyAsync(s->guide_captured.data() + (size_t)done * k * 3, c0->d_cand, (size_t)k * 3, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
            }
            guided_next_slot(c0, palette, index);
            if (log) log[done] = r;
            S.calls++; S.windows++; S.scored += k; S.useful += k; if (r.changed) S.accepted++;
            done++;
            continue;
        }
        uint32_t K = window ? window : s->win->g_adapt;
        if (K > n_calls - done) K = n_calls - done;
        if (K > kmax) K = kmax;
        CHECK(sg_ready(s, k)); // (the member table, should a call on its own have moved it)
        uint32_t taken = 0, n = 0, used = 0, acc = 0;
        CHECK(shared_window_run(s, K, 0, 0, *palette, *index, 0, 0, k, log ? log + done : nullptr, &taken, &n, &used, &acc, &gen));
        if (s->guide_capture && used) { // the lists of the calls that took effect, from where the scorers read them
            HIPCHK(hipMemcpyAsync(s->guide_captured.data() + (size_t)done * k * 3, s->win->rec.d_cand, (size_t)used * k * 3, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        for (uint32_t j = 0; j < used; j++) guided_next_slot(c0, palette, index);
        done += used;
        S.calls += used; S.windows++; S.scored += (uint64_t)taken * n; S.useful += (uint64_t)used * n; S.accepted += acc;
        // The weight of a call in WindowPolicy::next: its F scorings, and the form of the single image's guided windows
        // (guided_window_host.inc: four scorings at 8,192 pixels per subpalette, in proportion to the pixels) scaled by the pixels
        // per subpalette over all members.  Chosen between two by measurement (BASELINE.md, "Guided calls of a set through the slot
        // windows").  The other was fitted to the clean windows there — a call adds 0.04 ms per member and 0.015 ms per 1,024 pixels
        // of its own list, a window costs 0.57 ms and 0.0135 ms per 1,024 pixels of a subpalette: weights of 1.4 to 3 where this form
        // gives 9 to 36 — and lost from the k-means start, where two calls in three accept and the policy's estimate of the
        // acceptance rate lags: 1.60 / 1.16 / 0.78 k calls/s at 2 / 4 / 8 frames of 256 x 224 at 8 x 15 against 1.72 / 1.35 / 0.84 k
        // with this form (the parent's sweep: 1.63 / 1.21 / 0.82 k); at the converged state the two were level within 4 %.
        // Speed only: results do not depend on the size.
        const double weight = (double)F + 4.0 * ((double)F * (double)c0->npx / (double)c0->sub_count) / 8192.0;
        s->win->g_adapt = s->win->g_policy.next(used, acc, kGuidedWindowMin < kmax ? kGuidedWindowMin : kmax, kmax, 1, taken, weight);
    }
    if (stats) *stats = S;
    return SNES_OK;
}

int32_t snesimage_shared_debug_guided_capture(snesimage_shared *s, int32_t on) {
    if (!s) return fail(SNES_ERR_ARG, "null set");
    s->guide_capture = on != 0;
    if (!on) { s->guide_captured.clear(); s->guide_captured_k = 0; }
    return SNES_OK;
}

int32_t snesimage_shared_debug_guided_shortlists(snesimage_shared *s, uint8_t *rgb5, uint32_t cap, uint32_t *n_calls, uint32_t *k) {
    if (!s) return fail(SNES_ERR_ARG, "null set");
    const size_t bytes = s->guide_captured.size();
    if (n_calls) *n_calls = s->guide_captured_k ? (uint32_t)(bytes / (3 * (size_t)s->guide_captured_k)) : 0u;
    if (k) *k = s->guide_captured_k;
    if (rgb5) {
        if ((size_t)cap < bytes) return fail(SNES_ERR_ARG, "the buffer is shorter than the captured shortlists");
        if (bytes) memcpy(rgb5, s->guide_captured.data(), bytes);
    }
    return SNES_OK;
}

// The window generator's tables for the n given calls as one window, nothing scored or committed: costs[j * 32768 + u] = A + D of call j.
int32_t snesimage_shared_debug_guided_window_costs(snesimage_shared *s, const uint32_t *palettes, const uint32_t *indices, uint32_t n, uint64_t *costs) {
    CHECK(shared_enter(s, true, true)); // (the generator reads targets, tile_palettes and the palette: the stored maps are not read)
    if (!palettes || !indices || !costs) return fail(SNES_ERR_ARG, "null pointer");
    const snesimage_ctx *c0 = members(s)[0];
    if (n == 0 || n > shared_window_kmax(s)) return fail(SNES_ERR_ARG, "a guided window of this set holds 1 .. " + std::to_string(shared_window_kmax(s)) + " calls");
    for (uint32_t j = 0; j < n; j++) {
        CHECK(sg_check(s, palettes[j], indices[j], 0));
        if (s->backdrop && palettes[j] == c0->sub_count) return fail(SNES_ERR_ARG, "the tied slot is never a window's: it is stepped on its own");
    }
    if (s->guide_proxy != SNES_GUIDE_REDMEAN) return fail(SNES_ERR_UNSUPPORTED, "the guided windows have no CIELAB generator");
    CHECK(sg_ready(s, 1));
    CHECK(shared_window_reserve(s, n, 0));
    CHECK(sgw_alloc(s));
    CHECK(sg_order(s));
    hipStream_t st = s->b->stream;
    WindowRec &r = s->win->rec;
    r.h_slots = reinterpret_cast<snes::WindowSlot *>(r.h_blob); r.d_slots = reinterpret_cast<snes::WindowSlot *>(r.d_blob);
    for (uint32_t j = 0; j < n; j++) {
        snes::WindowSlot &sl = r.h_slots[j];
        sl.method = SNES_METHOD_RANDOM; sl.n = 0; sl.slot = (int)(palettes[j] * c0->sub_size + indices[j]); sl.channel = 0; sl.nes = 0; sl.member = -1; sl.key = 0; sl.cand0 = 0; sl.pad = 0;
    }
    HIPCHK(hipMemcpyAsync(r.d_blob, r.h_blob, window_slots_bytes(n), hipMemcpyHostToDevice, st));
    unsigned long long *A = nullptr, *D = nullptr; uint32_t subs = 0;
    CHECK(sgw_tables(s, r, n, &A, &D, &subs));
    std::vector<uint64_t> shared((size_t)snes::kGuideColors * subs);
    HIPCHK(hipMemcpyAsync(shared.data(), A, sizeof(uint64_t) * shared.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(costs, D, sizeof(uint64_t) * snes::kGuideColors * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t j = 0; j < n; j++) { // what ksgw_select ranks
        const uint64_t *a = shared.data() + (size_t)snes::kGuideColors * s->win->g_work->h_plan[j];
        for (int u = 0; u < snes::kGuideColors; u++) costs[(size_t)j * snes::kGuideColors + u] += a[u];
    }
    return SNES_OK;
}

} // extern "C"
