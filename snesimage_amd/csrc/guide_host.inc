// snesimage_amd/csrc/guide_host.inc — guided calls: snesimage_guided_costs, snesimage_guided_candidates, snesimage_guided_step(_async),
// snesimage_guided_sweep (definition: include/snesimage_hip.h; kernels: kernels_guide.hpp; DESIGN 5f), and the workspace and
// generator that the guided calls of a set (shared_guide_host.inc) run as well: a single image is a set of one.
//
// The generator (k_guide_gather, k_guide_cost, k_guide_select) writes the shortlist where k_gen_candidates writes a call's random
// candidates; from there a guided call is snesimage_step_async word for word: prep_for_slot, score_list, commit.  It reads the
// palette and tile_palettes on the device, so the calls of a sweep are enqueued back to back.  Included by capi.hip behind level_host.inc.
// snesimage_set_guided_proxy selects the table's metric: the redmean key (kernels_guide.hpp) or CIEDE2000 in Q16
// (kernels_guide_lab.hpp; DESIGN 5f''); k_guide_select and everything behind it take either table as it is.

struct snesimage_guidework {
    GuidePixel *list = nullptr;          // the population: 64 pixels per global tile (512 KB at 256 x 256, 4 MB at kSetTiles)
    GuideLabPixel *lab = nullptr;        // the same population under SNES_GUIDE_CIELAB, 16 bytes a pixel: made when that proxy is first used
    unsigned long long *tab = nullptr;   // cost[32768], the list's tile count (8 bytes), the shortlist's costs [64]
    StepResult *log = nullptr;           // a sweep's records (256: a palette holds at most 253 entries and B)
    GuideMember *d_mem = nullptr;        // the member table, and what it holds
    std::vector<GuideMember> h_mem;
    unsigned long long *costs() const { return tab; }
    unsigned int *count() const { return reinterpret_cast<unsigned int *>(tab + kGuideColors); }
    unsigned long long *short_costs() const { return tab + kGuideColors + 1; }
};

namespace {

void guide_free(snesimage_guidework *&w) { if (w) { dfree(w->list); dfree(w->lab); dfree(w->tab); dfree(w->log); dfree(w->d_mem); delete w; w = nullptr; } }

// The workspace of F members and G global tiles; the CIELAB list joins it when that proxy is first used.  All or nothing: a
// failed allocation leaves the owner without a workspace (or without the CIELAB list), as it was.  oom: the owner's error text.
int32_t guide_alloc(snesimage_guidework *&w, size_t F, size_t G, uint32_t proxy, const char *oom) {
    if (w) {
        if (proxy == SNES_GUIDE_CIELAB && !w->lab && dmalloc(&w->lab, sizeof(GuideLabPixel) * 64 * G) != hipSuccess) { w->lab = nullptr; return fail(SNES_ERR_HIP, oom); }
        return SNES_OK;
    }
    snesimage_guidework n;
    if (proxy == SNES_GUIDE_CIELAB && dmalloc(&n.lab, sizeof(GuideLabPixel) * 64 * G) != hipSuccess) return fail(SNES_ERR_HIP, oom);
    if (dmalloc(&n.list, sizeof(GuidePixel) * 64 * G) != hipSuccess || dmalloc(&n.tab, sizeof(unsigned long long) * (kGuideColors + 1 + kGuideShort)) != hipSuccess ||
        dmalloc(&n.log, sizeof(StepResult) * 256) != hipSuccess || dmalloc(&n.d_mem, sizeof(GuideMember) * F) != hipSuccess) {
        dfree(n.list); dfree(n.lab); dfree(n.tab); dfree(n.log); dfree(n.d_mem);
        return fail(SNES_ERR_HIP, oom);
    }
    w = new snesimage_guidework(n);
    return SNES_OK;
}

// Room for k candidates in every member's list, and the member table on the device.  The table changes on the first call and
// when a member's candidate storage grew or its target moved (an ordered-dither table or a level bank set or cleared): then, and
// only then, the stream is awaited.  The copy goes through that stream, behind the launches that still read the old table: a
// hipMemcpy would open the null stream, whose hardware queue a context's scoring streams then share (measured on an MI355X: the
// random calls of 16 and of 64 behind it 0.33 - 0.57 ms against 0.27 - 0.35 at 256 x 256).
int32_t guide_table(snesimage_guidework &w, hipStream_t st, const std::vector<snesimage_ctx *> &M, uint32_t k) {
    std::vector<GuideMember> tab(M.size());
    for (size_t i = 0; i < M.size(); i++) {
        CHECK(ensure_cand_capacity(M[i], k));
        tab[i].target = M[i]->d_target; tab[i].tile_pal = M[i]->d_tile_pal; tab[i].cand = M[i]->d_cand;
    }
    if (w.h_mem.size() != tab.size() || memcmp(w.h_mem.data(), tab.data(), sizeof(GuideMember) * tab.size()) != 0) {
        w.h_mem.clear();
        HIPCHK(hipMemcpyAsync(w.d_mem, tab.data(), sizeof(GuideMember) * tab.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        w.h_mem = tab;
    }
    return SNES_OK;
}

// A slot in the members' own terms: entry si of the subpalette, entry `slot` of the palette; its population is the tiles of
// subpalette sp, or every tile (sp = -1: the backdrop slot).
struct GuideSlot { int sp, si, slot; };

// cost(u) of the slot over the members of the table, for all 32,768 colours, into the workspace; on stream st.  c0: the first
// member (the members' geometry, palette and sRGB tables are one: the first member's serve all).
int32_t guide_costs(snesimage_guidework &w, hipStream_t st, const snesimage_ctx *c0, uint32_t proxy, GuideSlot q) {
    const uint32_t ntile = (c0->W / 8) * (c0->H / 8), G = (uint32_t)w.h_mem.size() * ntile;
    // the host does not know the count: the cost grids cover the largest list, G * 64 pixels (at most 512 slices at kSetTiles)
    const dim3 grid(kGuideColors / 256, (G * 64 + kGuideSlice - 1) / kGuideSlice);
    HIPCHK(hipMemsetAsync(w.tab, 0, sizeof(unsigned long long) * (kGuideColors + 1), st)); // the table and the count
    if (proxy == SNES_GUIDE_CIELAB) {
        hipLaunchKernelGGL(k_guide_gather_lab, dim3(G), dim3(64), 0, st, (const GuideMember *)w.d_mem, (const uint8_t *)c0->d_colors, (const float *)c0->d_lab_eotf, (int)ntile, (int)c0->W, (int)c0->sub_size,
                           q.sp, q.si, w.lab, w.count());
        hipLaunchKernelGGL(k_guide_cost_lab, grid, dim3(256), 0, st, (const GuideLabPixel *)w.lab, (const unsigned int *)w.count(), (const float *)c0->d_lab_eotf, w.costs());
    } else {
        hipLaunchKernelGGL(k_guide_gather, dim3(G), dim3(64), 0, st, (const GuideMember *)w.d_mem, (const uint8_t *)c0->d_colors, (int)ntile, (int)c0->W, (int)c0->sub_size, q.sp, q.si, w.list, w.count());
        hipLaunchKernelGGL(k_guide_cost, grid, dim3(256), 0, st, (const GuidePixel *)w.list, (const unsigned int *)w.count(), w.costs());
    }
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
// ... and the k cheapest but the slot's current colour into every member's d_cand, where a call's candidates live
int32_t guide_generate(snesimage_guidework &w, hipStream_t st, const snesimage_ctx *c0, uint32_t proxy, GuideSlot q, uint32_t k) {
    CHECK(guide_costs(w, st, c0, proxy, q));
    hipLaunchKernelGGL(k_guide_select, dim3(1), dim3(1024), 0, st, (const unsigned long long *)w.costs(), (const uint8_t *)c0->d_colors, q.slot, (int)k, (const GuideMember *)w.d_mem, (int)w.h_mem.size(),
                       w.short_costs());
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

// The n records of a sweep, in the workspace's log, as the caller's log and statistics; the one synchronisation of the sweep.
int32_t guide_sweep_results(snesimage_guidework &w, hipStream_t st, uint32_t n, uint32_t k, snesimage_call_result *log, snesimage_run_stats *stats) {
    std::vector<StepResult> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), w.log, sizeof(StepResult) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    snesimage_run_stats S{};
    for (uint32_t j = 0; j < n; j++) {
        if (log) { log[j].error = h[j].error; log[j].best_k = h[j].best_k; memcpy(log[j].rgb5, h[j].rgb5, 3); log[j].changed = h[j].changed; }
        S.calls += 1; S.windows += 1; S.accepted += h[j].changed ? 1u : 0u; S.scored += k; S.useful += k;
    }
    if (stats) *stats = S;
    return SNES_OK;
}

int32_t guide_check(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k) {
    CHECK(check_slot(c, palette, index));
    if (k > (uint32_t)kGuideShort) return fail(SNES_ERR_ARG, "a guided shortlist holds at most 64 candidates (0 = 16)");
    if (c->nes) return fail(SNES_ERR_UNSUPPORTED, "the context was created with SNES_NES: its NES call already scores all 56 colours of the table");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first");
    if (c->owner || c->group) return fail(SNES_ERR_STATE, "the context is lent to a batch, a set or a group: guided calls run on a context of its own");
    return SNES_OK;
}

// The workspace, room for k candidates, and the context's one-entry member table
int32_t guide_ready(snesimage_ctx *c, uint32_t k) {
    CHECK(guide_alloc(c->guide, 1, (size_t)(c->W / 8) * (c->H / 8), c->guide_proxy, "out of device memory for the guided calls' workspace"));
    return guide_table(*c->guide, c->stream, {c}, k);
}

// the scope's slot — the context's own terms, see SlotScope — for the generator
GuideSlot guide_slot(const SlotScope &s) { return GuideSlot{s.c->tied_call ? -1 : (int)s.sp, (int)s.si, (int)(s.sp * s.c->sub_size + s.si)}; }

int32_t guide_step_async(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k) { // snesimage_step_async with the generator in gen_candidates' place
    CHECK(guide_ready(c, k));
    CHECK(ensure_incumbent(c)); // lib.rs:199
    SlotScope s(c, palette, index);
    CHECK(guide_generate(*c->guide, c->stream, c, c->guide_proxy, guide_slot(s), k));
    CHECK(prep_for_slot(c, (int)s.sp, (int)s.si));
    CHECK(score_list(c, c->d_cand, k, c->d_errs, 1, 0, (int)s.sp, (int)s.si, nullptr));
    CHECK(commit(c, c->d_errs, k, SNES_METHOD_RANDOM, s.sp, s.si));
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_set_guided_proxy(snesimage_ctx *c, uint32_t proxy) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (proxy != SNES_GUIDE_REDMEAN && proxy != SNES_GUIDE_CIELAB) return fail(SNES_ERR_ARG, "a guided proxy is SNES_GUIDE_REDMEAN (0) or SNES_GUIDE_CIELAB (1)");
    if (c->nes) return fail(SNES_ERR_UNSUPPORTED, "the context was created with SNES_NES: it makes no guided calls");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first");
    if (c->owner || c->group) return fail(SNES_ERR_STATE, "the context is lent to a batch, a set or a group: guided calls run on a context of its own");
    c->guide_proxy = proxy;
    return SNES_OK;
}

int32_t snesimage_get_guided_proxy(snesimage_ctx *c, uint32_t *proxy) {
    if (!c || !proxy) return fail(SNES_ERR_ARG, "null pointer");
    *proxy = c->guide_proxy;
    return SNES_OK;
}

int32_t snesimage_guided_costs(snesimage_ctx *c, uint32_t palette, uint32_t index, uint64_t *costs) {
    CHECK(guide_check(c, palette, index, 0));
    if (!costs) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(set_device(c));
    CHECK(guide_ready(c, 1));
    SlotScope s(c, palette, index);
    CHECK(guide_costs(*c->guide, c->stream, c, c->guide_proxy, guide_slot(s)));
    HIPCHK(hipMemcpyAsync(costs, c->guide->costs(), sizeof(uint64_t) * kGuideColors, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

int32_t snesimage_guided_candidates(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k, uint8_t *rgb5, uint64_t *costs) {
    CHECK(guide_check(c, palette, index, k));
    if (!rgb5) return fail(SNES_ERR_ARG, "null pointer");
    if (k == 0) k = 16;
    CHECK(set_device(c));
    CHECK(guide_ready(c, k));
    SlotScope s(c, palette, index);
    CHECK(guide_generate(*c->guide, c->stream, c, c->guide_proxy, guide_slot(s), k));
    HIPCHK(hipMemcpyAsync(rgb5, c->d_cand, 3 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    if (costs) HIPCHK(hipMemcpyAsync(costs, c->guide->short_costs(), sizeof(uint64_t) * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

int32_t snesimage_guided_step_async(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k) {
    CHECK(guide_check(c, palette, index, k));
    if (k == 0) k = 16;
    CHECK(set_device(c));
    return guide_step_async(c, palette, index, k);
}

int32_t snesimage_guided_step(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k, double *best_error, uint8_t *best_rgb5) {
    CHECK(snesimage_guided_step_async(c, palette, index, k));
    return snesimage_last_step(c, best_error, best_rgb5, nullptr);
}

int32_t snesimage_guided_sweep(snesimage_ctx *c, uint32_t k, snesimage_call_result *log, snesimage_run_stats *stats) {
    CHECK(guide_check(c, 0, 0, k));
    if (k == 0) k = 16;
    CHECK(set_device(c));
    const uint32_t size = c->backdrop ? c->user_size : c->sub_size;
    const uint32_t n = c->sub_count * size + (c->backdrop ? 1u : 0u); // the schedule's slot order: (p, i) with i inner, the tied slot last
    for (uint32_t j = 0; j < n; j++) {
        const bool tied = j == c->sub_count * size;
        CHECK(guide_step_async(c, tied ? c->sub_count : j / size, tied ? 0u : j % size, k));
        HIPCHK(hipMemcpyAsync(c->guide->log + j, c->d_last, sizeof(StepResult), hipMemcpyDeviceToDevice, c->stream));
    }
    return guide_sweep_results(*c->guide, c->stream, n, k, log, stats);
}

} // extern "C"
