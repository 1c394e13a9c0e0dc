// snesimage_amd/csrc/shared_guide_host.inc — guided calls of a shared-palette set: snesimage_shared_guided_costs,
// snesimage_shared_guided_candidates, snesimage_shared_guided_step(_async), snesimage_shared_guided_sweep (definition:
// include/snesimage_hip.h; kernels: kernels_guide_set.hpp; DESIGN 5f').  Included by capi.hip behind guide_host.inc.
//
// The generator (ks_guide_gather, k_guide_cost, ks_guide_select) runs once per call on the set's stream and writes the shortlist
// into every member's candidate list, where kb_gen_candidates writes a batched call's random candidates; from there a guided
// call is snesimage_shared_step_async(SNES_METHOD_RANDOM, ...) word for word: batch_call's scoring launches and ks_commit on a
// regular slot, shared_tied_call and ks_commit_tied on the backdrop slot.  It reads the palette and tile_palettes on the device,
// so the calls of a sweep are enqueued back to back.

struct snesimage_sharedguide {
    GuidePixel *list = nullptr;          // the population: 64 pixels per global tile, 4 MB at kSetTiles
    GuideLabPixel *lab = nullptr;        // the same under SNES_GUIDE_CIELAB, 16 bytes a pixel (8 MB at kSetTiles): made when that proxy is first used
    unsigned long long *tab = nullptr;   // cost[32768], the list's tile count (8 bytes), the shortlist's costs [64]
    StepResult *log = nullptr;           // a sweep's records (256: a palette holds at most 253 entries and B)
    GuideMember *d_mem = nullptr;        // the member table, and what it holds
    std::vector<GuideMember> h_mem;
    unsigned long long *costs() const { return tab; }
    unsigned int *count() const { return reinterpret_cast<unsigned int *>(tab + kGuideColors); }
    unsigned long long *short_costs() const { return tab + kGuideColors + 1; }
};

namespace {

void shared_guide_free(snesimage_sharedguide *w) { if (w) { dfree(w->list); dfree(w->lab); dfree(w->tab); dfree(w->log); dfree(w->d_mem); delete w; } }

uint32_t sg_ntile(snesimage_shared *s) { const snesimage_ctx *c0 = members(s)[0]; return (c0->W / 8) * (c0->H / 8); }

// What every entry point checks behind shared_enter; a refusal leaves the set as it was.
int32_t sg_check(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k) {
    auto &M = members(s);
    CHECK(check_slot(M[0], palette, index)); // (the backdrop slot on a plain set is out of range, as snesimage_shared_step refuses it)
    if (k > (uint32_t)kGuideShort) return fail(SNES_ERR_ARG, "a guided shortlist holds at most 64 candidates (0 = 16)");
    if (M[0]->nes) return fail(SNES_ERR_UNSUPPORTED, "the members were created with SNES_NES: their NES call already scores all 56 colours of the table");
    if ((uint64_t)M.size() * sg_ntile(s) > (uint64_t)kSetTiles)
        return fail(SNES_ERR_UNSUPPORTED, "the guided calls of a set hold at most 8192 tiles in all (this set: " + std::to_string((uint64_t)M.size() * sg_ntile(s)) + "): a cost must stay below 2^49");
    return SNES_OK;
}

int32_t sg_alloc(snesimage_shared *s) { // all or nothing: a failed allocation leaves the set without a workspace, as it was
    const size_t F = members(s).size(), G = F * sg_ntile(s);
    if (s->guide) {
        if (s->guide_proxy == SNES_GUIDE_CIELAB && !s->guide->lab && dmalloc(&s->guide->lab, sizeof(GuideLabPixel) * 64 * G) != hipSuccess) {
            s->guide->lab = nullptr;
            return fail(SNES_ERR_HIP, "out of device memory for the workspace of the set's guided calls");
        }
        return SNES_OK;
    }
    snesimage_sharedguide w;
    if (s->guide_proxy == SNES_GUIDE_CIELAB && dmalloc(&w.lab, sizeof(GuideLabPixel) * 64 * G) != hipSuccess)
        return fail(SNES_ERR_HIP, "out of device memory for the workspace of the set's guided calls");
    if (dmalloc(&w.list, sizeof(GuidePixel) * 64 * G) != hipSuccess || dmalloc(&w.tab, sizeof(unsigned long long) * (kGuideColors + 1 + kGuideShort)) != hipSuccess ||
        dmalloc(&w.log, sizeof(StepResult) * 256) != hipSuccess || dmalloc(&w.d_mem, sizeof(GuideMember) * F) != hipSuccess) {
        dfree(w.list); dfree(w.lab); dfree(w.tab); dfree(w.log); dfree(w.d_mem);
        return fail(SNES_ERR_HIP, "out of device memory for the workspace of the set's guided calls");
    }
    s->guide = new snesimage_sharedguide(w);
    return SNES_OK;
}

// Room for k candidates in every member's list, and the member table on the device.  The table changes on the first call and
// when a member's candidate storage grew or its target moved: then, and only then, the set's stream is awaited.
int32_t sg_table(snesimage_shared *s, uint32_t k) {
    auto &M = members(s);
    snesimage_sharedguide &w = *s->guide;
    std::vector<GuideMember> tab(M.size());
    for (size_t i = 0; i < M.size(); i++) {
        CHECK(ensure_cand_capacity(M[i], k));
        tab[i].target = M[i]->d_target; tab[i].tile_pal = M[i]->d_tile_pal; tab[i].cand = M[i]->d_cand;
    }
    if (w.h_mem.size() != tab.size() || memcmp(w.h_mem.data(), tab.data(), sizeof(GuideMember) * tab.size()) != 0) {
        HIPCHK(hipStreamSynchronize(s->b->stream));
        w.h_mem.clear();
        HIPCHK(hipMemcpy(w.d_mem, tab.data(), sizeof(GuideMember) * tab.size(), hipMemcpyHostToDevice));
        w.h_mem = tab;
    }
    return SNES_OK;
}

// The slot in the members' own terms (SlotScope's rule without its side effect): the backdrop slot is entry user_size of
// subpalette 0, the first of the tied entries, and its population is every tile (sp = -1).
struct SgSlot { int sp, si, slot; };
SgSlot sg_slot(snesimage_shared *s, uint32_t palette, uint32_t index) {
    const snesimage_ctx *c0 = members(s)[0];
    if (s->backdrop && palette == c0->sub_count) return SgSlot{-1, (int)c0->user_size, (int)c0->user_size};
    return SgSlot{(int)palette, (int)index, (int)(palette * c0->sub_size + index)};
}

// cost(u) of the slot over all members, for all 32,768 colours, into the workspace; on stream st.
int32_t sg_costs(snesimage_shared *s, hipStream_t st, uint32_t palette, uint32_t index) {
    snesimage_sharedguide &w = *s->guide;
    const snesimage_ctx *c0 = members(s)[0];
    const uint32_t ntile = sg_ntile(s), G = (uint32_t)members(s).size() * ntile;
    const SgSlot q = sg_slot(s, palette, index);
    HIPCHK(hipMemsetAsync(w.tab, 0, sizeof(unsigned long long) * (kGuideColors + 1), st)); // the table and the count
    if (s->guide_proxy == SNES_GUIDE_CIELAB) { // (the members' sRGB tables are one table: the first member's serves all)
        hipLaunchKernelGGL(ks_guide_gather_lab, dim3(G), dim3(64), 0, st, (const GuideMember *)w.d_mem, (const uint8_t *)c0->d_colors, (const float *)c0->d_lab_eotf, (int)ntile, (int)c0->W, (int)c0->sub_size,
                           q.sp, q.si, w.lab, w.count());
        hipLaunchKernelGGL(k_guide_cost_lab, dim3(kGuideColors / 256, (G * 64 + kGuideSlice - 1) / kGuideSlice), dim3(256), 0, st, (const GuideLabPixel *)w.lab, (const unsigned int *)w.count(),
                           (const float *)c0->d_lab_eotf, w.costs());
        HIPCHK(hipGetLastError());
        return SNES_OK;
    }
    hipLaunchKernelGGL(ks_guide_gather, dim3(G), dim3(64), 0, st, (const GuideMember *)w.d_mem, (const uint8_t *)c0->d_colors, (int)ntile, (int)c0->W, (int)c0->sub_size, q.sp, q.si, w.list, w.count());
    // the host does not know the count: the grid covers the largest list, G * 64 pixels (at most 512 slices at kSetTiles)
    hipLaunchKernelGGL(k_guide_cost, dim3(kGuideColors / 256, (G * 64 + kGuideSlice - 1) / kGuideSlice), dim3(256), 0, st, (const GuidePixel *)w.list, (const unsigned int *)w.count(), w.costs());
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
// ... and the k cheapest but the slot's current colour into every member's d_cand
int32_t sg_generate(snesimage_shared *s, hipStream_t st, uint32_t palette, uint32_t index, uint32_t k) {
    CHECK(sg_costs(s, st, palette, index));
    const snesimage_ctx *c0 = members(s)[0];
    hipLaunchKernelGGL(ks_guide_select, dim3(1), dim3(1024), 0, st, (const unsigned long long *)s->guide->costs(), (const uint8_t *)c0->d_colors, sg_slot(s, palette, index).slot, (int)k,
                       (const GuideMember *)s->guide->d_mem, (int)members(s).size(), s->guide->short_costs());
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
int32_t sg_enqueue(void *self, hipStream_t st, uint32_t palette, uint32_t index, uint32_t n) { return sg_generate(static_cast<snesimage_shared *>(self), st, palette, index, n); }

// The set's stream behind whatever the members still hold on their own (as batch_call orders a call when the stream is idle).
int32_t sg_order(snesimage_shared *s) {
    if (s->b->busy) return SNES_OK;
    for (auto *c : members(s)) {
        if (!c->ev_own) HIPCHK(hipEventCreateWithFlags(&c->ev_own, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_own, c->stream));
        HIPCHK(hipStreamWaitEvent(s->b->stream, c->ev_own, 0));
    }
    return SNES_OK;
}

// snesimage_shared_step_async(SNES_METHOD_RANDOM, ...) with the set's generator in kb_gen_candidates' / gen_candidates' place
int32_t sg_step_async(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k) {
    auto &M = members(s);
    CHECK(sg_table(s, k));
    const BatchGen gen{sg_enqueue, s};
    if (s->backdrop && palette == M[0]->sub_count && index == 0) CHECK(shared_tied_call(s, SNES_METHOD_RANDOM, 0, 0, 0, k, &gen));
    else {
        const std::vector<uint64_t> seeds(M.size(), 0); // (unused: the generator draws nothing)
        CHECK(batch_call(s->b, SNES_METHOD_RANDOM, palette, index, 0, seeds.data(), 0, k, s->d_joint, &gen));
    }
    for (size_t i = 0; i < M.size(); i++) s->epoch[i] = M[i]->epoch;
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_shared_set_guided_proxy(snesimage_shared *s, uint32_t proxy) {
    CHECK(shared_enter(s, true, true)); // (nothing on the device is touched)
    if (proxy != SNES_GUIDE_REDMEAN && proxy != SNES_GUIDE_CIELAB) return fail(SNES_ERR_ARG, "a guided proxy is SNES_GUIDE_REDMEAN (0) or SNES_GUIDE_CIELAB (1)");
    if (members(s)[0]->nes) return fail(SNES_ERR_UNSUPPORTED, "the members were created with SNES_NES: the set makes no guided calls");
    s->guide_proxy = proxy;
    return SNES_OK;
}

int32_t snesimage_shared_get_guided_proxy(snesimage_shared *s, uint32_t *proxy) {
    if (!s || !proxy) return fail(SNES_ERR_ARG, "null pointer");
    *proxy = s->guide_proxy;
    return SNES_OK;
}

int32_t snesimage_shared_guided_costs(snesimage_shared *s, uint32_t palette, uint32_t index, uint64_t *costs) {
    CHECK(shared_enter(s, true, true)); // (the generator reads targets, tile_palettes and the palette: the stored maps are not read)
    CHECK(sg_check(s, palette, index, 0));
    if (!costs) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(sg_alloc(s));
    CHECK(sg_table(s, 1));
    CHECK(sg_order(s));
    hipStream_t st = s->b->stream;
    CHECK(sg_costs(s, st, palette, index));
    HIPCHK(hipMemcpyAsync(costs, s->guide->costs(), sizeof(uint64_t) * kGuideColors, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SNES_OK;
}

int32_t snesimage_shared_guided_candidates(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k, uint8_t *rgb5, uint64_t *costs) {
    CHECK(shared_enter(s, true, true));
    CHECK(sg_check(s, palette, index, k));
    if (!rgb5) return fail(SNES_ERR_ARG, "null pointer");
    if (k == 0) k = 16;
    CHECK(sg_alloc(s));
    CHECK(sg_table(s, k));
    CHECK(sg_order(s));
    hipStream_t st = s->b->stream;
    CHECK(sg_generate(s, st, palette, index, k));
    HIPCHK(hipMemcpyAsync(rgb5, members(s)[0]->d_cand, 3 * (size_t)k, hipMemcpyDeviceToHost, st));
    if (costs) HIPCHK(hipMemcpyAsync(costs, s->guide->short_costs(), sizeof(uint64_t) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SNES_OK;
}

int32_t snesimage_shared_guided_step_async(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k) {
    CHECK(shared_enter(s, false));
    CHECK(sg_check(s, palette, index, k));
    if (k == 0) k = 16;
    CHECK(sg_alloc(s));
    return sg_step_async(s, palette, index, k);
}

int32_t snesimage_shared_guided_step(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k, double *error, uint8_t *best_rgb5) {
    CHECK(snesimage_shared_guided_step_async(s, palette, index, k));
    snesimage_call_result r;
    CHECK(snesimage_shared_last_step(s, &r));
    if (error) *error = r.error;
    if (best_rgb5) { best_rgb5[0] = r.rgb5[0]; best_rgb5[1] = r.rgb5[1]; best_rgb5[2] = r.rgb5[2]; }
    return SNES_OK;
}

int32_t snesimage_shared_guided_sweep(snesimage_shared *s, uint32_t k, snesimage_call_result *log, snesimage_run_stats *stats) {
    CHECK(shared_enter(s, false));
    CHECK(sg_check(s, 0, 0, k));
    if (k == 0) k = 16;
    CHECK(sg_alloc(s));
    const snesimage_ctx *c0 = members(s)[0];
    const uint32_t size = s->backdrop ? c0->user_size : c0->sub_size;
    const uint32_t n = c0->sub_count * size + (s->backdrop ? 1u : 0u); // the schedule's slot order: (p, i) with i inner, the tied slot last
    hipStream_t st = s->b->stream;
    for (uint32_t j = 0; j < n; j++) {
        const bool tied = j == c0->sub_count * size;
        CHECK(sg_step_async(s, tied ? c0->sub_count : j / size, tied ? 0u : j % size, k));
        HIPCHK(hipMemcpyAsync(s->guide->log + j, s->d_joint, sizeof(StepResult), hipMemcpyDeviceToDevice, st));
    }
    std::vector<StepResult> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), s->guide->log, sizeof(StepResult) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one synchronisation of the sweep
    s->b->busy = false;
    snesimage_run_stats S{};
    for (uint32_t j = 0; j < n; j++) {
        if (log) { log[j].error = h[j].error; log[j].best_k = h[j].best_k; memcpy(log[j].rgb5, h[j].rgb5, 3); log[j].changed = h[j].changed; }
        S.calls += 1; S.windows += 1; S.accepted += h[j].changed ? 1u : 0u; S.scored += k; S.useful += k;
    }
    if (stats) *stats = S;
    return SNES_OK;
}

} // extern "C"
