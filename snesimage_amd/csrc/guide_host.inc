// snesimage_amd/csrc/guide_host.inc — guided calls: snesimage_guided_costs, snesimage_guided_candidates, snesimage_guided_step(_async),
// snesimage_guided_sweep (definition: include/snesimage_hip.h; kernels: kernels_guide.hpp; DESIGN 5f).
//
// The generator (gather, cost, select) writes the shortlist where k_gen_candidates writes a call's random candidates; from there
// a guided call is snesimage_step_async word for word: prep_for_slot, score_list, commit.  It reads the palette and tile_palettes
// on the device, so the calls of a sweep are enqueued back to back.  Included by capi.hip behind level_host.inc.
// snesimage_set_guided_proxy selects the table's metric: the redmean key (kernels_guide.hpp) or CIEDE2000 in Q16
// (kernels_guide_lab.hpp; DESIGN 5f''); k_guide_select and everything behind it take either table as it is.

struct snesimage_guidework {
    GuidePixel *list = nullptr;          // the population: (w/8)*(h/8)*64 pixels at most, 512 KB at 256 x 256
    GuideLabPixel *lab = nullptr;        // the same population under SNES_GUIDE_CIELAB, 16 bytes a pixel: made when that proxy is first used
    unsigned long long *tab = nullptr;   // cost[32768], the list's tile count (8 bytes), the shortlist's costs [64]
    StepResult *log = nullptr;           // a sweep's records
    unsigned long long *costs() const { return tab; }
    unsigned int *count() const { return reinterpret_cast<unsigned int *>(tab + kGuideColors); }
    unsigned long long *short_costs() const { return tab + kGuideColors + 1; }
};

namespace {

void guide_free(snesimage_ctx *c) { if (c->guide) { dfree(c->guide->list); dfree(c->guide->lab); dfree(c->guide->tab); dfree(c->guide->log); delete c->guide; c->guide = nullptr; } }

int32_t guide_alloc(snesimage_ctx *c) { // all or nothing: a failed allocation leaves the context without a workspace, as it was
    const size_t ntile = (size_t)(c->W / 8) * (c->H / 8);
    if (c->guide) {
        if (c->guide_proxy == SNES_GUIDE_CIELAB && !c->guide->lab && dmalloc(&c->guide->lab, sizeof(GuideLabPixel) * 64 * ntile) != hipSuccess) {
            c->guide->lab = nullptr;
            return fail(SNES_ERR_HIP, "out of device memory for the guided calls' workspace");
        }
        return SNES_OK;
    }
    snesimage_guidework w;
    if (c->guide_proxy == SNES_GUIDE_CIELAB && dmalloc(&w.lab, sizeof(GuideLabPixel) * 64 * ntile) != hipSuccess)
        return fail(SNES_ERR_HIP, "out of device memory for the guided calls' workspace");
    if (dmalloc(&w.list, sizeof(GuidePixel) * 64 * ntile) != hipSuccess || dmalloc(&w.tab, sizeof(unsigned long long) * (kGuideColors + 1 + kGuideShort)) != hipSuccess ||
        dmalloc(&w.log, sizeof(StepResult) * 256) != hipSuccess) {
        dfree(w.list); dfree(w.lab); dfree(w.tab); dfree(w.log);
        return fail(SNES_ERR_HIP, "out of device memory for the guided calls' workspace");
    }
    c->guide = new snesimage_guidework(w);
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

// cost(u) of slot (sp, si) — the context's own terms, see SlotScope — for all 32,768 colours, into the workspace
int32_t guide_costs(snesimage_ctx *c, uint32_t sp, uint32_t si) {
    snesimage_guidework &w = *c->guide;
    const uint32_t ntile = (c->W / 8) * (c->H / 8);
    HIPCHK(hipMemsetAsync(w.tab, 0, sizeof(unsigned long long) * (kGuideColors + 1), c->stream)); // the table and the count
    if (c->guide_proxy == SNES_GUIDE_CIELAB) {
        hipLaunchKernelGGL(k_guide_gather_lab, dim3(ntile), dim3(64), 0, c->stream, (const uint8_t *)c->d_target, (const uint8_t *)c->d_tile_pal, (const uint8_t *)c->d_colors, (const float *)c->d_lab_eotf,
                           (int)c->W, (int)c->sub_size, c->tied_call ? -1 : (int)sp, (int)si, w.lab, w.count());
        hipLaunchKernelGGL(k_guide_cost_lab, dim3(kGuideColors / 256, (ntile * 64 + kGuideSlice - 1) / kGuideSlice), dim3(256), 0, c->stream, (const GuideLabPixel *)w.lab, (const unsigned int *)w.count(),
                           (const float *)c->d_lab_eotf, w.costs());
        HIPCHK(hipGetLastError());
        return SNES_OK;
    }
    hipLaunchKernelGGL(k_guide_gather, dim3(ntile), dim3(64), 0, c->stream, (const uint8_t *)c->d_target, (const uint8_t *)c->d_tile_pal, (const uint8_t *)c->d_colors, (int)c->W, (int)c->sub_size,
                       c->tied_call ? -1 : (int)sp, (int)si, w.list, w.count());
    hipLaunchKernelGGL(k_guide_cost, dim3(kGuideColors / 256, (ntile * 64 + kGuideSlice - 1) / kGuideSlice), dim3(256), 0, c->stream, (const GuidePixel *)w.list, (const unsigned int *)w.count(), w.costs());
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
// ... and the k cheapest but the slot's current colour into c->d_cand, where a call's candidates live
int32_t guide_generate(snesimage_ctx *c, uint32_t sp, uint32_t si, uint32_t k) {
    CHECK(guide_costs(c, sp, si));
    hipLaunchKernelGGL(k_guide_select, dim3(1), dim3(1024), 0, c->stream, (const unsigned long long *)c->guide->costs(), (const uint8_t *)c->d_colors, (int)(sp * c->sub_size + si), (int)k, c->d_cand,
                       c->guide->short_costs());
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

int32_t guide_step_async(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k) { // snesimage_step_async with the generator in gen_candidates' place
    CHECK(ensure_cand_capacity(c, k));
    CHECK(ensure_incumbent(c)); // lib.rs:199
    SlotScope s(c, palette, index);
    CHECK(guide_generate(c, s.sp, s.si, k));
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
    CHECK(guide_alloc(c));
    SlotScope s(c, palette, index);
    CHECK(guide_costs(c, s.sp, s.si));
    HIPCHK(hipMemcpyAsync(costs, c->guide->costs(), sizeof(uint64_t) * kGuideColors, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

int32_t snesimage_guided_candidates(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k, uint8_t *rgb5, uint64_t *costs) {
    CHECK(guide_check(c, palette, index, k));
    if (!rgb5) return fail(SNES_ERR_ARG, "null pointer");
    if (k == 0) k = 16;
    CHECK(set_device(c));
    CHECK(guide_alloc(c));
    CHECK(ensure_cand_capacity(c, k));
    SlotScope s(c, palette, index);
    CHECK(guide_generate(c, s.sp, s.si, k));
    HIPCHK(hipMemcpyAsync(rgb5, c->d_cand, 3 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    if (costs) HIPCHK(hipMemcpyAsync(costs, c->guide->short_costs(), sizeof(uint64_t) * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

int32_t snesimage_guided_step_async(snesimage_ctx *c, uint32_t palette, uint32_t index, uint32_t k) {
    CHECK(guide_check(c, palette, index, k));
    if (k == 0) k = 16;
    CHECK(set_device(c));
    CHECK(guide_alloc(c));
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
    CHECK(guide_alloc(c));
    const uint32_t size = c->backdrop ? c->user_size : c->sub_size;
    const uint32_t n = c->sub_count * size + (c->backdrop ? 1u : 0u); // the schedule's slot order: (p, i) with i inner, the tied slot last
    for (uint32_t j = 0; j < n; j++) {
        const bool tied = j == c->sub_count * size;
        CHECK(guide_step_async(c, tied ? c->sub_count : j / size, tied ? 0u : j % size, k));
        HIPCHK(hipMemcpyAsync(c->guide->log + j, c->d_last, sizeof(StepResult), hipMemcpyDeviceToDevice, c->stream));
    }
    std::vector<StepResult> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), c->guide->log, sizeof(StepResult) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the one synchronisation of the sweep
    snesimage_run_stats S{};
    for (uint32_t j = 0; j < n; j++) {
        if (log) { log[j].error = h[j].error; log[j].best_k = h[j].best_k; memcpy(log[j].rgb5, h[j].rgb5, 3); log[j].changed = h[j].changed; }
        S.calls += 1; S.windows += 1; S.accepted += h[j].changed ? 1u : 0u; S.scored += k; S.useful += k;
    }
    if (stats) *stats = S;
    return SNES_OK;
}

} // extern "C"
