// snesimage_amd/csrc/shared_guide_host.inc — guided calls of a shared-palette set: snesimage_shared_guided_costs,
// snesimage_shared_guided_candidates, snesimage_shared_guided_step(_async), snesimage_shared_guided_sweep (definition:
// include/snesimage_hip.h; kernels: kernels_guide.hpp; DESIGN 5f').  Included by capi.hip behind guide_host.inc, whose workspace
// and generator (snesimage_guidework) run here over all members.
//
// The generator (k_guide_gather, k_guide_cost, k_guide_select) runs once per call on the set's stream and writes the shortlist
// into every member's candidate list, where kb_gen_candidates writes a batched call's random candidates; from there a guided
// call is snesimage_shared_step_async(SNES_METHOD_RANDOM, ...) word for word: batch_call's scoring launches and ks_commit on a
// regular slot, shared_tied_call and ks_commit_tied on the backdrop slot.  It reads the palette and tile_palettes on the device,
// so the calls of a sweep are enqueued back to back.

namespace {

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

// The workspace, room for k candidates in every member's list, and the member table
int32_t sg_ready(snesimage_shared *s, uint32_t k) {
    auto &M = members(s);
    CHECK(guide_alloc(s->guide, M.size(), M.size() * sg_ntile(s), s->guide_proxy, "out of device memory for the workspace of the set's guided calls"));
    return guide_table(*s->guide, s->b->stream, M, k);
}

// The slot in the members' own terms (SlotScope's rule without its side effect): the backdrop slot is entry user_size of
// subpalette 0, the first of the tied entries, and its population is every tile (sp = -1).
GuideSlot sg_slot(snesimage_shared *s, uint32_t palette, uint32_t index) {
    const snesimage_ctx *c0 = members(s)[0];
    if (s->backdrop && palette == c0->sub_count) return GuideSlot{-1, (int)c0->user_size, (int)c0->user_size};
    return GuideSlot{(int)palette, (int)index, (int)(palette * c0->sub_size + index)};
}
int32_t sg_enqueue(void *self, hipStream_t st, uint32_t palette, uint32_t index, uint32_t n) {
    snesimage_shared *s = static_cast<snesimage_shared *>(self);
    return guide_generate(*s->guide, st, members(s)[0], s->guide_proxy, sg_slot(s, palette, index), n);
}

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
    CHECK(sg_ready(s, k));
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
    CHECK(sg_ready(s, 1));
    CHECK(sg_order(s));
    hipStream_t st = s->b->stream;
    CHECK(guide_costs(*s->guide, st, members(s)[0], s->guide_proxy, sg_slot(s, palette, index)));
    HIPCHK(hipMemcpyAsync(costs, s->guide->costs(), sizeof(uint64_t) * kGuideColors, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SNES_OK;
}

int32_t snesimage_shared_guided_candidates(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k, uint8_t *rgb5, uint64_t *costs) {
    CHECK(shared_enter(s, true, true));
    CHECK(sg_check(s, palette, index, k));
    if (!rgb5) return fail(SNES_ERR_ARG, "null pointer");
    if (k == 0) k = 16;
    CHECK(sg_ready(s, k));
    CHECK(sg_order(s));
    hipStream_t st = s->b->stream;
    CHECK(guide_generate(*s->guide, st, members(s)[0], s->guide_proxy, sg_slot(s, palette, index), k));
    HIPCHK(hipMemcpyAsync(rgb5, members(s)[0]->d_cand, 3 * (size_t)k, hipMemcpyDeviceToHost, st));
    if (costs) HIPCHK(hipMemcpyAsync(costs, s->guide->short_costs(), sizeof(uint64_t) * k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SNES_OK;
}

int32_t snesimage_shared_guided_step_async(snesimage_shared *s, uint32_t palette, uint32_t index, uint32_t k) {
    CHECK(shared_enter(s, false));
    CHECK(sg_check(s, palette, index, k));
    if (k == 0) k = 16;
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
    const snesimage_ctx *c0 = members(s)[0];
    const uint32_t size = s->backdrop ? c0->user_size : c0->sub_size;
    const uint32_t n = c0->sub_count * size + (s->backdrop ? 1u : 0u); // the schedule's slot order: (p, i) with i inner, the tied slot last
    hipStream_t st = s->b->stream;
    for (uint32_t j = 0; j < n; j++) {
        const bool tied = j == c0->sub_count * size;
        CHECK(sg_step_async(s, tied ? c0->sub_count : j / size, tied ? 0u : j % size, k));
        HIPCHK(hipMemcpyAsync(s->guide->log + j, s->d_joint, sizeof(StepResult), hipMemcpyDeviceToDevice, st));
    }
    CHECK(guide_sweep_results(*s->guide, st, n, k, log, stats));
    s->b->busy = false;
    return SNES_OK;
}

} // extern "C"
