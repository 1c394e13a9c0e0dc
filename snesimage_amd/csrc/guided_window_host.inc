// snesimage_amd/csrc/guided_window_host.inc — guided calls through the slot windows: snesimage_guided_run_slots (definition:
// include/snesimage_hip.h; kernels: kernels_guide_window.hpp; DESIGN 5f''').
//
// A guided call's shortlist depends on the palette, tile_palettes and the target image only, none of which a rejected call
// changes: call j+1 sees the state call j saw whenever call j accepted nothing, exactly as a scheduled call does.  So a guided
// window IS a scheduled window (window_host.inc) — the same slot contexts, batched scoring, kw_commit with the random method's
// rule, --dither branch, ring of records, window ahead and d_dead — whose candidate lists are written by the batched generator
// instead of kw_gen_candidates (window_enqueue's `gen` argument: the slot order and the generator are handed in as a WindowGen,
// so window_host.inc names nothing of this file).  Included by capi.hip behind guide_host.inc and window_host.inc.

namespace {

constexpr uint32_t kGuidedWindowMin = 2; // the adaptive size's floor (kWindowMin for the scheduled windows, whose calls cost their scoring only)

// the guided sweep's slot order: index inner, palette outer, the tied slot of a backdrop context last, then (0, 0) again
void guided_next_slot(const snesimage_ctx *c, uint32_t *palette, uint32_t *index) {
    const uint32_t size = c->backdrop ? c->user_size : c->sub_size;
    if (*palette >= c->sub_count) { *palette = 0; *index = 0; return; } // behind the tied slot
    if (++*index < size) return;
    *index = 0;
    if (++*palette == c->sub_count && !c->backdrop) *palette = 0;
}

size_t guided_window_counts() { return ((size_t)window_max() + 1) / 2; } // 64-bit words in front of the tables: they hold a 32-bit count per call, two to a word

// The generator's workspace for window_max() calls: all or nothing.
int32_t guided_window_alloc(snesimage_ctx *c) {
    snesimage_window *w = c->win;
    if (w->g_list) return SNES_OK;
    const size_t ntile = (size_t)(c->W / 8) * (c->H / 8), cap = window_max();
    snes::GuidePixel *list = nullptr; unsigned long long *tab = nullptr;
    if (dmalloc(&list, sizeof(snes::GuidePixel) * 64 * ntile * cap) != hipSuccess || dmalloc(&tab, sizeof(unsigned long long) * (guided_window_counts() + (size_t)snes::kGuideColors * cap)) != hipSuccess) {
        dfree(list); dfree(tab);
        return fail(SNES_ERR_HIP, "out of device memory for the guided windows' workspace");
    }
    w->g_list = list; w->g_tab = tab;
    return SNES_OK;
}

// The shortlists of the window's K calls into r.d_cand, the errors preset to +inf: on the main stream, where kw_gen_candidates
// runs — behind the previous window's commit, so one workspace serves all windows in flight.
int32_t guided_window_generate(snesimage_ctx *c, WindowRec &r, uint32_t K, uint32_t k, double *d_errors) {
    snesimage_window *w = c->win;
    hipStream_t st = c->stream;
    const uint32_t ntile = (c->W / 8) * (c->H / 8);
    unsigned int *counts = reinterpret_cast<unsigned int *>(w->g_tab);
    unsigned long long *costs = w->g_tab + guided_window_counts();
    HIPCHK(hipMemsetAsync(w->g_tab, 0, sizeof(unsigned long long) * (guided_window_counts() + (size_t)snes::kGuideColors * K), st)); // the counts and the K tables
    hipLaunchKernelGGL(kw_guide_gather, dim3(ntile, K), dim3(64), 0, st, (const snes::WindowSlot *)r.d_slots, (const uint8_t *)c->d_target, (const uint8_t *)c->d_tile_pal, (const uint8_t *)c->d_colors, (int)ntile, (int)c->W,
                       (int)c->sub_size, w->g_list, counts, (const int *)w->d_dead, r.base);
    // the host does not know the counts: the grid covers the largest list, every tile
    hipLaunchKernelGGL(kw_guide_cost, dim3(snes::kGuideColors / 256, (ntile * 64 + snes::kGuideSlice - 1) / snes::kGuideSlice, K), dim3(256), 0, st, (const snes::GuidePixel *)w->g_list, (const unsigned int *)counts, (int)ntile,
                       costs, (const int *)w->d_dead, r.base);
    hipLaunchKernelGGL(kw_guide_select, dim3(K), dim3(1024), 0, st, (const snes::WindowSlot *)r.d_slots, (const unsigned long long *)costs, (const uint8_t *)c->d_colors, (int)k, r.d_cand, d_errors,
                       (const int *)w->d_dead, r.base);
    return SNES_OK;
}

} // namespace

extern "C" {

// snesimage_run_slots' loop with the guided sweep's slot order in the scheduler's place and guide_step_async in snesimage_step_async's.
int32_t snesimage_guided_run_slots(snesimage_ctx *c, uint32_t n_calls, uint32_t k, uint32_t *palette, uint32_t *index, uint32_t window, snesimage_call_result *log, snesimage_run_stats *stats) {
    if (!c || !palette || !index) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(guide_check(c, *palette, *index, k));
    if (k == 0) k = 16;
    CHECK(set_device(c));
    snesimage_run_stats S{};
    const bool windows = window_capable(c) && window != 1 && c->guide_proxy == SNES_GUIDE_REDMEAN;
    if (windows && n_calls) { // the workspace first: a refusal leaves the context as it was
        if (!c->win) CHECK(window_reserve(c, 0, 0));
        CHECK(guided_window_alloc(c));
    }
    const WindowGen gen{k, guided_next_slot, guided_window_generate};
    if (c->guide_capture) { c->guide_captured.assign((size_t)n_calls * k * 3, 0xffu); c->guide_captured_k = k; }
    uint32_t done = 0;
    struct Flight { int rec; uint32_t first, taken, p, i; }; // a window in flight and the slot it starts from
    Flight fl[snesimage_window::kRing]; uint32_t nfl = 0; int next_rec = 0; uint32_t win_seq = 0;
    uint32_t q_done = 0, qp = *palette, qi = *index; // where the next window to enqueue starts if all in flight stay clean
    while (done < n_calls) {
        if (!windows || !c->map_synced || (c->backdrop && nfl == 0 && *palette == c->sub_count)) {
            // One call on its own: what the windows do not cover, the tied slot, and a first call from a palette_map that is not optimize() of the palette
            const uint32_t p = *palette, i = *index;
            guided_next_slot(c, palette, index);
            CHECK(guide_step_async(c, p, i, k));
            snes::StepResult r;
            HIPCHK(hipMemcpyAsync(&r, c->d_last, sizeof(r), hipMemcpyDeviceToHost, c->stream));
            if (c->guide_capture) HIPCHK(hipMemcpyAsync(c->guide_captured.data() + (size_t)done * k * 3, c->d_cand, (size_t)k * 3, hipMemcpyDeviceToHost, c->stream)); // (the list the scorer read)
            HIPCHK(hipStreamSynchronize(c->stream));
            if (log) { log[done].error = r.error; log[done].best_k = r.best_k; memcpy(log[done].rgb5, r.rgb5, 3); log[done].changed = r.changed; }
            S.calls++; S.windows++; S.scored += k; S.useful += k; if (r.changed) S.accepted++;
            done++;
            q_done = done; qp = *palette; qi = *index;
            continue;
        }
        CHECK(window_reserve(c, window_max(), 0)); // (argument arrays are never regrown while windows are in flight)
        snesimage_window *w = c->win;
        const uint32_t eff_depth = (w->depth > 1 && w->g_clean_streak >= 2) ? w->depth : 1; // a window ahead only while windows come back clean
        while (nfl < eff_depth && q_done < n_calls && !(c->backdrop && qp == c->sub_count)) { // (the tied slot is stepped on its own once the windows in front of it are in)
            uint32_t K = window ? window : w->g_adapt;
            if (K > n_calls - q_done) K = n_calls - q_done;
            if (K > window_max()) K = window_max();
            const bool ahead = eff_depth > 1;
            if (nfl == 0) {
                CHECK(window_prepare(c, SNES_METHOD_RANDOM));
                if (ahead && w->use_side) { HIPCHK(hipEventRecord(w->ev_ready, c->stream)); HIPCHK(hipStreamWaitEvent(w->side, w->ev_ready, 0)); }
            }
            WindowRec &r = w->rec[next_rec];
            r.seq = w->seq_next++; r.base = nfl ? w->rec[fl[0].rec].seq : r.seq; // void once a window in flight before it has accepted
            CHECK(window_enqueue(c, r, K, 0, 0, qp, qi, 0, 0, k, 0, 1, nullptr, ahead ? (int)(win_seq & 1) : 0, ahead, &gen));
            win_seq++;
            CHECK(window_enqueue_commit(c, r, nullptr, log != nullptr));
            fl[nfl++] = Flight{next_rec, q_done, r.K, qp, qi};
            next_rec = (next_rec + 1) % snesimage_window::kRing;
            for (uint32_t j = 0; j < r.K; j++) guided_next_slot(c, &qp, &qi);
            q_done += r.K;
        }
        // the oldest window's result
        const Flight f = fl[0];
        for (uint32_t j = 1; j < nfl; j++) fl[j - 1] = fl[j];
        nfl--;
        WindowRec &r = w->rec[f.rec];
        uint32_t used = 0, acc = 0;
        CHECK(window_collect(c, r, &used, &acc, log ? log + f.first : nullptr));
        *palette = f.p; *index = f.i;
        for (uint32_t j = 0; j < used; j++) guided_next_slot(c, palette, index);
        if (c->guide_capture && used) { // the lists of the calls that took effect, from where the scorer read them (the record is not enqueued again before the next turn of this loop)
            HIPCHK(hipMemcpyAsync(c->guide_captured.data() + (size_t)f.first * k * 3, r.d_cand, (size_t)used * k * 3, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        done = f.first + used;
        S.calls += used; S.windows++; S.scored += (uint64_t)f.taken * r.stride; S.useful += (uint64_t)used * r.stride; S.accepted += acc;
        if (acc) { // the windows behind it were built for the old palette: the device has voided them, collect and forget them
            for (uint32_t j = 0; j < nfl; j++) { uint32_t u = 0, a = 0; CHECK(window_collect(c, w->rec[fl[j].rec], &u, &a, nullptr)); S.voided++; }
            nfl = 0;
            q_done = done; qp = *palette; qi = *index;
        }
        if (!acc) w->g_clean_streak++; else w->g_clean_streak = 0;
        // A voided guided call wastes its generator as well as its scoring: about four times the scoring of a call at 8,192 pixels
        // per subpalette (BASELINE.md, "Guided calls", Cost: a guided call of 16 takes 0.13 ms more than a random call of 16, which
        // is a window's ~31 us per call four times over), in proportion to the pixels.  So windows shrink further than the
        // scheduled ones while calls are accepted often (measured from the k-means start, 25 % acceptance, 256 x 256: windows of
        // 8 and more ran at 2.3 k calls/s against 2.6 k call by call).  Speed only: results do not depend on the size.
        const double weight = 1.0 + 4.0 * ((double)c->npx / (double)c->sub_count) / 8192.0;
        w->g_adapt = w->g_policy.next(used, acc, kGuidedWindowMin, window_max(), 1, f.taken, weight);
    }
    if (stats) *stats = S;
    return SNES_OK;
}

int32_t snesimage_debug_guided_capture(snesimage_ctx *c, int32_t on) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    c->guide_capture = on != 0;
    if (!on) { c->guide_captured.clear(); c->guide_captured_k = 0; }
    return SNES_OK;
}

int32_t snesimage_debug_guided_shortlists(snesimage_ctx *c, uint8_t *rgb5, uint32_t cap, uint32_t *n_calls, uint32_t *k) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    const size_t bytes = c->guide_captured.size();
    if (n_calls) *n_calls = c->guide_captured_k ? (uint32_t)(bytes / (3 * (size_t)c->guide_captured_k)) : 0u;
    if (k) *k = c->guide_captured_k;
    if (rgb5) {
        if ((size_t)cap < bytes) return fail(SNES_ERR_ARG, "the buffer is shorter than the captured shortlists");
        if (bytes) memcpy(rgb5, c->guide_captured.data(), bytes);
    }
    return SNES_OK;
}

} // extern "C"
