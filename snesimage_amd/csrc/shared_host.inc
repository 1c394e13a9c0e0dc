// snesimage_amd/csrc/shared_host.inc — one palette shared by several images (DESIGN §5b).  Included by capi.hip after
// batch_host.inc.  A set is an image batch (it borrows its members the same way: `owner`, the batch's stream, its ring of
// argument blocks) whose optimizer calls give every member the same candidate list and commit once on the joint error
// (ks_commit, kernels_shared.hpp).  The k-means initialisers run on the member stack — the members top to bottom in
// member order, W x F*H — with the point order of the reference's own initialisers over that picture.

struct snesimage_shared_window; // slot windows of the set (shared_window_host.inc)
struct snesimage_sharedchar;    // workspace of the set's character budget (shared_char_host.inc)
struct snesimage_sharedlevel;   // workspace of the set's per-tile dither levels (shared_level_host.inc)
struct snesimage_guidework;     // workspace and generator of guided calls, a context's and the set's (guide_host.inc)
namespace { void shared_window_free(snesimage_shared_window *w); void shared_char_free(snesimage_sharedchar *w); void shared_level_free(snesimage_sharedlevel *w); void guide_free(snesimage_guidework *&w); }

struct snesimage_shared {
    snesimage_batch *b = nullptr;
    snesimage_shared_window *win = nullptr;   // slot contexts and records of snesimage_shared_run_slots, made on first use
    snes::StepResult *d_joint = nullptr;      // the set's record of the last call (error = E)
    double *d_sum = nullptr; uint32_t sum_cap = 0; // snesimage_shared_score_candidates: E_k
    const double **d_tab = nullptr;           // the members' error vectors, for ks_sum
    std::vector<unsigned long long> epoch;    // each member's palette / tile-map generation when the set last touched it
    snesimage_sharedchar *chr = nullptr;      // the character budget of the set, made on first use
    snesimage_sharedlevel *lvl = nullptr;     // the tied level calls of the set, made on first use
    snesimage_guidework *guide = nullptr;     // the guided calls of the set, made on first use
    uint32_t guide_proxy = 0;                 // snesimage_shared_set_guided_proxy: the set's own, the members' are neither read nor written
    bool guide_capture = false; std::vector<uint8_t> guide_captured; uint32_t guide_captured_k = 0; // snesimage_shared_debug_guided_capture: the last run's shortlists (shared_guided_window_host.inc)
    bool reduced = false;                     // snesimage_shared_reduce_characters left merged maps: stored maps that are no optimize() of the palette
    // a backdrop set (snesimage_shared_create_backdrop; DESIGN §5c''): every member is a SNES_BACKDROP context and holds the set's B
    bool backdrop = false;
    hipEvent_t ev_tied = nullptr;             // orders the members' streams and the set's around a call on the backdrop slot
    snes::TiedMember *d_tied = nullptr; std::vector<snes::TiedMember> h_tied; // ks_commit_tied's member table, and what it holds
};

namespace {

std::vector<snesimage_ctx *> &members(snesimage_shared *s) { return s->b->ctx; }

// What a backdrop set does not carry yet: the character budget, the refit, the set tilemap and the per-tile dither levels.
int32_t shared_refuse_backdrop(snesimage_shared *s, const char *call) {
    if (s && s->backdrop) return fail(SNES_ERR_UNSUPPORTED, std::string(call) + " is not supported on a backdrop set (snesimage_shared_create_backdrop): the character budget, the refit, the set tilemap and the per-tile dither levels do not carry the backdrop colour yet");
    return SNES_OK;
}

// Every set call starts here: the set is intact, and no member was changed behind its back since the set last touched it.
// wait: the call works on the members outside the batched launches, so the set's stream must be idle first.
// A character reduction is the last stage of a run: every call that optimizes first gives each member that received a merge
// its optimize() and its incumbent back (what shared_settle leaves), so the batched launches never meet an unsynced member.
// keep_merged: the call only reads the members as they stand (the error, the character calls) and leaves the merged maps.
int32_t shared_enter(snesimage_shared *s, bool wait = true, bool keep_merged = false) {
    if (!s) return fail(SNES_ERR_ARG, "null set");
    if (s->b->dead) return fail(SNES_ERR_STATE, "a member context of this set was destroyed");
    auto &M = members(s);
    for (size_t i = 0; i < M.size(); i++)
        if (M[i]->epoch != s->epoch[i] || M[i]->pend || M[i]->win_pend)
            return fail(SNES_ERR_STATE, "member " + std::to_string(i) + " of the set was changed outside it (its palette, tile palettes or map): the members no longer share one state");
    HIPCHK(hipSetDevice(s->b->device));
    if (s->reduced && !keep_merged) {
        CHECK(batch_quiesce(s->b));
        for (auto *c : M) {
            CHECK(ensure_tables(c));
            CHECK(ensure_source(c));
            if (!c->map_synced) CHECK(do_optimize(c));
            CHECK(ensure_incumbent(c));
        }
        for (auto *c : M) HIPCHK(hipStreamSynchronize(c->stream));
        s->reduced = false;
    }
    return wait ? batch_quiesce(s->b) : SNES_OK;
}

// After a set call that changed the members outside the batched launches: everything a batched call takes for granted
// (as snesimage_batch_create leaves it), then the members' generations are recorded.
int32_t shared_settle(snesimage_shared *s) {
    auto &M = members(s);
    for (auto *c : M) {
        CHECK(ensure_tables(c));
        CHECK(ensure_source(c));
        if (!c->map_synced) CHECK(do_optimize(c));
        CHECK(ensure_incumbent(c));
    }
    for (size_t i = 0; i < M.size(); i++) { HIPCHK(hipStreamSynchronize(M[i]->stream)); s->epoch[i] = M[i]->epoch; }
    return SNES_OK;
}

// The palette of every member := rgb5 (as snesimage_set_palette_rgb5 does: on a backdrop set the sub_count * user_size regular
// entries, B stays); optimize() follows in shared_settle.
int32_t shared_put_palette(snesimage_shared *s, const uint8_t *rgb5) {
    for (auto *c : members(s)) {
        CHECK(ensure_map(c));
        if (c->backdrop) for (uint32_t p = 0; p < c->sub_count; p++) HIPCHK(hipMemcpyAsync(c->d_colors + 3 * (size_t)p * c->sub_size, rgb5 + 3 * (size_t)p * c->user_size, 3 * (size_t)c->user_size, hipMemcpyHostToDevice, c->stream));
        else
        HIPCHK(hipMemcpyAsync(c->d_colors, rgb5, 3 * (size_t)c->ncol, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->tables_valid = false; c->pack_valid = false; c->inc_valid = false; c->map_synced = false; c->epoch++; c->epoch_by_commit = false;
    }
    return SNES_OK;
}

// The regular entries of member 0's palette, sub_count * user_size of them: the whole palette of a plain context, the expanded
// palette without its tied column of a backdrop context.
int32_t shared_read_regular(snesimage_ctx *c0, std::vector<uint8_t> &col) {
    std::vector<uint8_t> all(3 * (size_t)c0->ncol);
    HIPCHK(hipMemcpyAsync(all.data(), c0->d_colors, all.size(), hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(hipStreamSynchronize(c0->stream));
    col.resize(3 * (size_t)c0->sub_count * c0->user_size);
    for (uint32_t p = 0; p < c0->sub_count; p++) memcpy(&col[3 * (size_t)p * c0->user_size], &all[3 * (size_t)p * c0->sub_size], 3 * (size_t)c0->user_size);
    return SNES_OK;
}

// recalculate_palette(p) (lib.rs:330-405) over the member stack for every p in `which`: the points of subpalette p are the
// opaque pixels of every tile that uses it, member after member, tiles row-major, x outer and y inner within a tile
// (pixel coordinates of the stack: member i's row y is row i*H + y).  One k-means problem per subpalette on member 0's
// workspace, the points gathered there from every member's planes; the colours go to every member.
int32_t shared_kmeans_recalculate(snesimage_shared *s, const std::vector<uint32_t> &which) {
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const size_t F = M.size();
    std::vector<std::vector<uint8_t>> tp(F, std::vector<uint8_t>(1024));
    for (size_t i = 0; i < F; i++) {
        snesimage_ctx *c = M[i];
        if (c->perceptual) CHECK(ensure_source(c)); // per-pixel Lab
        HIPCHK(hipMemcpyAsync(tp[i].data(), c->d_tile_pal, 1024, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    const uint32_t wt = c0->W / 8, ht = c0->H / 8;
    struct Run { size_t member; long long off, n; };
    std::vector<uint32_t> index; std::vector<Run> runs;
    std::vector<int> n; std::vector<long long> off;
    for (uint32_t palette : which) {
        off.push_back((long long)index.size());
        for (size_t i = 0; i < F; i++) {
            const long long r0 = (long long)index.size();
            for (uint32_t tile = 0; tile < 1024; tile++) {
                if (tp[i][tile] != palette) continue;
                const uint32_t tx = tile % wt, ty = tile / wt;
                if (ty >= ht) continue;
                for (uint32_t x = 0; x < 8; x++)
                    for (uint32_t y = 0; y < 8; y++) {
                        const uint32_t px = (ty * 8 + y) * c0->W + tx * 8 + x;
                        if (M[i]->h_orig[4 * (size_t)px + 3] > 0) index.push_back(px);
                    }
            }
            if ((long long)index.size() > r0) runs.push_back(Run{i, r0, (long long)index.size() - r0});
        }
        n.push_back((int)((long long)index.size() - off.back()));
    }
    const int k = (int)c0->user_size; // (a backdrop set: the regular entries; B is not an initialiser's to move, as in kmeans_host.inc)
    for (size_t p = 0; p < n.size(); p++)
        if (!(2 <= k && k < n[p])) return fail(SNES_ERR_KMEANS, "k-means precondition 2 <= k < n violated (the reference panics here)");
    CHECK(kmeans_reserve(c0, index.size(), (int)which.size(), k));
    HIPCHK(hipMemcpyAsync(c0->km.d_index, index.data(), sizeof(uint32_t) * index.size(), hipMemcpyHostToDevice, c0->stream));
    for (const Run &r : runs) { // member r.member's pixels, indices local to that member, into their place in the point list
        const snesimage_ctx *c = M[r.member];
        hipLaunchKernelGGL(k_gather_points, dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, c0->stream, c->d_orig, c->d_labpx, c0->km.d_index + r.off, r.n, c->perceptual ? 1 : 0,
                           c0->km.pts + 3 * r.off);
    }
    HIPCHK(hipGetLastError());
    std::vector<double> centres;
    CHECK(kmeans_run(c0, n, off, k, centres, nullptr));
    std::vector<uint8_t> col;
    CHECK(shared_read_regular(c0, col));
    for (size_t p = 0; p < which.size(); p++)
        for (int i = 0; i < k; i++) host_centre_to_color(c0, &centres[3 * (p * k + i)], &col[3 * ((size_t)which[p] * c0->user_size + i)]);
    return shared_put_palette(s, col.data());
}

// initialize_tiles (lib.rs:79-189) over the member stack: the tile means in the reference's order over that picture —
// tile_x outer, the stack's tile rows inner, i.e. for every column of tiles member 0's tiles top to bottom, then member
// 1's, ... (the members interleave column by column) — with its drop rule; k-means with sub_count clusters; the stack's
// tile palettes split back to the members by rows; every entry of subpalette p seeded with centre p.
int32_t shared_kmeans_initialize_tiles(snesimage_shared *s) {
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const size_t F = M.size();
    if (c0->sub_count == 1) return shared_kmeans_recalculate(s, std::vector<uint32_t>{0}); // lib.rs:80-84
    const uint32_t wt = c0->W / 8, ht = c0->H / 8, ntile = wt * ht;
    std::vector<std::vector<float>> sums(F, std::vector<float>(3 * (size_t)ntile));
    std::vector<std::vector<int>> counts(F, std::vector<int>(ntile));
    for (size_t i = 0; i < F; i++) { // every member's tile sums on its own stream and workspace (a tile's sums are its own pixels')
        snesimage_ctx *c = M[i];
        if (c->perceptual) CHECK(ensure_source(c));
        CHECK(kmeans_reserve(c, 1, 1, (int)c->sub_count));
        hipLaunchKernelGGL(k_unit_sums, dim3((ntile + 63) / 64), dim3(64), 0, c->stream, (const uint8_t *)c->d_orig, (const float *)c->d_labpx, (int)c->W, (int)c->H, c->perceptual ? 1 : 0, 0, 0,
                           c->km.d_sums, c->km.d_counts); // (the members of a set hold 1 x 1 blocks: tiles)
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sums[i].data(), c->km.d_sums, sizeof(float) * sums[i].size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(counts[i].data(), c->km.d_counts, sizeof(int) * counts[i].size(), hipMemcpyDeviceToHost, c->stream));
    }
    for (auto *c : M) HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<double> means; std::vector<std::pair<size_t, uint32_t>> map; // (member, tile) of every point
    for (uint32_t tx = 0; tx < wt; tx++)
        for (size_t i = 0; i < F; i++)
            for (uint32_t ty = 0; ty < ht; ty++) {
                const uint32_t index = ty * wt + tx;
                const float *sm = &sums[i][3 * (size_t)index];
                if (sm[0] + sm[1] + sm[2] > 0.0f) { // lib.rs:118
                    for (int q = 0; q < 3; q++) means.push_back((double)sm[q] / (double)counts[i][index]);
                    map.emplace_back(i, index);
                }
            }
    const int k = (int)c0->sub_count;
    std::vector<int> n{(int)map.size()}; std::vector<long long> off{0};
    if (!(2 <= k && k < n[0])) return fail(SNES_ERR_KMEANS, "k-means precondition 2 <= k < n violated (the reference panics here)");
    CHECK(kmeans_reserve(c0, map.size(), 1, k));
    HIPCHK(hipMemcpyAsync(c0->km.pts, means.data(), sizeof(double) * means.size(), hipMemcpyHostToDevice, c0->stream));
    std::vector<double> centres; std::vector<uint32_t> assign;
    CHECK(kmeans_run(c0, n, off, k, centres, &assign));
    std::vector<std::vector<uint8_t>> tp(F, std::vector<uint8_t>(1024));
    for (size_t i = 0; i < F; i++) {
        HIPCHK(hipMemcpyAsync(tp[i].data(), M[i]->d_tile_pal, 1024, hipMemcpyDeviceToHost, M[i]->stream));
        HIPCHK(hipStreamSynchronize(M[i]->stream));
    }
    for (size_t t = 0; t < map.size(); t++) tp[map[t].first][map[t].second] = (uint8_t)assign[t]; // lib.rs:133-138
    std::vector<uint8_t> col(3 * (size_t)c0->sub_count * c0->user_size); // (the regular entries: all there is in a plain set)
    for (int i = 0; i < k; i++) {
        uint8_t color[3];
        host_centre_to_color(c0, &centres[3 * (size_t)i], color);
        for (uint32_t j = 0; j < c0->user_size; j++) memcpy(&col[3 * ((size_t)i * c0->user_size + j)], color, 3); // lib.rs:181-183
    }
    for (size_t i = 0; i < F; i++) {
        HIPCHK(hipMemcpyAsync(M[i]->d_tile_pal, tp[i].data(), 1024, hipMemcpyHostToDevice, M[i]->stream));
        HIPCHK(hipStreamSynchronize(M[i]->stream));
    }
    return shared_put_palette(s, col.data());
}

// One optimizer call on the backdrop slot of a backdrop set (DESIGN §5c'').  A backdrop call leaves no row group untouched, so
// the group-sparse launches gain nothing: every member scores the one candidate list — snesimage_step's for (seed, step_id) —
// through its own dense tied path (SlotScope, pack mode 3) on its own stream, behind whatever the set's stream still holds,
// so the members overlap; ks_commit_tied follows on the set's stream behind the members' events.  With SNES_DITHER every
// member then takes the winner's map from its lanes (k_take_best_map + do_optimize(may_skip), as commit() does for a single
// context) on its own stream, and the set's stream waits for that.  No host synchronisation once the workspaces exist.
// gen: the set's generator in gen_candidates' place (a guided call, shared_guide_host.inc).  It runs ONCE, on the set's stream,
// and writes the list into every member's d_cand.  It reads the members' targets and tile_palettes (constant during set calls)
// and the palette, which ks_commit / ks_commit_tied write on the set's stream: stream order covers that.  It overwrites the
// lists the members' score_list of the previous call read on their own streams: the set's stream waited for those (ev_own)
// before that call's commit — or, when the set's stream is idle, waits for the members' streams here.  Every member's stream
// then waits for the generator (ev_tied) before prep_for_slot / score_list.
int32_t shared_tied_call(snesimage_shared *s, uint32_t method, uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_random, const BatchGen *gen = nullptr) {
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    if (method > 2 || channel > 2) return fail(SNES_ERR_ARG, "bad method or channel");
    const uint32_t n = method_count(method, n_random), F = (uint32_t)M.size();
    HIPCHK(hipSetDevice(s->b->device));
    hipStream_t st = s->b->stream;
    if (!s->ev_tied) HIPCHK(hipEventCreateWithFlags(&s->ev_tied, hipEventDisableTiming));
    for (auto *c : M)
        if (!c->tables_valid || !c->src_valid || !c->inc_valid) return fail(SNES_ERR_STATE, "a member context was modified outside the set");
    if (gen) {
        if (!s->b->busy) for (auto *c : M) { // work a member queued on its own stream since the last set call (as batch_call orders it)
            if (!c->ev_own) HIPCHK(hipEventCreateWithFlags(&c->ev_own, hipEventDisableTiming));
            HIPCHK(hipEventRecord(c->ev_own, c->stream));
            HIPCHK(hipStreamWaitEvent(st, c->ev_own, 0));
        }
        CHECK(gen->enqueue(gen->self, st, c0->sub_count, 0, n));
        HIPCHK(hipEventRecord(s->ev_tied, st)); // behind the generator, and so behind the batched call before it
    } else
    if (s->b->busy) HIPCHK(hipEventRecord(s->ev_tied, st)); // the batched call before this one may still be running
    std::vector<snes::TiedMember> tab(F);
    for (uint32_t i = 0; i < F; i++) {
        snesimage_ctx *c = M[i];
        if (gen || s->b->busy) HIPCHK(hipStreamWaitEvent(c->stream, s->ev_tied, 0));
        CHECK(ensure_cand_capacity(c, n)); // (a guided call has made room before its generator ran)
        SlotScope sc(c, c->sub_count, 0);
        if (!gen) CHECK(gen_candidates(c, method, sc.sp, sc.si, channel, seed, step_id, n));
        CHECK(prep_for_slot(c, (int)sc.sp, (int)sc.si));
        CHECK(score_list(c, c->d_cand, n, c->d_errs, 1, 0, (int)sc.sp, (int)sc.si, nullptr));
        if (!c->ev_own) HIPCHK(hipEventCreateWithFlags(&c->ev_own, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_own, c->stream));
        HIPCHK(hipStreamWaitEvent(st, c->ev_own, 0));
        snes::TiedMember &a = tab[i];
        a.errors = c->d_errs; a.cand = c->d_cand; a.colors = c->d_colors; a.inc_err = c->d_inc_err; a.last = c->d_last;
        a.T.eotf = c->d_eotf; a.T.lab_eotf = c->d_lab_eotf; a.T.rgb8 = c->d_pal_rgb8; a.T.lin = c->d_pal_lin; a.T.xyb = c->d_pal_xyb; a.T.lab = c->perceptual ? c->d_pal_lab : nullptr;
    }
    if (s->h_tied.size() != F || memcmp(s->h_tied.data(), tab.data(), sizeof(snes::TiedMember) * F) != 0) { // first call, or a member's candidate storage grew
        HIPCHK(hipStreamSynchronize(st));
        if (!s->d_tied) HIPCHK(hipMalloc(&s->d_tied, sizeof(snes::TiedMember) * F));
        HIPCHK(hipMemcpy(s->d_tied, tab.data(), sizeof(snes::TiedMember) * F, hipMemcpyHostToDevice));
        s->h_tied = tab;
    }
    hipLaunchKernelGGL(ks_commit_tied, dim3(1), dim3(256), 0, st, (const snes::TiedMember *)s->d_tied, (int)F, (int)n, method == SNES_METHOD_NES ? 1 : 0, (int)c0->user_size, (int)c0->sub_count,
                       (int)c0->sub_size, s->d_joint);
    HIPCHK(hipGetLastError());
    if (c0->dither) HIPCHK(hipEventRecord(s->ev_tied, st));
    for (auto *c : M) { // what commit() leaves behind in a context after a tied call
        c->pack_valid = false; c->sp.plist_valid = false; c->sp.counters_cleared = false; c->epoch++; c->epoch_by_commit = false;
        if (!c->dither) { c->map_pending = true; c->map_synced = true; c->inc_valid = true; continue; }
        HIPCHK(hipStreamWaitEvent(c->stream, s->ev_tied, 0));
        bool may_skip = false;
        if (c->d_skip) { // the winner's map is optimize() of the committed palette when a lane of this member scored it
            hipLaunchKernelGGL(k_take_best_map, dim3(1), dim3(1024), 0, c->stream, c->d_last, c->d_bestrecs_all, c->best_valid ? (int)c->nlanes : 0, c->d_bestmaps_all, (int)c->npx, 1, c->d_map, c->d_skip);
            may_skip = true;
        }
        c->best_valid = false;
        CHECK(do_optimize(c, may_skip)); // lib.rs:237
        c->inc_valid = true; // ks_commit_tied left the committed state's error in d_inc_err
        HIPCHK(hipEventRecord(c->ev_own, c->stream));
        HIPCHK(hipStreamWaitEvent(st, c->ev_own, 0));
    }
    s->b->busy = true;
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_shared_create(snesimage_ctx **ctxs, uint32_t n, snesimage_shared **out) {
    if (!ctxs || !out || n == 0) return fail(SNES_ERR_ARG, "null pointer or empty set");
    *out = nullptr;
    for (uint32_t i = 0; i < n; i++) {
        if (!ctxs[i]) return fail(SNES_ERR_ARG, "null context in set");
        if (ctxs[i]->group) return fail(SNES_ERR_STATE, "context belongs to a group");
        if (ctxs[i]->backdrop) return fail(SNES_ERR_UNSUPPORTED, kBackdropRefused);
        if (ctxs[i]->od_L > 1) return fail(SNES_ERR_ARG, kLevelsRefused);
        if (blocked(ctxs[i])) return fail(SNES_ERR_UNSUPPORTED, kBlockedRefused);
        for (uint32_t j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) return fail(SNES_ERR_ARG, "a context appears twice in the set");
    }
    // the batch checks the rest (device, size, geometry, chunk, flags, the group-sparse path) and readies every member
    snesimage_batch *b = nullptr;
    CHECK(snesimage_batch_create(ctxs, n, &b));
    std::unique_ptr<snesimage_shared> s(new snesimage_shared());
    s->b = b;
    auto undo = [&](int32_t rc) { snesimage_shared_destroy(s.release()); return rc; };
    std::vector<uint8_t> p0, pi;
    for (uint32_t i = 0; i < n; i++) {
        snesimage_ctx *c = ctxs[i];
        (i ? pi : p0).resize(3 * (size_t)c->ncol);
        if (hipMemcpyAsync((i ? pi : p0).data(), c->d_colors, 3 * (size_t)c->ncol, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return undo(fail(SNES_ERR_HIP, "hipMemcpy failed"));
        if (i && pi != p0) return undo(fail(SNES_ERR_STATE, "the members of a set must hold the same palette (member " + std::to_string(i) + " differs from member 0)"));
    }
    if (hipMalloc(&s->d_joint, sizeof(snes::StepResult)) != hipSuccess || hipMalloc(&s->d_tab, sizeof(double *) * n) != hipSuccess)
        return undo(fail(SNES_ERR_HIP, "hipMalloc failed"));
    s->epoch.resize(n);
    for (uint32_t i = 0; i < n; i++) s->epoch[i] = ctxs[i]->epoch;
    *out = s.release();
    return SNES_OK;
}

// A set of SNES_BACKDROP members that carries B (DESIGN §5c''): the batch's checks through its internal path, the regular
// entries compared, B written to every member, then everything a set call takes for granted (shared_settle).
int32_t snesimage_shared_create_backdrop(snesimage_ctx **ctxs, uint32_t n, const uint8_t *backdrop_rgb5, snesimage_shared **out) {
    if (!ctxs || !out || n == 0) return fail(SNES_ERR_ARG, "null pointer or empty set");
    *out = nullptr;
    for (uint32_t i = 0; i < n; i++) {
        if (!ctxs[i]) return fail(SNES_ERR_ARG, "null context in set");
        if (ctxs[i]->group) return fail(SNES_ERR_STATE, "context belongs to a group");
        if (!ctxs[i]->backdrop) return fail(SNES_ERR_ARG, "member " + std::to_string(i) + " was created without SNES_BACKDROP: a set of plain contexts is made by snesimage_shared_create");
        if (ctxs[i]->od_L > 1) return fail(SNES_ERR_ARG, kLevelsRefused);
        if (blocked(ctxs[i])) return fail(SNES_ERR_UNSUPPORTED, kBlockedRefused);
        for (uint32_t j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) return fail(SNES_ERR_ARG, "a context appears twice in the set");
    }
    if (backdrop_rgb5 && (backdrop_rgb5[0] > 31 || backdrop_rgb5[1] > 31 || backdrop_rgb5[2] > 31)) return fail(SNES_ERR_ARG, "backdrop channels are 5-bit values");
    snesimage_batch *b = nullptr;
    CHECK(batch_create_members(ctxs, n, &b, true));
    std::unique_ptr<snesimage_shared> s(new snesimage_shared());
    s->b = b; s->backdrop = true;
    auto undo = [&](int32_t rc) { std::string keep = g_err; snesimage_shared_destroy(s.release()); g_err = keep; return rc; };
    std::vector<uint8_t> p0, pi;
    for (uint32_t i = 0; i < n; i++) {
        if (shared_read_regular(ctxs[i], i ? pi : p0) != SNES_OK) return undo(SNES_ERR_HIP);
        if (i && pi != p0) return undo(fail(SNES_ERR_STATE, "the members of a set must hold the same palette (the regular entries of member " + std::to_string(i) + " differ from member 0's)"));
    }
    if (hipMalloc(&s->d_joint, sizeof(snes::StepResult)) != hipSuccess || hipMalloc(&s->d_tab, sizeof(double *) * n) != hipSuccess)
        return undo(fail(SNES_ERR_HIP, "hipMalloc failed"));
    uint8_t B[3] = {0, 0, 0};
    if (backdrop_rgb5) memcpy(B, backdrop_rgb5, 3);
    else { // snesimage_create's rule on the member stack
        snesimage_ctx *c0 = ctxs[0];
        unsigned long long sum[3] = {0, 0, 0}, cnt = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t *rgba = ctxs[i]->h_orig.data();
            for (size_t px = 0; px < c0->npx; px++)
                if (rgba[4 * px + 3] != 0) { sum[0] += rgba[4 * px]; sum[1] += rgba[4 * px + 1]; sum[2] += rgba[4 * px + 2]; cnt++; }
        }
        if (cnt) for (int ch = 0; ch < 3; ch++) B[ch] = (uint8_t)(((sum[ch] + cnt / 2) / cnt) >> 3);
        if (c0->nes) { uint8_t raw[3] = {B[0], B[1], B[2]}; host_new_nes_only(raw, c0->perceptual, c0->h_lab_eotf, B); }
    }
    s->epoch.resize(n);
    for (uint32_t i = 0; i < n; i++) { const int32_t rc = write_backdrop(ctxs[i], B); if (rc != SNES_OK) return undo(rc); }
    { const int32_t rc = shared_settle(s.get()); if (rc != SNES_OK) return undo(rc); }
    *out = s.release();
    return SNES_OK;
}

int32_t snesimage_shared_get_backdrop_rgb5(snesimage_shared *s, uint8_t *out) {
    if (!out) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s, true, true));
    if (!s->backdrop) return fail(SNES_ERR_ARG, "the set was created without a backdrop colour (snesimage_shared_create_backdrop)");
    snesimage_ctx *c0 = members(s)[0];
    HIPCHK(hipMemcpyAsync(out, c0->d_colors + 3 * (size_t)c0->user_size, 3, hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(hipStreamSynchronize(c0->stream));
    return SNES_OK;
}

int32_t snesimage_shared_set_backdrop_rgb5(snesimage_shared *s, const uint8_t *in) {
    if (!in) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s));
    if (!s->backdrop) return fail(SNES_ERR_ARG, "the set was created without a backdrop colour (snesimage_shared_create_backdrop)");
    if (in[0] > 31 || in[1] > 31 || in[2] > 31) return fail(SNES_ERR_ARG, "backdrop channels are 5-bit values");
    for (auto *c : members(s)) CHECK(write_backdrop(c, in));
    return shared_settle(s);
}

void snesimage_shared_destroy(snesimage_shared *s) {
    if (!s) return;
    (void)hipSetDevice(s->b->device);
    if (s->b->stream) (void)hipStreamSynchronize(s->b->stream);
    if (s->win) { shared_window_free(s->win); s->win = nullptr; } // (its slot contexts borrow the members' planes: before the members go)
    if (s->chr) { shared_char_free(s->chr); s->chr = nullptr; }
    if (s->lvl) { shared_level_free(s->lvl); s->lvl = nullptr; }
    guide_free(s->guide);
    snesimage_batch_destroy(s->b); // (waits for its stream)
    if (s->d_joint) (void)hipFree(s->d_joint);
    if (s->d_sum) (void)hipFree(s->d_sum);
    if (s->d_tab) (void)hipFree(s->d_tab);
    if (s->d_tied) (void)hipFree(s->d_tied);
    if (s->ev_tied) (void)hipEventDestroy(s->ev_tied);
    delete s;
}

int32_t snesimage_shared_initialize_tiles(snesimage_shared *s) {
    CHECK(shared_enter(s));
    CHECK(shared_kmeans_initialize_tiles(s));
    return shared_settle(s);
}

int32_t snesimage_shared_recalculate_palettes(snesimage_shared *s) { // lib.rs:407-415 over the member stack
    CHECK(shared_enter(s));
    std::vector<uint32_t> which;
    for (uint32_t p = 0; p < members(s)[0]->sub_count; p++) which.push_back(p);
    CHECK(shared_kmeans_recalculate(s, which));
    return shared_settle(s);
}

int32_t snesimage_shared_set_palette_rgb5(snesimage_shared *s, const uint8_t *in) {
    if (!in) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s));
    CHECK(shared_put_palette(s, in));
    return shared_settle(s);
}

int32_t snesimage_shared_error(snesimage_shared *s, double *out) {
    if (!out) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s, true, true));
    double E = 0.0;
    auto &M = members(s);
    for (size_t i = 0; i < M.size(); i++) {
        double e = 0.0;
        CHECK(do_error(M[i], M[i]->d_scratch_err));
        HIPCHK(hipMemcpyAsync(&e, M[i]->d_scratch_err, sizeof(double), hipMemcpyDeviceToHost, M[i]->stream));
        HIPCHK(hipStreamSynchronize(M[i]->stream));
        E = i == 0 ? e : E + e; // member order, as ks_commit sums
    }
    *out = E;
    return SNES_OK;
}

// E_k for an explicit candidate list: every member scores it on its own stream (snesimage_score_candidates_device), ks_sum
// adds the error vectors in member order on the set's stream.  The members are left unchanged.
int32_t snesimage_shared_score_candidates(snesimage_shared *s, uint32_t palette, uint32_t index, const uint8_t *rgb5, uint32_t n, double *errors) {
    if (!rgb5 || !errors) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s, true, true)); // (the candidates are remapped from the palette: the stored maps are not read)
    auto &M = members(s);
    CHECK(check_slot(M[0], palette, index));
    if (n == 0) return SNES_OK;
    if (s->sum_cap < n) {
        if (s->d_sum) { HIPCHK(hipFree(s->d_sum)); s->d_sum = nullptr; s->sum_cap = 0; }
        HIPCHK(hipMalloc(&s->d_sum, sizeof(double) * n));
        s->sum_cap = n;
    }
    std::vector<const double *> tab(M.size());
    for (size_t i = 0; i < M.size(); i++) {
        snesimage_ctx *c = M[i];
        CHECK(ensure_cand_capacity(c, n));
        HIPCHK(hipMemcpyAsync(c->d_cand_sel, rgb5, 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        SlotScope sc(c, palette, index); // (the backdrop slot of a backdrop set: the member's dense tied path)
        CHECK(prep_for_slot(c, (int)sc.sp, (int)sc.si));
        CHECK(score_list(c, c->d_cand_sel, n, c->d_errs_sel, 1, 0, (int)sc.sp, (int)sc.si, nullptr));
        tab[i] = c->d_errs_sel;
    }
    for (auto *c : M) HIPCHK(hipStreamSynchronize(c->stream));
    hipStream_t st = s->b->stream;
    HIPCHK(hipMemcpyAsync(s->d_tab, tab.data(), sizeof(double *) * tab.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ks_sum, dim3((n + 255) / 256), dim3(256), 0, st, s->d_tab, (int)M.size(), (int)n, s->d_sum);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(errors, s->d_sum, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SNES_OK;
}

int32_t snesimage_shared_step_async(snesimage_shared *s, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_random) {
    CHECK(shared_enter(s, false));
    auto &M = members(s);
    if (s->backdrop && palette == M[0]->sub_count && index == 0) { // the backdrop slot
        CHECK(shared_tied_call(s, method, channel, seed, step_id, n_random));
        for (size_t i = 0; i < M.size(); i++) s->epoch[i] = M[i]->epoch;
        return SNES_OK;
    }
    const std::vector<uint64_t> seeds(M.size(), seed); // one candidate list for every member: snesimage_step's for (seed, step_id)
    CHECK(batch_call(s->b, method, palette, index, channel, seeds.data(), step_id, n_random, s->d_joint));
    for (size_t i = 0; i < M.size(); i++) s->epoch[i] = M[i]->epoch;
    return SNES_OK;
}

int32_t snesimage_shared_last_step(snesimage_shared *s, snesimage_call_result *out) {
    if (!s || !out) return fail(SNES_ERR_ARG, "null pointer");
    if (s->b->dead) return fail(SNES_ERR_STATE, "a member context of this set was destroyed");
    HIPCHK(hipSetDevice(s->b->device));
    snes::StepResult r;
    HIPCHK(hipMemcpyAsync(&r, s->d_joint, sizeof(r), hipMemcpyDeviceToHost, s->b->stream));
    HIPCHK(hipStreamSynchronize(s->b->stream));
    s->b->busy = false;
    out->error = r.error; out->best_k = r.best_k; out->rgb5[0] = r.rgb5[0]; out->rgb5[1] = r.rgb5[1]; out->rgb5[2] = r.rgb5[2]; out->changed = r.changed;
    return SNES_OK;
}

int32_t snesimage_shared_step(snesimage_shared *s, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel, uint64_t seed, uint64_t step_id, uint32_t n_random,
                              double *error, uint8_t *best_rgb5) {
    CHECK(snesimage_shared_step_async(s, method, palette, index, channel, seed, step_id, n_random));
    snesimage_call_result r;
    CHECK(snesimage_shared_last_step(s, &r));
    if (error) *error = r.error;
    if (best_rgb5) { best_rgb5[0] = r.rgb5[0]; best_rgb5[1] = r.rgb5[1]; best_rgb5[2] = r.rgb5[2]; }
    return SNES_OK;
}

// Tile reassignment stays per member: a tile's cost depends on its own pixels and the (shared) palette only.
int32_t snesimage_shared_reassign_tiles(snesimage_shared *s, uint32_t *moved) {
    CHECK(shared_enter(s));
    uint32_t total = 0;
    for (auto *c : members(s)) {
        uint32_t m = 0;
        CHECK(snesimage_reassign_tiles(c, &m));
        total += m;
    }
    if (moved) *moved = total;
    return shared_settle(s);
}

} // extern "C"
