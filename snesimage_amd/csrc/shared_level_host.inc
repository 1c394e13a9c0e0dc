// snesimage_amd/csrc/shared_level_host.inc — per-tile ordered-dither levels of a shared-palette set, tied or per frame:
// snesimage_shared_set_ordered_dither_bank, snesimage_shared_set_tile_levels, snesimage_shared_score_tile_levels,
// snesimage_shared_level_sweep (definition: include/snesimage_hip.h, "tied level call"; kernel: ks_level_commit of
// kernels_level.hpp; DESIGN 5d'').
//
// The set owns the bank; every member holds it and its own levels, and reads its own d_target, so every set path takes such
// members as it takes members with one table.  A tied window is one candidate list for all members — candidate j is "every
// member's tile ltiles[j] on level llevels[j]" — scored by each member as candidate j of its own tile workspace (k_level_remap
// between tile_score_head and tile_score_tail, unchanged, every launch on the set's stream), then ks_level_commit and one
// synchronisation that reads the records.  The per-frame sweep is level_sweep_impl member after member.
// Included by capi.hip last: it uses level_host.inc, the member streams of shared_char_host.inc and sr_incumbents.

struct snesimage_sharedlevel {
    uint32_t cap = 0, F = 0; // candidates (and calls) the arrays hold
    uint16_t *ltiles = nullptr; uint8_t *llevels = nullptr; snes::TileCall *calls = nullptr; unsigned char *result = nullptr; // result: TileWinRes (16 bytes), then cap TileLog records
    snes::SetLevelMember *tab = nullptr;
    std::vector<snes::SetLevelMember> h_tab; // (kept here: the copy to the device may still read it when the filling function returns)
    WindowPolicy policy; uint32_t adapt = 8;
};

namespace {

void shared_level_release(snesimage_sharedlevel *w) { dfree(w->ltiles); dfree(w->llevels); dfree(w->calls); dfree(w->result); dfree(w->tab); w->cap = 0; }
void shared_level_free(snesimage_sharedlevel *w) { shared_level_release(w); delete w; }

// grow-only, all or nothing: a failed grow releases everything (set and members hold nothing of this)
int32_t sl_alloc(snesimage_shared *s, uint32_t need) {
    if (!s->lvl) s->lvl = new snesimage_sharedlevel();
    snesimage_sharedlevel &w = *s->lvl;
    const uint32_t F = (uint32_t)members(s).size();
    if (w.cap >= need && w.F == F) return SNES_OK;
    if (need < 16) need = 16;
    HIPCHK(hipStreamSynchronize(s->b->stream));
    shared_level_release(&w);
    if (dmalloc(&w.ltiles, sizeof(uint16_t) * need) != hipSuccess || dmalloc(&w.llevels, need) != hipSuccess || dmalloc(&w.calls, sizeof(snes::TileCall) * need) != hipSuccess ||
        dmalloc(&w.result, 16 + sizeof(snes::TileLog) * (size_t)need) != hipSuccess || dmalloc(&w.tab, sizeof(snes::SetLevelMember) * F) != hipSuccess) {
        shared_level_release(&w);
        return fail(SNES_ERR_HIP, "out of device memory for the level candidates of the set");
    }
    w.cap = need; w.F = F;
    return SNES_OK;
}

// The set's slot contexts (shared_window_host.inc) borrow the members' target pointers and keep packs of their own; their packs
// are rebuilt from the borrowed pointers by every window's own launches, which is how a tile move of a member reaches them.  So a
// level path reaches them by keeping the pointers the members' and everything kept per slot context invalid.
void sl_reach_slots(snesimage_shared *s) {
    if (!s->win) return;
    auto &M = members(s);
    for (size_t i = 0; i < M.size() && i < s->win->child.size(); i++)
        for (snesimage_ctx *k : s->win->child[i]) {
            const snesimage_ctx *c = M[i];
            k->d_target = c->d_target; k->d_labpx_t = c->d_labpx_t; k->d_labpxT_t = c->d_labpxT_t; k->od_n = c->od_n; memcpy(k->od_tab, c->od_tab, sizeof k->od_tab);
            k->pack_valid = false; k->sp.plist_valid = false; k->sp.counters_cleared = false;
        }
}

// what every entry point checks behind shared_enter: the members hold a bank (the set's: they hold the same one)
int32_t sl_check_bank(snesimage_shared *s) {
    for (auto *c : members(s))
        if (c->od_L == 0) return fail(SNES_ERR_STATE, "no ordered-dither bank is set: call snesimage_shared_set_ordered_dither_bank first");
    return SNES_OK;
}

uint32_t sl_group(snesimage_shared *s) { // candidates of a window: within every member's launch group and the commit's LDS
    uint32_t g = (uint32_t)snes::kSetLevelCands;
    for (auto *c : members(s)) if (tile_group(c) < g) g = tile_group(c);
    return g;
}

// every member ready to score `need` candidates from its stored map (the optimize() of the palette against its T), its incumbent
// known, its own stream idle; then the members' table for the commit
int32_t sl_prepare(snesimage_shared *s, uint32_t need, bool table) {
    for (auto *c : members(s)) {
        const uint8_t *base_map = nullptr;
        CHECK(tile_prepare(c, need, &base_map));
        if (base_map != c->d_map) return fail(SNES_ERR_STATE, "a member of the set holds a stored map that is no optimize() of the palette");
    }
    for (auto *c : members(s)) HIPCHK(hipStreamSynchronize(c->stream));
    if (!table) return SNES_OK;
    snesimage_sharedlevel &w = *s->lvl;
    auto &M = members(s);
    w.h_tab.resize(M.size());
    for (size_t i = 0; i < M.size(); i++) {
        snesimage_ctx *c = M[i];
        w.h_tab[i] = snes::SetLevelMember{c->d_orig, c->d_lab_eotf, c->tile->errs, c->tile->lmaps, c->d_level, c->d_map, c->d_target_own,
                                          c->perceptual ? c->d_labpx_t_own : nullptr, c->perceptual ? c->d_labpxT_t_own : nullptr, c->d_inc_err};
    }
    HIPCHK(hipMemcpyAsync(w.tab, w.h_tab.data(), sizeof(snes::SetLevelMember) * M.size(), hipMemcpyHostToDevice, s->b->stream));
    return SNES_OK;
}

// nc pairs at h_tiles / h_levels, uploaded, and scored by every member: maps into the member's lmaps, errors into its errs[0, nc).
// Under ScStreams; the host arrays stay as they are until the set's stream has been synchronised.
int32_t sl_enqueue(snesimage_shared *s, const uint16_t *h_tiles, const uint8_t *h_levels, uint32_t nc) {
    snesimage_sharedlevel &w = *s->lvl;
    hipStream_t st = s->b->stream;
    HIPCHK(hipMemcpyAsync(w.ltiles, h_tiles, sizeof(uint16_t) * nc, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.llevels, h_levels, nc, hipMemcpyHostToDevice, st));
    for (auto *c : members(s)) CHECK(level_score_pairs(c, w.ltiles, w.llevels, nc, c->d_map, c->tile->errs));
    return SNES_OK;
}

double sl_sum(const double *v, uint32_t F) { double e = 0.0; for (uint32_t m = 0; m < F; m++) e = m == 0 ? v[m] : e + v[m]; return e; } // member order, as ks_level_commit sums

int32_t sl_tied_sweep(snesimage_shared *s, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats &S) {
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const uint32_t F = (uint32_t)M.size(), m = c0->od_L - 1; // candidates per call
    const uint32_t kmax = window_limit(sl_group(s), m, n_tiles, window);
    if (m) CHECK(sl_alloc(s, kmax * m)); // (every allocation comes before the first commit)
    CHECK(sl_prepare(s, kmax * m > 0 ? kmax * m : 1, m != 0));
    hipStream_t st = s->b->stream;
    if (m == 0) { // one table: no candidates, nothing accepted
        std::vector<double> inc; double E = 0.0;
        CHECK(sr_incumbents(s, inc, &E));
        window_idle(n_tiles, E, log, S);
        return SNES_OK;
    }
    snesimage_sharedlevel &w = *s->lvl;
    uint32_t K = window_first(window, w.adapt, kmax);
    struct Flags { bool pack_valid, plist_valid, map_synced, map_pending, inc_valid, best_valid, epoch_by_commit; };
    std::vector<Flags> saved(F);
    WindowCalls wc;
    ScStreams on_set(s);
    // One window.  From the launch of the commit on, every member's stored map may be a candidate's: the flags say "a stored map
    // of unknown error" before anything can fail.  Once the records are read, an accepted call leaves every member as
    // level_sweep_impl leaves a context after an accept, its new epoch recorded in the set; otherwise the flags are put back.
    uint32_t pos = 0;
    while (pos < n_tiles) {
        const uint32_t k = K < n_tiles - pos ? K : n_tiles - pos;
        // (every member is on c0's level: checked before any work, kept by every commit)
        const uint32_t nc = window_build(wc, first_tile + pos, k, c0->od_L, [&](uint32_t tile) { return (uint32_t)c0->od_level[tile]; });
        HIPCHK(hipMemcpyAsync(w.calls, wc.calls.data(), sizeof(snes::TileCall) * k, hipMemcpyHostToDevice, st));
        CHECK(sl_enqueue(s, wc.units.data(), wc.opts.data(), nc));
        for (uint32_t i = 0; i < F; i++) {
            snesimage_ctx *c = M[i];
            saved[i] = Flags{c->pack_valid, c->sp.plist_valid, c->map_synced, c->map_pending, c->inc_valid, c->best_valid, c->epoch_by_commit};
            c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
            c->map_synced = false; c->map_pending = false; c->inc_valid = false; c->best_valid = false;
            s->epoch[i] = c->epoch; // (the set did this: it stays intact whatever follows)
        }
        s->reduced = true; // (until the records are read: stored maps that may be no optimize() of the palette)
        snes::SetLevelCommitParams P{};
        P.tab = w.tab; P.F = (int)F; P.calls = w.calls; P.ncalls = (int)k; P.ncand = (int)nc; P.llevels = w.llevels; P.npx = (int)c0->npx; P.n = (int)c0->od_n; P.W = (int)c0->W; P.H = (int)c0->H;
        P.log = reinterpret_cast<snes::TileLog *>(w.result + 16); P.res = reinterpret_cast<snes::TileWinRes *>(w.result);
        hipLaunchKernelGGL(ks_level_commit, dim3(1), dim3(1024), 0, st, P, level_bank(c0));
        WindowOutcome o{};
        CHECK(window_read_record(st, w.result, wc.res, k, nc, m, F, "level window of the set", log ? log + pos : nullptr, S, o));
        for (uint32_t i = 0; i < F; i++) {
            snesimage_ctx *c = M[i];
            if (o.accepted >= 0) { // as snesimage_shared_set_tile_levels + optimize() would leave the member, with the incumbent error known
                c->od_level[first_tile + pos + (uint32_t)o.accepted] = o.opt;
                c->sp.counters_cleared = false; c->map_synced = true; c->inc_valid = true;
                if (c->win)
                    for (auto &set : c->win->child)
                        for (snesimage_ctx *kc : set) { kc->pack_valid = false; kc->sp.plist_valid = false; kc->sp.counters_cleared = false; }
                continue;
            }
            const Flags &f = saved[i]; // nothing of this member changed
            c->pack_valid = f.pack_valid; c->sp.plist_valid = f.plist_valid; c->map_synced = f.map_synced; c->map_pending = f.map_pending; c->inc_valid = f.inc_valid; c->best_valid = f.best_valid;
            c->epoch_by_commit = f.epoch_by_commit; c->epoch--; s->epoch[i] = c->epoch;
        }
        s->reduced = false; // every stored map is the optimize() of the palette against its member's T again
        if (o.accepted >= 0) sl_reach_slots(s);
        pos += o.used;
        K = window_next(window, K, w.policy, w.adapt, o, kmax, k, 0.2 * (double)m * (double)F);
    }
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_shared_set_ordered_dither_bank(snesimage_shared *s, const int8_t *tables, uint32_t n, uint32_t L, uint32_t start_level) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_set_ordered_dither_bank"));
    if (!s) return fail(SNES_ERR_ARG, "null set");
    const bool off = L == 0 || n == 0;
    if (!off) {
        if (n != 2 && n != 4 && n != 8 && n != 16) return fail(SNES_ERR_ARG, "an ordered-dither table is 2, 4, 8 or 16 offsets wide (0 switches it off)");
        if (L > 8) return fail(SNES_ERR_ARG, "an ordered-dither bank holds at most 8 tables");
        if (!tables) return fail(SNES_ERR_ARG, "null bank");
        if (start_level >= L) return fail(SNES_ERR_ARG, "the start level is not a table of the bank");
    }
    CHECK(shared_enter(s)); // (a pending split-phase step or window of a member: SNES_ERR_STATE)
    auto &M = members(s);
    if (!off) for (auto *c : M) if (c->dither) return fail(SNES_ERR_UNSUPPORTED, "the set was created with SNES_DITHER: error diffusion and ordered dithering are alternatives");
    if (s->win && s->win->side) HIPCHK(hipStreamSynchronize(s->win->side)); // nothing of the set may still read the buffers that change hands
    if (off) {
        for (auto *c : M) CHECK(ordered_set_body(c, nullptr, 0));
        sl_reach_slots(s);
        return shared_settle(s);
    }
    // every member's buffers first: a failed allocation leaves every member as it was
    struct Fresh { bool target = false, level = false; };
    std::vector<Fresh> fresh(M.size());
    bool ok = true;
    for (size_t i = 0; i < M.size() && ok; i++) {
        snesimage_ctx *c = M[i];
        if (!c->d_target_own) {
            fresh[i].target = true;
            ok = dmalloc(&c->d_target_own, c->npx * 4) == hipSuccess;
            if (ok && c->perceptual) ok = dmalloc(&c->d_labpx_t_own, c->npx * 3 * 4) == hipSuccess && dmalloc(&c->d_labpxT_t_own, c->npx * 3 * 4) == hipSuccess;
        }
        if (ok && !c->d_level) { fresh[i].level = true; ok = dmalloc(&c->d_level, 1024) == hipSuccess; }
    }
    if (!ok) {
        for (size_t i = 0; i < M.size(); i++) { // (nothing names them yet)
            snesimage_ctx *c = M[i];
            if (fresh[i].target) { dfree(c->d_target_own); dfree(c->d_labpx_t_own); dfree(c->d_labpxT_t_own); }
            if (fresh[i].level) dfree(c->d_level);
        }
        return fail(SNES_ERR_HIP, "out of device memory for the target images of the set");
    }
    int8_t bank[8 * 256] = {};
    for (uint32_t l = 0; l < L; l++) memcpy(bank + 256 * l, tables + (size_t)l * n * n, (size_t)n * n);
    for (auto *c : M) {
        uint8_t level[1024] = {}; // (the rows of tiles below the image stay 0, as in tile_palettes)
        memset(level, (int)start_level, (size_t)(c->W / 8) * (c->H / 8));
        CHECK(level_rebuild(c, bank, n, L, level));
    }
    sl_reach_slots(s);
    return shared_settle(s);
}

int32_t snesimage_shared_set_tile_levels(snesimage_shared *s, uint32_t member, const uint8_t *in) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_set_tile_levels"));
    if (!s || !in) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s));
    auto &M = members(s);
    if (member >= M.size()) return fail(SNES_ERR_ARG, "member beyond the set");
    CHECK(sl_check_bank(s));
    snesimage_ctx *c = M[member];
    const uint32_t ntile = (c->W / 8) * (c->H / 8);
    uint8_t level[1024] = {};
    for (uint32_t t = 0; t < ntile; t++) {
        if (in[t] >= c->od_L) return fail(SNES_ERR_ARG, "tile level beyond the bank");
        level[t] = in[t];
    }
    if (s->win && s->win->side) HIPCHK(hipStreamSynchronize(s->win->side));
    int8_t bank[8 * 256];
    memcpy(bank, c->od_bank, sizeof bank);
    CHECK(level_rebuild(c, bank, c->od_n, c->od_L, level));
    sl_reach_slots(s);
    return shared_settle(s);
}

int32_t snesimage_shared_score_tile_levels(snesimage_shared *s, const uint16_t *tiles, const uint8_t *levels, uint32_t n, double *errors, double *member_errors) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_score_tile_levels"));
    if (!s) return fail(SNES_ERR_ARG, "null set");
    if (!tiles || !levels || !errors) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(shared_enter(s, true, true)); // (the state is left as it is: merged maps of a character reduction are refused below, not replaced)
    CHECK(sl_check_bank(s));
    if (n == 0) return SNES_OK;
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const uint32_t F = (uint32_t)M.size(), ntile = (c0->W / 8) * (c0->H / 8);
    for (uint32_t j = 0; j < n; j++) {
        if (tiles[j] >= ntile) return fail(SNES_ERR_ARG, "tile beyond the image");
        if (levels[j] >= c0->od_L) return fail(SNES_ERR_ARG, "tile level beyond the bank");
    }
    const uint32_t group = n < sl_group(s) ? n : sl_group(s);
    CHECK(sl_alloc(s, group));
    CHECK(sl_prepare(s, group, false));
    hipStream_t st = s->b->stream;
    std::vector<double> e((size_t)n * F), part((size_t)group * F);
    ScStreams on_set(s);
    for (uint32_t j0 = 0; j0 < n; j0 += group) {
        const uint32_t nc = n - j0 < group ? n - j0 : group;
        CHECK(sl_enqueue(s, tiles + j0, levels + j0, nc));
        for (uint32_t m = 0; m < F; m++) HIPCHK(hipMemcpyAsync(part.data() + (size_t)m * group, M[m]->tile->errs, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st)); // the workspaces are free again
        for (uint32_t j = 0; j < nc; j++)
            for (uint32_t m = 0; m < F; m++) e[(size_t)(j0 + j) * F + m] = part[(size_t)m * group + j];
    }
    for (uint32_t j = 0; j < n; j++) errors[j] = sl_sum(&e[(size_t)j * F], F);
    if (member_errors) memcpy(member_errors, e.data(), sizeof(double) * e.size());
    return SNES_OK;
}

int32_t snesimage_shared_level_sweep(snesimage_shared *s, uint32_t first_tile, uint32_t n_tiles, uint32_t window, uint32_t tied, snesimage_tile_result *log, snesimage_run_stats *stats) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_level_sweep"));
    if (!s) return fail(SNES_ERR_ARG, "null set");
    snesimage_run_stats T{};
    if (stats) *stats = T;
    CHECK(shared_enter(s));
    CHECK(sl_check_bank(s));
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    const uint32_t ntile = (c0->W / 8) * (c0->H / 8);
    if (first_tile > ntile || n_tiles > ntile - first_tile) return fail(SNES_ERR_ARG, "tile range beyond the image");
    if (tied)
        for (uint32_t t = first_tile; t < first_tile + n_tiles; t++)
            for (auto *c : M)
                if (c->od_level[t] != c0->od_level[t])
                    return fail(SNES_ERR_STATE, "the members of the set differ in level on tile " + std::to_string(t) + ": a tied level call needs one common level (set it with snesimage_shared_set_tile_levels)");
    if (n_tiles == 0) return SNES_OK;
    CHECK(shared_settle(s)); // an optimize() still owed belongs to the state the candidates are compared with
    int32_t rc = SNES_OK;
    if (tied) {
        rc = sl_tied_sweep(s, first_tile, n_tiles, window, log, T);
    } else {
        size_t i = 0;
        for (auto *c : M) { // each call decided on the member's own error, as snesimage_shared_tile_sweep decides
            snesimage_run_stats S{};
            rc = level_check(c);
            if (rc == SNES_OK) rc = level_sweep_impl(c, first_tile, n_tiles, window, log ? log + i * n_tiles : nullptr, S);
            T.calls += S.calls; T.accepted += S.accepted; T.windows += S.windows; T.scored += S.scored; T.useful += S.useful;
            if (rc != SNES_OK) break;
            i++;
        }
        if (T.accepted) sl_reach_slots(s);
    }
    if (stats) *stats = T; // (a window that fails leaves the accepted calls standing and counted)
    if (rc != SNES_OK) { // the accepted calls stand: the set records them; whatever a failed window left is re-made by the next call that optimizes
        auto &E = s->epoch;
        for (size_t i = 0; i < M.size(); i++) E[i] = M[i]->epoch;
        return rc;
    }
    return shared_settle(s);
}

} // extern "C"
