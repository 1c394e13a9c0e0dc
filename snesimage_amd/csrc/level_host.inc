// snesimage_amd/csrc/level_host.inc — per-tile ordered-dither levels chosen by the objective: snesimage_set_ordered_dither_bank,
// snesimage_set_tile_levels, snesimage_score_tile_levels, snesimage_level_step, snesimage_level_sweep (definition:
// include/snesimage_hip.h; kernels: kernels_level.hpp; DESIGN 5d').
//
// The target image is the aliasing buffer every nearest-colour choice reads (ordered_host.inc), so a context whose T is built
// from a level per tile takes every existing path as it is.  A level candidate's palette_map goes through the tile moves'
// workspace and scorer (tile_prepare / tile_score_head / tile_score_tail); k_level_commit keeps T on the device equal to
// T(level) tile by tile, so a sweep needs no rebuild.  Included by capi.hip behind ordered_host.inc.

struct snesimage_levelwork {
    uint32_t cap = 0; uint16_t *ltiles = nullptr; uint8_t *llevels = nullptr; // the candidates' (tile, level) pairs
    WindowPolicy policy; uint32_t adapt = 8;
};

namespace {

void level_release(snesimage_levelwork *w) { dfree(w->ltiles); dfree(w->llevels); w->cap = 0; }
void level_free(snesimage_ctx *c) { if (c->lvl) { level_release(c->lvl); delete c->lvl; c->lvl = nullptr; } }

int32_t level_alloc(snesimage_ctx *c, uint32_t need) { // grow-only; a failed grow releases both
    if (!c->lvl) c->lvl = new snesimage_levelwork();
    snesimage_levelwork &w = *c->lvl;
    if (w.cap >= need) return SNES_OK;
    if (need < 16) need = 16;
    HIPCHK(hipStreamSynchronize(c->stream));
    level_release(&w);
    if (dmalloc(&w.ltiles, sizeof(uint16_t) * need) != hipSuccess || dmalloc(&w.llevels, need) != hipSuccess) { level_release(&w); return fail(SNES_ERR_HIP, "out of device memory for the level candidates"); }
    w.cap = need;
    return SNES_OK;
}

snes::OrderedBank level_bank(const snesimage_ctx *c) { snes::OrderedBank b; memcpy(b.d, c->od_bank, sizeof b.d); return b; }

int32_t level_check(snesimage_ctx *c) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first (its candidates were scored against the current target image)");
    if (c->od_L == 0) return fail(SNES_ERR_STATE, "no ordered-dither bank is set: call snesimage_set_ordered_dither_bank first");
    return SNES_OK;
}

// T := T(bank, level) for the whole picture, and everything built from T invalid: what both setters do.  The streams are
// waited for first and every buffer belongs to the context as soon as it exists, so a failure leaks nothing; the bank, the
// levels and the pointers change hands only behind the last device call, so a failure in front of that leaves the host state
// as it was (d_target still names what it named).
int32_t level_rebuild(snesimage_ctx *c, const int8_t *bank /* 8 * 256 */, uint32_t n, uint32_t L, const uint8_t *level /* 1024 */) {
    CHECK(set_device(c));
    CHECK(ensure_map(c)); // the owed optimize() belongs to the state before this change
    CHECK(ordered_quiesce(c));
    const bool had = c->d_target_own != nullptr; // (the three target buffers exist together or not at all: the plain setter counts on it)
    bool ok = had || dmalloc(&c->d_target_own, c->npx * 4) == hipSuccess;
    if (ok && !had && c->perceptual) ok = dmalloc(&c->d_labpx_t_own, c->npx * 3 * 4) == hipSuccess && dmalloc(&c->d_labpxT_t_own, c->npx * 3 * 4) == hipSuccess;
    if (ok && !c->d_level) ok = dmalloc(&c->d_level, 1024) == hipSuccess;
    if (!ok) {
        if (!had) { dfree(c->d_target_own); dfree(c->d_labpx_t_own); dfree(c->d_labpxT_t_own); } // (nothing names them yet)
        return fail(SNES_ERR_HIP, "out of device memory for the target image");
    }
    snes::OrderedBank b;
    memcpy(b.d, bank, sizeof b.d);
    HIPCHK(hipMemcpy(c->d_level, level, 1024, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_build_target_levels, dim3((unsigned)((c->npx / 4 + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->d_orig, b, (int)n, (const uint8_t *)c->d_level,
                       (const float *)c->d_lab_eotf, (int)c->W, (int)c->H, c->d_target_own, c->d_labpx_t_own, c->d_labpxT_t_own);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(c->od_bank, bank, sizeof c->od_bank); memcpy(c->od_level, level, sizeof c->od_level);
    c->od_L = L; c->od_n = n; memcpy(c->od_tab, c->od_bank, sizeof c->od_tab);
    c->d_target = c->d_target_own; c->d_labpx_t = c->perceptual ? c->d_labpx_t_own : c->d_labpx; c->d_labpxT_t = c->perceptual ? c->d_labpxT_t_own : c->d_labpxT;
    ordered_invalidate(c);
    return SNES_OK;
}

int32_t level_setter_check(snesimage_ctx *c) {
    if (c->dither) return fail(SNES_ERR_UNSUPPORTED, "the context was created with SNES_DITHER: error diffusion and ordered dithering are alternatives");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first (its candidates were scored against the current target image)");
    if (c->owner || c->group) return fail(SNES_ERR_STATE, "the context is lent to a batch, a set or a group, whose members share one table: destroy that first");
    return SNES_OK;
}

// nc candidates, pairs at ltiles / llevels [0, nc) in device memory: maps into t.lmaps, errors into d_errors[0, nc)
int32_t level_score_pairs(snesimage_ctx *c, const uint16_t *ltiles, const uint8_t *llevels, uint32_t nc, const uint8_t *base_map, double *d_errors) {
    snesimage_tilework &t = *c->tile;
    tile_score_head(c, nc);
    snes::LevelRemapParams R{};
    R.orig = c->d_orig; R.base_map = base_map; R.tile_pal = c->d_tile_pal; R.pal_rgb8 = c->d_pal_rgb8; R.pal_lab = c->d_pal_lab; R.lab_eotf = c->d_lab_eotf;
    R.ltiles = ltiles; R.llevels = llevels; R.tiles = t.tiles; R.subs = t.subs; R.lmaps = t.lmaps;
    R.W = (int)c->W; R.H = (int)c->H; R.sub_size = (int)c->sub_size; R.perceptual = c->perceptual ? 1 : 0; R.n = (int)c->od_n;
    hipLaunchKernelGGL(k_level_remap, dim3(nc), dim3(256), 0, c->stream, R, level_bank(c));
    return tile_score_tail(c, nc, d_errors, tile_geom(c)); // (the pair k_level_remap wrote is the tile with its own subpalette)
}
// ... the pairs in the context's own arrays
int32_t level_score_group(snesimage_ctx *c, uint32_t nc, const uint8_t *base_map, double *d_errors) { return level_score_pairs(c, c->lvl->ltiles, c->lvl->llevels, nc, base_map, d_errors); }

int32_t level_sweep_impl(snesimage_ctx *c, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats &S) {
    const uint32_t ntile = (c->W / 8) * (c->H / 8);
    if (first_tile > ntile || n_tiles > ntile - first_tile) return fail(SNES_ERR_ARG, "tile range beyond the image");
    CHECK(set_device(c));
    if (n_tiles == 0) return SNES_OK;
    const uint32_t m = c->od_L - 1; // candidates per call
    const uint32_t kmax = window_limit(tile_group(c), m, n_tiles, window);
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, (kmax * m > 0 ? kmax * m : 1), &base_map));
    if (m == 0) return window_idle_ctx(c, n_tiles, log, S); // one table
    CHECK(level_alloc(c, kmax * m));
    snesimage_tilework &t = *c->tile;
    snesimage_levelwork &w = *c->lvl;
    uint32_t K = window_first(window, w.adapt, kmax);
    WindowCalls wc;
    uint32_t pos = 0;
    while (pos < n_tiles) {
        const uint32_t k = K < n_tiles - pos ? K : n_tiles - pos;
        const uint32_t nc = window_build(wc, first_tile + pos, k, c->od_L, [&](uint32_t tile) { return (uint32_t)c->od_level[tile]; });
        HIPCHK(hipMemcpyAsync(w.ltiles, wc.units.data(), sizeof(uint16_t) * nc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(w.llevels, wc.opts.data(), nc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(t.calls, wc.calls.data(), sizeof(snes::TileCall) * k, hipMemcpyHostToDevice, c->stream));
        CHECK(level_score_group(c, nc, base_map, t.errs));
        snes::LevelCommitParams P{};
        P.errs = t.errs; P.calls = t.calls; P.ncalls = (int)k; P.llevels = w.llevels; P.lmaps = t.lmaps; P.npx = (int)c->npx;
        P.level = c->d_level; P.map = c->d_map; P.inc_err = c->d_inc_err; P.log = reinterpret_cast<snes::TileLog *>(t.result + 16); P.res = reinterpret_cast<snes::TileWinRes *>(t.result);
        P.orig = c->d_orig; P.lab_eotf = c->d_lab_eotf; P.n = (int)c->od_n; P.W = (int)c->W; P.H = (int)c->H;
        P.target = c->d_target_own; P.labpx = c->perceptual ? c->d_labpx_t_own : nullptr; P.labpxT = c->perceptual ? c->d_labpxT_t_own : nullptr;
        hipLaunchKernelGGL(k_level_commit, dim3(1), dim3(1024), 0, c->stream, P, level_bank(c));
        WindowOutcome o{};
        CHECK(window_read_record(c->stream, t.result, wc.res, k, nc, m, 1, "level window", log ? log + pos : nullptr, S, o));
        if (o.accepted >= 0) { // as snesimage_set_tile_levels + snesimage_optimize would leave it, with the incumbent error known
            c->od_level[first_tile + pos + (uint32_t)o.accepted] = o.opt;
            c->pack_valid = false; c->sp.plist_valid = false; c->sp.counters_cleared = false; c->epoch++; c->epoch_by_commit = false;
            c->map_synced = true; c->map_pending = false; c->inc_valid = true; c->best_valid = false;
            // (the workspace's planes stay: with maps handed in the scorer takes the transparency marker from them and nothing else, and T.a == orig.a)
            if (c->win)
                for (auto &set : c->win->child)
                    for (snesimage_ctx *kc : set) { kc->pack_valid = false; kc->sp.plist_valid = false; kc->sp.counters_cleared = false; }
            base_map = c->d_map;
        }
        pos += o.used;
        K = window_next(window, K, w.policy, w.adapt, o, kmax, k, 0.2 * (double)m);
    }
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_set_ordered_dither_bank(snesimage_ctx *c, const int8_t *tables, uint32_t n, uint32_t L, uint32_t start_level) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (L == 0 || n == 0) return snesimage_set_ordered_dither(c, nullptr, 0);
    if (n != 2 && n != 4 && n != 8 && n != 16) return fail(SNES_ERR_ARG, "an ordered-dither table is 2, 4, 8 or 16 offsets wide (0 switches it off)");
    if (L > 8) return fail(SNES_ERR_ARG, "an ordered-dither bank holds at most 8 tables");
    if (!tables) return fail(SNES_ERR_ARG, "null bank");
    if (start_level >= L) return fail(SNES_ERR_ARG, "the start level is not a table of the bank");
    CHECK(level_setter_check(c));
    int8_t bank[8 * 256] = {};
    for (uint32_t l = 0; l < L; l++) memcpy(bank + 256 * l, tables + (size_t)l * n * n, (size_t)n * n);
    uint8_t level[1024] = {}; // (the rows of tiles below the image stay 0, as in tile_palettes)
    memset(level, (int)start_level, (size_t)(c->W / 8) * (c->H / 8));
    return level_rebuild(c, bank, n, L, level);
}

int32_t snesimage_get_ordered_dither_bank(snesimage_ctx *c, int8_t *tables, uint32_t *n, uint32_t *L) {
    if (!c || !tables || !n || !L) return fail(SNES_ERR_ARG, "null pointer");
    memcpy(tables, c->od_bank, sizeof c->od_bank); // (zeros behind each table's n * n offsets and behind the L tables)
    *n = c->od_n; *L = c->od_L;
    return SNES_OK;
}

int32_t snesimage_get_tile_levels(snesimage_ctx *c, uint8_t *out) {
    if (!c || !out) return fail(SNES_ERR_ARG, "null pointer");
    memcpy(out, c->od_level, sizeof c->od_level);
    return SNES_OK;
}

int32_t snesimage_set_tile_levels(snesimage_ctx *c, const uint8_t *in) {
    if (!c || !in) return fail(SNES_ERR_ARG, "null pointer");
    if (c->od_L == 0) return fail(SNES_ERR_STATE, "no ordered-dither bank is set: call snesimage_set_ordered_dither_bank first");
    CHECK(level_setter_check(c));
    const uint32_t ntile = (c->W / 8) * (c->H / 8);
    uint8_t level[1024] = {};
    for (uint32_t t = 0; t < ntile; t++) {
        if (in[t] >= c->od_L) return fail(SNES_ERR_ARG, "tile level beyond the bank");
        level[t] = in[t];
    }
    int8_t bank[8 * 256];
    memcpy(bank, c->od_bank, sizeof bank);
    return level_rebuild(c, bank, c->od_n, c->od_L, level);
}

int32_t snesimage_score_tile_levels(snesimage_ctx *c, const uint16_t *tiles, const uint8_t *levels, uint32_t n, double *errors, uint8_t *maps_out) {
    CHECK(level_check(c));
    if (!tiles || !levels || !errors) return fail(SNES_ERR_ARG, "null pointer");
    if (n == 0) return SNES_OK;
    const uint32_t ntile = (c->W / 8) * (c->H / 8);
    for (uint32_t j = 0; j < n; j++) {
        if (tiles[j] >= ntile) return fail(SNES_ERR_ARG, "tile beyond the image");
        if (levels[j] >= c->od_L) return fail(SNES_ERR_ARG, "tile level beyond the bank");
    }
    CHECK(set_device(c));
    const uint32_t group = n < tile_group(c) ? n : tile_group(c);
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, group, &base_map));
    CHECK(level_alloc(c, group));
    return score_pair_groups(c, tiles, levels, n, group, c->lvl->ltiles, c->lvl->llevels, errors, maps_out, [&](uint32_t nc) { return level_score_group(c, nc, base_map, c->tile->errs); });
}

int32_t snesimage_level_sweep(snesimage_ctx *c, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats *stats) {
    CHECK(level_check(c));
    snesimage_run_stats S{};
    const int32_t rc = level_sweep_impl(c, first_tile, n_tiles, window, log, S);
    if (stats) *stats = S; // (a window that fails leaves the accepted calls standing and counted)
    return rc;
}

int32_t snesimage_level_step(snesimage_ctx *c, uint32_t tile, snesimage_tile_result *out) {
    snesimage_tile_result r{};
    CHECK(snesimage_level_sweep(c, tile, 1, 1, &r, nullptr));
    if (out) *out = r;
    return SNES_OK;
}

} // extern "C"
