// snesimage_amd/csrc/tile_host.inc — tile moves decided by the objective: snesimage_score_tile_moves, snesimage_tile_step,
// snesimage_tile_sweep, snesimage_shared_tile_sweep (definition: include/snesimage_hip.h; kernels: kernels_tile.hpp).  The block
// moves (block_host.inc) run through the same code with the context's BlockGeom handed in: a tile is a 1 x 1 block.  The steps
// of a window loop and of a scored list are plain functions here, which the level moves share (level_host.inc,
// shared_level_host.inc).
//
// Every (tile, subpalette) candidate gets its own palette_map and the batch goes through the map-reading scorer of the
// --dither path (score_stages with use_maps), fed with maps that hold full colour indices and a tile table of zeros.
// The workspace below is the feature's own — the context's pack, planes and lane storage are never touched — so a scoring
// call leaves the context as it found it, and a failed allocation has nothing to undo.
// A window of a sweep is one such batch over the candidates of the coming K calls plus k_move_commit; unlike the slot
// windows, whose calls need a base image each, all tile calls of a window share the image as it stands.
// Included by capi.hip last (it uses shared_enter / shared_settle and WindowPolicy).

struct snesimage_tilework {
    uint32_t cap = 0;          // candidates the arrays hold
    bool planes_ready = false; // pack (transparency marker) and the all-zero subpalette planes: they depend on the image alone
    float *work = nullptr, *cand_tab = nullptr; double *part = nullptr, *errs = nullptr;
    uint8_t *zero_rgb5 = nullptr, *zero_tile = nullptr, *lmaps = nullptr, *maps = nullptr, *mapsT = nullptr, *mapsC4 = nullptr, *mapsR4 = nullptr, *tabs = nullptr, *basemap = nullptr;
    uint8_t *sub0C4 = nullptr, *sub0R4 = nullptr, *subs = nullptr; uint16_t *tiles = nullptr;
    unsigned long long *pack = nullptr, *packT = nullptr, *packC4 = nullptr, *packR4 = nullptr;
    snes::TileCall *calls = nullptr; unsigned char *result = nullptr; // result: TileWinRes (16 bytes), then cap TileLog records
    WindowPolicy policy; uint32_t adapt = 8;
};

namespace {

constexpr uint32_t kTileGroup = 512; // most candidates per launch group (3.7 MB of planes each at 256 x 256)
static_assert(sizeof(snes::TileLog) == sizeof(snesimage_tile_result) && sizeof(snes::TileLog) == 16, "the log records are copied out as they are");

void tile_release(snesimage_tilework *t) {
    dfree(t->work); dfree(t->cand_tab); dfree(t->part); dfree(t->errs); dfree(t->zero_rgb5); dfree(t->zero_tile); dfree(t->lmaps); dfree(t->maps); dfree(t->mapsT); dfree(t->mapsC4);
    dfree(t->mapsR4); dfree(t->tabs); dfree(t->basemap); dfree(t->sub0C4); dfree(t->sub0R4); dfree(t->subs); dfree(t->tiles); dfree(t->pack); dfree(t->packT); dfree(t->packC4); dfree(t->packR4);
    dfree(t->calls); dfree(t->result);
    t->cap = 0; t->planes_ready = false;
}
void tile_free(snesimage_ctx *c) { if (c->tile) { tile_release(c->tile); delete c->tile; c->tile = nullptr; } }

uint32_t tile_group(const snesimage_ctx *c) { // candidates per launch group: the context's chunk, at most kTileGroup, at least one tile call
    uint32_t g = c->chunk < kTileGroup ? c->chunk : kTileGroup;
    if (g < c->sub_count) g = c->sub_count;
    return g;
}

// grow-only; a failed grow releases everything (the context itself holds nothing of this)
int32_t tile_alloc(snesimage_ctx *c, uint32_t need) {
    if (!c->tile) c->tile = new snesimage_tilework();
    snesimage_tilework &t = *c->tile;
    if (t.cap >= need) return SNES_OK;
    if (need < 16) need = 16;
    HIPCHK(hipStreamSynchronize(c->stream));
    tile_release(&t);
    const size_t npx = c->npx;
    auto body = [&]() -> int32_t {
        HIPCHK(dmalloc(&t.work, sizeof(float) * (size_t)c->G.cand_stride * need));
        HIPCHK(dmalloc(&t.cand_tab, sizeof(float) * 8 * (size_t)need));
        HIPCHK(dmalloc(&t.part, sizeof(double) * (size_t)need * kMaxScales * 18));
        HIPCHK(dmalloc(&t.errs, sizeof(double) * need));
        HIPCHK(dmalloc(&t.zero_rgb5, 3 * (size_t)need));
        HIPCHK(dmalloc(&t.zero_tile, 1024));
        HIPCHK(dmalloc(&t.lmaps, npx * need)); HIPCHK(dmalloc(&t.maps, npx * need)); HIPCHK(dmalloc(&t.mapsT, npx * need)); HIPCHK(dmalloc(&t.mapsC4, npx * need)); HIPCHK(dmalloc(&t.mapsR4, npx * need));
        if (c->dither) HIPCHK(dmalloc(&t.tabs, 1024 * (size_t)need));
        HIPCHK(dmalloc(&t.basemap, npx));
        HIPCHK(dmalloc(&t.sub0C4, npx)); HIPCHK(dmalloc(&t.sub0R4, npx));
        HIPCHK(dmalloc(&t.subs, need)); HIPCHK(dmalloc(&t.tiles, sizeof(uint16_t) * need));
        HIPCHK(dmalloc(&t.pack, npx * 8)); HIPCHK(dmalloc(&t.packT, npx * 8)); HIPCHK(dmalloc(&t.packC4, npx * 8)); HIPCHK(dmalloc(&t.packR4, npx * 8));
        HIPCHK(dmalloc(&t.calls, sizeof(snes::TileCall) * need));
        HIPCHK(dmalloc(&t.result, 16 + sizeof(snes::TileLog) * (size_t)need));
        HIPCHK(hipMemsetAsync(t.zero_rgb5, 0, 3 * (size_t)need, c->stream));
        HIPCHK(hipMemsetAsync(t.zero_tile, 0, 1024, c->stream));
        if (g_poison_alloc.load()) { // whatever the scorer reads must have been written by this batch's own kernels
            HIPCHK(hipMemsetAsync(t.work, 0xff, sizeof(float) * (size_t)c->G.cand_stride * need, c->stream));
            HIPCHK(hipMemsetAsync(t.part, 0xff, sizeof(double) * (size_t)need * kMaxScales * 18, c->stream));
            HIPCHK(hipMemsetAsync(t.errs, 0xff, sizeof(double) * need, c->stream));
            HIPCHK(hipMemsetAsync(t.lmaps, 0xff, npx * need, c->stream)); HIPCHK(hipMemsetAsync(t.maps, 0xff, npx * need, c->stream));
            HIPCHK(hipMemsetAsync(t.mapsT, 0xff, npx * need, c->stream)); HIPCHK(hipMemsetAsync(t.mapsC4, 0xff, npx * need, c->stream)); HIPCHK(hipMemsetAsync(t.mapsR4, 0xff, npx * need, c->stream));
        }
        return SNES_OK;
    };
    const int32_t rc = body();
    if (rc != SNES_OK) { tile_release(&t); return rc; }
    t.cap = need;
    return SNES_OK;
}

// What every tile entry point needs first.  *base_map: the optimize() of the state as it stands, which the candidates of a
// context without --dither start from — the stored map, or one made here if the stored map does not belong to the palette.
// stored_base: the candidates start from the stored map whatever it belongs to (the character merges, char_host.inc).
int32_t tile_prepare(snesimage_ctx *c, uint32_t need, const uint8_t **base_map, bool stored_base = false) {
    CHECK(ensure_map(c)); // an optimize() still owed belongs to the state the candidates are compared with
    CHECK(ensure_tables(c));
    CHECK(ensure_source(c));
    CHECK(ensure_incumbent(c));
    CHECK(tile_alloc(c, need));
    snesimage_tilework &t = *c->tile;
    PrepParams P{};
    P.orig = c->d_target; P.pal_rgb8 = c->d_pal_rgb8; P.pack = t.pack; P.packT = t.packT; P.packC4 = t.packC4; P.packR4 = t.packR4;
    P.W = (int)c->W; P.H = (int)c->H; P.sub_size = (int)c->sub_size; P.ncol = c->ncol; P.sp = -1; P.si = -1;
    const dim3 grid((unsigned)((c->npx + 255) / 256));
    if (!t.planes_ready) { // mode 1 over a tile table of zeros: the pack's transparency marker, and subpalette planes of 0 (255 = transparent)
        P.tile_pal = t.zero_tile; P.map = c->d_map; P.mode = 1; P.subC4 = t.sub0C4; P.subR4 = t.sub0R4;
        hipLaunchKernelGGL(k_prep, grid, dim3(256), 0, c->stream, P);
        t.planes_ready = true;
    }
    *base_map = c->d_map;
    if (!c->dither && !c->map_synced && !stored_base) { // (mode 0 leaves the same transparency marker in the pack)
        P.tile_pal = c->d_tile_pal; P.map = t.basemap; P.mode = 0; P.subC4 = nullptr; P.subR4 = nullptr;
        P.labpx = c->d_labpx_t; P.pal_lab = c->d_pal_lab; P.perceptual = c->perceptual ? 1 : 0;
        hipLaunchKernelGGL(k_prep, grid, dim3(256), 0, c->stream, P);
        *base_map = t.basemap;
    }
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

// The two ends of a launch group, shared with the character merges: the candidates' colour tables in front of whatever
// writes their maps into t.lmaps (and their pairs into t.tiles / t.subs), the scorer behind it.
void tile_score_head(snesimage_ctx *c, uint32_t nc) {
    snesimage_tilework &t = *c->tile;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_candidate_tables, dim3((nc + 63) / 64), dim3(64), 0, st, t.zero_rgb5, (int)nc, c->d_eotf, t.cand_tab);
    hipLaunchKernelGGL(k_candidate_slot, dim3((nc + 63) / 64), dim3(64), 0, st, t.cand_tab, (int)nc, 0xffffffffu); // no colour index is "the candidate's"
}
// g: the blocks that the pairs at t.tiles / t.subs name — tile_geom for (tile, subpalette) pairs
int32_t tile_score_tail(snesimage_ctx *c, uint32_t nc, double *d_errors, const BlockGeom &g) {
    snesimage_tilework &t = *c->tile;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_move_full, dim3((unsigned)((c->npx / 4 + 255) / 256), nc), dim3(256), 0, st, (const uint8_t *)t.lmaps, (const uint8_t *)c->d_tile_pal, (const uint16_t *)t.tiles,
                       (const uint8_t *)t.subs, (int)c->W, (int)c->H, (int)c->sub_size, g.lbw, g.lbh, t.maps, t.mapsC4);
    const bool fast0 = (c->fast_mask & 1) != 0;
    hipLaunchKernelGGL(k_maps_relayout, dim3((unsigned)(c->H / 4), nc), dim3(256), 0, st, (const uint8_t *)t.maps, (int)c->W, (int)c->H, reinterpret_cast<uint32_t *>(t.mapsR4),
                       fast0 ? (uint32_t *)nullptr : reinterpret_cast<uint32_t *>(t.mapsT));
    // the scorer's own stages, on this workspace: full-index maps, a tile table and subpalette planes of zeros
    DenseView V{t.pack, t.packT, t.packC4, t.packR4, t.sub0C4, t.sub0R4, t.zero_tile, t.work, t.cand_tab, nullptr, t.part, t.maps, t.mapsT, t.mapsC4, t.mapsR4, true, false};
    CHECK(score_stages(c, V, nc, d_errors, 1, 0, nullptr));
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

// The candidates' Floyd-Steinberg runs, each under its own tile table (t.tabs, written by the caller): maps into t.lmaps
void tile_dither_launch(snesimage_ctx *c, uint32_t nc) {
    snesimage_tilework &t = *c->tile;
    hipStream_t st = c->stream;
    DitherParams Dp{};
    Dp.orig = c->d_orig; Dp.tile_pal = c->d_tile_pal; Dp.pal_rgb8 = c->d_pal_rgb8; Dp.pal_lab = c->d_pal_lab; Dp.cand_tab = t.cand_tab; Dp.cand_lab = nullptr;
    Dp.lab_eotf = c->d_lab_eotf; Dp.maps = t.lmaps; Dp.mapsC4 = nullptr;
    Dp.W = (int)c->W; Dp.H = (int)c->H; Dp.sub_size = (int)c->sub_size; Dp.ncol = c->ncol; Dp.slot_ci = 0xffffffffu; Dp.perceptual = c->perceptual ? 1 : 0;
    const bool quad = c->dither4 && nc <= c->dither4_max; // as launch_dither: a quad of lanes per row while the runs are few
    if (c->perceptual && quad) hipLaunchKernelGGL((k_dither4_tile<0, true>), dim3(nc), dim3(512), 0, st, Dp, (const uint8_t *)t.tabs);
    else if (c->perceptual) hipLaunchKernelGGL((k_dither_tile<true, 0>), dim3(nc), dim3(128), 0, st, Dp, (const uint8_t *)t.tabs);
    else if (quad && c->sub_size == 15) hipLaunchKernelGGL((k_dither4_tile<15, false>), dim3(nc), dim3(512), 0, st, Dp, (const uint8_t *)t.tabs);
    else if (quad && c->sub_size == 16) hipLaunchKernelGGL((k_dither4_tile<16, false>), dim3(nc), dim3(512), 0, st, Dp, (const uint8_t *)t.tabs);
    else if (quad) hipLaunchKernelGGL((k_dither4_tile<0, false>), dim3(nc), dim3(512), 0, st, Dp, (const uint8_t *)t.tabs);
    else if (c->sub_size == 15) hipLaunchKernelGGL((k_dither_tile<false, 15>), dim3(nc), dim3(128), 0, st, Dp, (const uint8_t *)t.tabs);
    else if (c->sub_size == 16) hipLaunchKernelGGL((k_dither_tile<false, 16>), dim3(nc), dim3(128), 0, st, Dp, (const uint8_t *)t.tabs);
    else hipLaunchKernelGGL((k_dither_tile<false, 0>), dim3(nc), dim3(128), 0, st, Dp, (const uint8_t *)t.tabs);
}

// nc move candidates, (block, subpalette) pairs of g's blocks at t.tiles / t.subs [0, nc): maps into t.lmaps, errors into d_errors[0, nc)
int32_t tile_score_group(snesimage_ctx *c, uint32_t nc, const uint8_t *base_map, double *d_errors, const BlockGeom &g) {
    snesimage_tilework &t = *c->tile;
    hipStream_t st = c->stream;
    tile_score_head(c, nc);
    if (c->dither) {
        hipLaunchKernelGGL(k_move_tabs, dim3(nc), dim3(256), 0, st, (const uint8_t *)c->d_tile_pal, (const uint16_t *)t.tiles, (const uint8_t *)t.subs, g.lbw, g.lbh, t.tabs);
        tile_dither_launch(c, nc);
    } else {
        MoveRemapParams R{};
        R.orig = c->d_target; R.base_map = base_map; R.pal_rgb8 = c->d_pal_rgb8; R.pal_lab = c->d_pal_lab; R.labpx = c->d_labpx_t;
        R.blocks = t.tiles; R.subs = t.subs; R.lmaps = t.lmaps; R.W = (int)c->W; R.H = (int)c->H; R.sub_size = (int)c->sub_size; R.perceptual = c->perceptual ? 1 : 0; R.lbw = g.lbw; R.lbh = g.lbh;
        hipLaunchKernelGGL(k_move_remap, dim3(nc), dim3(256), 0, st, R);
    }
    return tile_score_tail(c, nc, d_errors, g);
}

const char *kTileOnBlocks = "the context holds palette blocks (snesimage_set_palette_blocks): a single-tile move would leave a block with two subpalettes; use ";

int32_t tile_check(snesimage_ctx *c) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first (its candidates were scored for the current tile assignment)");
    return SNES_OK;
}

// ---- the common steps of a window loop: tile_sweep_impl, level_sweep_impl (level_host.inc), sl_tied_sweep (shared_level_host.inc) ----
// A sweep walks units (tiles or blocks), one call each: the unit's other options (subpalettes or levels), ascending, against the
// incumbent.  A window is the candidates of the coming k calls scored in one batch, one commit kernel (window_decide of
// kernels_tile.hpp) and one synchronisation; every call up to the first that accepts takes effect.

// most calls of a window: a launch group of `group` candidates at m per call, the units of the sweep, the caller's `window`
uint32_t window_limit(uint32_t group, uint32_t m, uint32_t n_units, uint32_t window) {
    uint32_t kmax = m ? group / m : n_units;
    if (kmax < 1) kmax = 1;
    if (kmax > n_units) kmax = n_units;
    if (window == 1) kmax = 1; else if (window > 1 && window < kmax) kmax = window;
    return kmax;
}
// calls of the first window: all of them, or (window == 0, the policy decides) what the last sweep settled on
uint32_t window_first(uint32_t window, uint32_t adapt, uint32_t kmax) {
    const uint32_t K = window == 0 ? (adapt < kmax ? adapt : kmax) : kmax;
    return K < 1 ? 1 : K;
}
struct WindowCalls { // one window on the host: the calls, their candidates as (unit, option) pairs, the commit record as copied back
    std::vector<uint16_t> units; std::vector<uint8_t> opts; std::vector<snes::TileCall> calls; std::vector<unsigned char> res;
};
// the calls of units [first, first + k), each with the nopt - 1 options other than cur_of(unit); the number of candidates
template <class Cur>
uint32_t window_build(WindowCalls &w, uint32_t first, uint32_t k, uint32_t nopt, Cur cur_of) {
    w.units.clear(); w.opts.clear(); w.calls.clear();
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t unit = first + i, cur = cur_of(unit);
        w.calls.push_back(snes::TileCall{unit, (uint32_t)w.units.size(), nopt - 1, cur});
        for (uint32_t o = 0; o < nopt; o++) if (o != cur) { w.units.push_back((uint16_t)unit); w.opts.push_back((uint8_t)o); }
    }
    return (uint32_t)w.units.size();
}
// no other option: no candidates, nothing accepted — every call logs the incumbent error
void window_idle(uint32_t n_units, double inc, snesimage_tile_result *log, snesimage_run_stats &S) {
    if (log) for (uint32_t i = 0; i < n_units; i++) { log[i].error = inc; log[i].sub = 0; log[i].changed = 0; }
    S.calls = n_units;
}
int32_t window_idle_ctx(snesimage_ctx *c, uint32_t n_units, snesimage_tile_result *log, snesimage_run_stats &S) { // ... of one image: its own incumbent
    double inc = 0.0;
    HIPCHK(hipMemcpyAsync(&inc, c->d_inc_err, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    window_idle(n_units, inc, log, S);
    return SNES_OK;
}
struct WindowOutcome { uint32_t used; int32_t accepted; uint8_t opt; }; // calls that took effect; the one that accepted (-1: none) and the option it took
// Behind the commit kernel of a window of k calls and nc candidates: the record (TileWinRes in 16 bytes, then the TileLog
// records) copied back — the one synchronisation of the window — validated, logged at log_at and counted.  m: candidates per
// call; F: images that scored each; name: "tile window", "block window", ... for the error text; buf: the host copy, kept by the
// caller from window to window.  (The slot windows' window_collect of window_host.inc reads another record: WindowResult.)
int32_t window_read_record(hipStream_t st, const unsigned char *d_result, std::vector<unsigned char> &buf, uint32_t k, uint32_t nc, uint32_t m, uint32_t F, const char *name,
                           snesimage_tile_result *log_at, snesimage_run_stats &S, WindowOutcome &out) {
    HIPCHK(hipGetLastError());
    buf.resize(16 + sizeof(snes::TileLog) * (size_t)k);
    HIPCHK(hipMemcpyAsync(buf.data(), d_result, buf.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    snes::TileWinRes res; memcpy(&res, buf.data(), sizeof(res));
    const uint32_t used = (uint32_t)res.consumed;
    if (used < 1 || used > k || res.accepted >= (int32_t)used) return fail(SNES_ERR_HIP, std::string(name) + ": bad commit record");
    const snes::TileLog *recs = reinterpret_cast<const snes::TileLog *>(buf.data() + 16);
    if (log_at) memcpy(log_at, recs, sizeof(snes::TileLog) * used);
    S.calls += used; S.windows += 1; S.scored += (uint64_t)nc * F; S.useful += (uint64_t)used * m * F;
    if (res.accepted >= 0) S.accepted += 1;
    out = WindowOutcome{used, res.accepted, res.accepted >= 0 ? (uint8_t)recs[res.accepted].sub : (uint8_t)0};
    return SNES_OK;
}
// calls of the next window: K as it is, or (window == 0) the policy's step from this window of k calls, within [1, kmax], kept in `adapt`
uint32_t window_next(uint32_t window, uint32_t K, WindowPolicy &policy, uint32_t &adapt, const WindowOutcome &o, uint32_t kmax, uint32_t k, double weight) {
    if (window != 0) return K;
    K = policy.next(o.used, o.accepted >= 0 ? 1u : 0u, kmax < 2 ? kmax : 2u, kmax, 1, k, weight);
    if (K > kmax) K = kmax;
    if (K < 1) K = 1;
    adapt = K;
    return K;
}

// n (unit, option) pairs in launch groups of `group`: each group's pairs uploaded to d_units / d_opts, scored by score(nc) —
// maps into t.lmaps, errors into t.errs — and copied out
template <class Score>
int32_t score_pair_groups(snesimage_ctx *c, const uint16_t *units, const uint8_t *opts, uint32_t n, uint32_t group, uint16_t *d_units, uint8_t *d_opts, double *errors, uint8_t *maps_out, Score score) {
    snesimage_tilework &t = *c->tile;
    for (uint32_t c0 = 0; c0 < n; c0 += group) {
        const uint32_t nc = n - c0 < group ? n - c0 : group;
        HIPCHK(hipMemcpyAsync(d_units, units + c0, sizeof(uint16_t) * nc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_opts, opts + c0, nc, hipMemcpyHostToDevice, c->stream));
        CHECK(score(nc));
        HIPCHK(hipMemcpyAsync(errors + c0, t.errs, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
        if (maps_out) HIPCHK(hipMemcpyAsync(maps_out + (size_t)c0 * c->npx, t.lmaps, c->npx * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

// snesimage_score_tile_moves and snesimage_score_block_moves: g's blocks, called `noun` in the error texts
int32_t move_score_list(snesimage_ctx *c, const uint16_t *blocks, const uint8_t *subs, uint32_t n, double *errors, uint8_t *maps_out, const BlockGeom &g, const char *noun) {
    if (!blocks || !subs || !errors) return fail(SNES_ERR_ARG, "null pointer");
    if (n == 0) return SNES_OK;
    for (uint32_t j = 0; j < n; j++) {
        if (blocks[j] >= g.nblock) return fail(SNES_ERR_ARG, std::string(noun) + " beyond the image");
        if (subs[j] >= c->sub_count) return fail(SNES_ERR_ARG, "subpalette out of range");
    }
    CHECK(set_device(c));
    const uint32_t group = n < tile_group(c) ? n : tile_group(c);
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, group, &base_map));
    snesimage_tilework &t = *c->tile;
    return score_pair_groups(c, blocks, subs, n, group, t.tiles, t.subs, errors, maps_out, [&](uint32_t nc) { return tile_score_group(c, nc, base_map, t.errs, g); });
}

// A sweep over g's blocks, called `noun` in the error texts: the calls walk blocks, a candidate moves every tile of its block and
// k_move_commit writes the accepted block's table entries.  The tile sweeps hand in tile_geom: a block is a tile.
int32_t tile_sweep_impl(snesimage_ctx *c, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats *stats, const BlockGeom &g, const char *noun) {
    CHECK(tile_check(c));
    if (first_tile > g.nblock || n_tiles > g.nblock - first_tile) return fail(SNES_ERR_ARG, std::string(noun) + " range beyond the image");
    CHECK(set_device(c));
    snesimage_run_stats S{};
    if (n_tiles == 0) { if (stats) *stats = S; return SNES_OK; }
    const uint32_t m = c->sub_count - 1; // candidates per call
    const uint32_t kmax = window_limit(tile_group(c), m, n_tiles, window);
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, (kmax * m > 0 ? kmax * m : 1), &base_map));
    snesimage_tilework &t = *c->tile;
    std::vector<uint8_t> tp(1024);
    HIPCHK(hipMemcpyAsync(tp.data(), c->d_tile_pal, 1024, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (m == 0) { // one subpalette
        CHECK(window_idle_ctx(c, n_tiles, log, S));
        if (stats) *stats = S;
        return SNES_OK;
    }
    const std::string name = std::string(noun) + " window";
    uint32_t K = window_first(window, t.adapt, kmax);
    WindowCalls w;
    uint32_t pos = 0;
    while (pos < n_tiles) {
        const uint32_t k = K < n_tiles - pos ? K : n_tiles - pos;
        const uint32_t nc = window_build(w, first_tile + pos, k, c->sub_count, [&](uint32_t b) { return (uint32_t)tp[block_first_tile(g, b)]; });
        HIPCHK(hipMemcpyAsync(t.tiles, w.units.data(), sizeof(uint16_t) * nc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(t.subs, w.opts.data(), nc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(t.calls, w.calls.data(), sizeof(snes::TileCall) * k, hipMemcpyHostToDevice, c->stream));
        CHECK(tile_score_group(c, nc, base_map, t.errs, g));
        hipLaunchKernelGGL(k_move_commit, dim3(1), dim3(1024), 0, c->stream, (const double *)t.errs, (const snes::TileCall *)t.calls, (int)k, (const uint8_t *)t.subs, (const uint8_t *)t.lmaps,
                           (int)c->npx, g.lbw, g.lbh, c->d_tile_pal, c->d_map, c->d_inc_err, reinterpret_cast<snes::TileLog *>(t.result + 16), reinterpret_cast<snes::TileWinRes *>(t.result));
        WindowOutcome o{};
        CHECK(window_read_record(c->stream, t.result, w.res, k, nc, m, 1, name.c_str(), log ? log + pos : nullptr, S, o));
        if (o.accepted >= 0) { // as snesimage_set_tile_palettes + snesimage_optimize would leave it, with the incumbent error known
            block_fill(g, tp.data(), first_tile + pos + (uint32_t)o.accepted, o.opt);
            c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
            c->map_synced = true; c->map_pending = false; c->inc_valid = true; c->best_valid = false;
            base_map = c->d_map;
        }
        pos += o.used;
        K = window_next(window, K, t.policy, t.adapt, o, kmax, k, 0.2 * (double)m);
    }
    if (stats) *stats = S;
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_score_tile_moves(snesimage_ctx *c, const uint16_t *tiles, const uint8_t *subs, uint32_t n, double *errors, uint8_t *maps_out) {
    CHECK(tile_check(c));
    if (blocked(c)) return fail(SNES_ERR_UNSUPPORTED, kTileOnBlocks + std::string("snesimage_score_block_moves"));
    return move_score_list(c, tiles, subs, n, errors, maps_out, tile_geom(c), "tile");
}

int32_t snesimage_tile_step(snesimage_ctx *c, uint32_t tile, snesimage_tile_result *out) {
    snesimage_tile_result r{};
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (blocked(c)) return fail(SNES_ERR_UNSUPPORTED, kTileOnBlocks + std::string("snesimage_block_step"));
    CHECK(tile_sweep_impl(c, tile, 1, 1, &r, nullptr, tile_geom(c), "tile"));
    if (out) *out = r;
    return SNES_OK;
}

int32_t snesimage_tile_sweep(snesimage_ctx *c, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats *stats) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (blocked(c)) return fail(SNES_ERR_UNSUPPORTED, kTileOnBlocks + std::string("snesimage_block_sweep"));
    return tile_sweep_impl(c, first_tile, n_tiles, window, log, stats, tile_geom(c), "tile");
}

// Per member, as snesimage_shared_reassign_tiles: a tile move in member i changes e_i alone.
int32_t snesimage_shared_tile_sweep(snesimage_shared *s, uint32_t first_tile, uint32_t n_tiles, uint32_t window, snesimage_tile_result *log, snesimage_run_stats *stats) {
    CHECK(shared_enter(s));
    snesimage_run_stats T{};
    size_t i = 0;
    for (auto *c : members(s)) {
        snesimage_run_stats S{};
        CHECK(tile_sweep_impl(c, first_tile, n_tiles, window, log ? log + i * n_tiles : nullptr, &S, tile_geom(c), "tile"));
        T.calls += S.calls; T.accepted += S.accepted; T.windows += S.windows; T.scored += S.scored; T.useful += S.useful;
        i++;
    }
    if (stats) *stats = T;
    return shared_settle(s);
}

} // extern "C"
