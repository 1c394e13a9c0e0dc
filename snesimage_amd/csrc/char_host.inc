// snesimage_amd/csrc/char_host.inc — the character budget: snesimage_characters, snesimage_merge_shortlist,
// snesimage_score_merges, snesimage_reduce_characters, snesimage_as_tilemap_json, and the refit of shared characters:
// snesimage_character_fits, snesimage_score_refits, snesimage_refit_characters (definition: include/snesimage_hip.h;
// kernels: kernels_char.hpp).
//
// Characters, classes and the proxy shortlist are recomputed from the stored map whenever they are asked for (five small
// launches over at most 1,024 tiles); nothing of them is cached in the context, so no other entry point has anything to
// invalidate.  The shortlisted merges are scored as the tile moves are: k_merge_maps writes each candidate's palette_map into
// the tile workspace's lmaps with (tiles[j], subs[j]) = (t, tile_palettes[t]), and tile_score_tail runs the map-reading scorer
// on them unchanged.  The base of every candidate is the stored map as it is (tile_prepare with stored_base): after the
// first merge the map is no optimize() of anything.
// A reduction step enqueues scoring, k_merge_commit and the next step's characters and shortlist, then reads the record and
// the next shortlist's length back: one synchronisation per step.
// A refit sweep takes the classes and their fits once (k_refit_fit: they depend on the snapshot, the original and the palette,
// not on the map), then goes through the classes whose fit differs from their character in windows as a tile sweep does:
// k_refit_maps, the scorer, k_refit_commit, one synchronisation per window.
// Included by capi.hip behind tile_host.inc (it uses the tile workspace).

struct snesimage_charwork {
    bool ready = false;
    uint8_t *chars = nullptr, *pinned = nullptr, *flip = nullptr;
    uint16_t *rep = nullptr, *csize = nullptr;
    unsigned long long *part = nullptr, *keys = nullptr; // part: a list of kCharShort keys per tile; keys: the shortlist, or the pairs of a score_merges launch group (kTileGroup)
    snes::CharInfo *info = nullptr; snes::MergeLog *log = nullptr;
    // the refit: fits[r * 64 + q] and fit[r] of the class tile r represents; the window's classes; its result (RefitWinRes, 16 bytes, then kTileGroup records)
    uint8_t *fits = nullptr; snes::RefitFit *fit = nullptr; uint16_t *rcalls = nullptr; unsigned char *rresult = nullptr;
    WindowPolicy policy; uint32_t adapt = 4;
};

namespace {

static_assert(sizeof(snes::MergeLog) == sizeof(snesimage_merge_result) && sizeof(snes::MergeLog) == 24, "the log record is copied out as it is");
static_assert(sizeof(snes::RefitLog) == sizeof(snesimage_refit_result) && sizeof(snes::RefitLog) == 24, "the log record is copied out as it is");
static_assert(sizeof(snes::RefitFit) == 16 && sizeof(snes::RefitWinRes) <= 16, "the layout of the refit workspace");

void char_release(snesimage_charwork *w) {
    dfree(w->chars); dfree(w->pinned); dfree(w->flip); dfree(w->rep); dfree(w->csize); dfree(w->part); dfree(w->keys); dfree(w->info); dfree(w->log);
    dfree(w->fits); dfree(w->fit); dfree(w->rcalls); dfree(w->rresult);
    w->ready = false;
}
void char_free(snesimage_ctx *c) { if (c->chr) { char_release(c->chr); delete c->chr; c->chr = nullptr; } }

// all or nothing: a failed allocation releases everything (the context itself holds nothing of this)
int32_t char_alloc(snesimage_ctx *c) {
    if (!c->chr) c->chr = new snesimage_charwork();
    snesimage_charwork &w = *c->chr;
    if (w.ready) return SNES_OK;
    auto body = [&]() -> int32_t {
        HIPCHK(dmalloc(&w.chars, 1024 * 64)); HIPCHK(dmalloc(&w.pinned, 1024)); HIPCHK(dmalloc(&w.flip, 1024));
        HIPCHK(dmalloc(&w.rep, sizeof(uint16_t) * 1024)); HIPCHK(dmalloc(&w.csize, sizeof(uint16_t) * 1024));
        HIPCHK(dmalloc(&w.part, sizeof(unsigned long long) * 1024 * kCharShort)); HIPCHK(dmalloc(&w.keys, sizeof(unsigned long long) * kTileGroup));
        HIPCHK(dmalloc(&w.info, sizeof(snes::CharInfo))); HIPCHK(dmalloc(&w.log, sizeof(snes::MergeLog)));
        HIPCHK(dmalloc(&w.fits, 1024 * 64)); HIPCHK(dmalloc(&w.fit, sizeof(snes::RefitFit) * 1024)); HIPCHK(dmalloc(&w.rcalls, sizeof(uint16_t) * kTileGroup));
        HIPCHK(dmalloc(&w.rresult, 16 + sizeof(snes::RefitLog) * kTileGroup));
        if (g_poison_alloc.load()) { // whatever is read must have been written by the call's own kernels
            HIPCHK(hipMemsetAsync(w.chars, 0xff, 1024 * 64, c->stream)); HIPCHK(hipMemsetAsync(w.pinned, 0xff, 1024, c->stream)); HIPCHK(hipMemsetAsync(w.flip, 0xff, 1024, c->stream));
            HIPCHK(hipMemsetAsync(w.rep, 0xff, sizeof(uint16_t) * 1024, c->stream)); HIPCHK(hipMemsetAsync(w.csize, 0xff, sizeof(uint16_t) * 1024, c->stream));
            HIPCHK(hipMemsetAsync(w.part, 0x5a, sizeof(unsigned long long) * 1024 * kCharShort, c->stream)); HIPCHK(hipMemsetAsync(w.keys, 0x5a, sizeof(unsigned long long) * kTileGroup, c->stream));
            HIPCHK(hipMemsetAsync(w.fits, 0xff, 1024 * 64, c->stream)); HIPCHK(hipMemsetAsync(w.fit, 0xff, sizeof(snes::RefitFit) * 1024, c->stream));
            HIPCHK(hipMemsetAsync(w.rcalls, 0xff, sizeof(uint16_t) * kTileGroup, c->stream)); HIPCHK(hipMemsetAsync(w.rresult, 0xff, 16 + sizeof(snes::RefitLog) * kTileGroup, c->stream));
        }
        return SNES_OK;
    };
    const int32_t rc = body();
    if (rc != SNES_OK) { char_release(&w); return rc; }
    w.ready = true;
    return SNES_OK;
}

int32_t char_check(snesimage_ctx *c) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first (its candidates were scored for the current map)");
    if (c->owner || c->group) return fail(SNES_ERR_STATE, "the context is lent to a batch, a set or a group: the character budget works on a context of its own");
    return SNES_OK;
}

uint32_t char_ntile(const snesimage_ctx *c) { return 32u * (c->H / 8); }
int char_zero_at(const snesimage_ctx *c) { return c->backdrop ? (int)c->user_size : -1; }
// a tile with a transparent source pixel: never changed, never a donor
bool char_pinned(const snesimage_ctx *c, uint32_t t) {
    for (uint32_t p = 0; p < 64; p++)
        if (c->h_orig[4 * ((size_t)((t >> 5) * 8 + (p >> 3)) * c->W + (t & 31) * 8 + (p & 7)) + 3] == 0) return true;
    return false;
}

// characters, classes and U of the stored map (info->unique)
int32_t char_classes(snesimage_ctx *c) {
    snesimage_charwork &w = *c->chr;
    const uint32_t ntile = char_ntile(c);
    hipLaunchKernelGGL(k_char_build, dim3(ntile), dim3(64), 0, c->stream, (const uint8_t *)c->d_orig, (const uint8_t *)c->d_map, (int)c->W, char_zero_at(c), w.chars, w.pinned);
    hipLaunchKernelGGL(k_char_classes, dim3(ntile), dim3(256), 0, c->stream, (const uint8_t *)w.chars, w.rep, w.flip);
    hipLaunchKernelGGL(k_char_count, dim3(1), dim3(1024), 0, c->stream, (const uint16_t *)w.rep, (int)ntile, w.csize, w.info);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
// and the K lowest candidates of the proxy into w.keys (info->nshort of them)
int32_t char_shortlist(snesimage_ctx *c, uint32_t k) {
    CHECK(char_classes(c));
    snesimage_charwork &w = *c->chr;
    const uint32_t ntile = char_ntile(c);
    hipLaunchKernelGGL(k_merge_proxy, dim3(ntile), dim3(256), sizeof(uint32_t) * 64 * (size_t)c->sub_size, c->stream, (const uint8_t *)c->d_orig, (int)c->W, (const uint8_t *)w.chars,
                       (const uint8_t *)w.pinned, (const uint16_t *)w.rep, (const uint16_t *)w.csize, (const uint8_t *)c->d_tile_pal, (const uint32_t *)c->d_pal_rgb8, (int)c->sub_size,
                       char_zero_at(c), (int)ntile, (int)k, w.part);
    hipLaunchKernelGGL(k_merge_topk, dim3(1), dim3(1024), 0, c->stream, (const unsigned long long *)w.part, (int)ntile, (int)k, w.keys, w.info);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

// nc candidates at w.keys[0, nc): maps into the tile workspace's lmaps, errors into d_errors[0, nc)
int32_t char_score_group(snesimage_ctx *c, uint32_t nc, double *d_errors) {
    snesimage_tilework &t = *c->tile;
    tile_score_head(c, nc);
    hipLaunchKernelGGL(k_merge_maps, dim3(nc), dim3(256), 0, c->stream, (const unsigned long long *)c->chr->keys, (const uint8_t *)c->d_map, (const uint8_t *)c->d_tile_pal, (int)c->W, (int)c->npx,
                       t.lmaps, t.tiles, t.subs);
    return tile_score_tail(c, nc, d_errors, tile_geom(c));
}

int32_t char_shortlist_len(uint32_t *k) {
    if (*k > (uint32_t)kCharShort) return fail(SNES_ERR_ARG, "a shortlist holds at most 64 candidates");
    if (*k == 0) *k = 16;
    return SNES_OK;
}

// the snapshot and the fits of a sweep: classes of the stored map, then every eligible class's fit (w.fits, w.fit)
int32_t char_fits(snesimage_ctx *c) {
    CHECK(char_classes(c));
    snesimage_charwork &w = *c->chr;
    const uint32_t ntile = char_ntile(c);
    hipLaunchKernelGGL(k_refit_fit, dim3(ntile), dim3(256), 0, c->stream, (const uint8_t *)c->d_orig, (const uint8_t *)c->d_map, (int)c->W, (const uint8_t *)w.pinned, (const uint16_t *)w.rep,
                       (const uint8_t *)w.flip, (const uint16_t *)w.csize, (const uint8_t *)c->d_tile_pal, (const uint32_t *)c->d_pal_rgb8, (int)c->sub_size, c->ncol, (int)ntile, w.fits, w.fit);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
// ... read back: fit[ntile], and U of the snapshot
int32_t char_fits_read(snesimage_ctx *c, std::vector<snes::RefitFit> &fit, uint32_t *unique) {
    snesimage_charwork &w = *c->chr;
    snes::CharInfo info{};
    fit.resize(char_ntile(c));
    HIPCHK(hipMemcpyAsync(fit.data(), w.fit, sizeof(snes::RefitFit) * fit.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *unique = info.unique;
    return SNES_OK;
}

// nc refit candidates, classes at w.rcalls[0, nc): maps into the tile workspace's lmaps, errors into d_errors[0, nc)
int32_t refit_score_group(snesimage_ctx *c, uint32_t nc, double *d_errors) {
    snesimage_tilework &t = *c->tile;
    snesimage_charwork &w = *c->chr;
    tile_score_head(c, nc);
    hipLaunchKernelGGL(k_refit_maps, dim3(nc), dim3(256), 0, c->stream, (const uint16_t *)w.rcalls, (const uint8_t *)c->d_map, (const uint16_t *)w.rep, (const uint8_t *)w.flip, (const uint8_t *)w.fits,
                       (const uint8_t *)c->d_tile_pal, (int)c->W, (int)c->npx, t.lmaps, t.tiles, t.subs);
    return tile_score_tail(c, nc, d_errors, tile_geom(c));
}

} // namespace

extern "C" {

int32_t snesimage_characters(snesimage_ctx *c, uint32_t *unique, uint16_t *rep, uint8_t *flip, uint8_t *chars) {
    CHECK(char_check(c));
    CHECK(set_device(c));
    CHECK(ensure_map(c)); // an optimize() still owed belongs to the state that is asked about
    CHECK(char_alloc(c));
    CHECK(char_classes(c));
    snesimage_charwork &w = *c->chr;
    const uint32_t ntile = char_ntile(c);
    snes::CharInfo info{};
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    if (rep) HIPCHK(hipMemcpyAsync(rep, w.rep, sizeof(uint16_t) * ntile, hipMemcpyDeviceToHost, c->stream));
    if (flip) HIPCHK(hipMemcpyAsync(flip, w.flip, ntile, hipMemcpyDeviceToHost, c->stream));
    if (chars) HIPCHK(hipMemcpyAsync(chars, w.chars, 64 * (size_t)ntile, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (unique) *unique = info.unique;
    return SNES_OK;
}

int32_t snesimage_merge_shortlist(snesimage_ctx *c, uint32_t k, uint16_t *tiles, uint16_t *donors, uint8_t *flips, uint64_t *costs, uint32_t *n) {
    CHECK(char_check(c));
    if (!n) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(char_shortlist_len(&k));
    CHECK(set_device(c));
    CHECK(ensure_map(c));
    CHECK(ensure_tables(c));
    CHECK(char_alloc(c));
    CHECK(char_shortlist(c, k));
    snesimage_charwork &w = *c->chr;
    snes::CharInfo info{};
    unsigned long long keys[kCharShort];
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(keys, w.keys, sizeof(keys), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (info.nshort > k) return fail(SNES_ERR_HIP, "merge shortlist: bad count");
    for (uint32_t j = 0; j < info.nshort; j++) {
        if (tiles) tiles[j] = (uint16_t)((keys[j] >> 12) & 1023u);
        if (donors) donors[j] = (uint16_t)((keys[j] >> 2) & 1023u);
        if (flips) flips[j] = (uint8_t)(keys[j] & 3u);
        if (costs) costs[j] = keys[j] >> 22;
    }
    *n = info.nshort;
    return SNES_OK;
}

int32_t snesimage_score_merges(snesimage_ctx *c, const uint16_t *tiles, const uint16_t *donors, const uint8_t *flips, uint32_t n, double *errors, uint8_t *maps_out) {
    CHECK(char_check(c));
    if (!tiles || !donors || !flips || !errors) return fail(SNES_ERR_ARG, "null pointer");
    if (n == 0) return SNES_OK;
    const uint32_t ntile = char_ntile(c);
    std::vector<unsigned long long> keys(n);
    for (uint32_t j = 0; j < n; j++) {
        if (tiles[j] >= ntile || donors[j] >= ntile) return fail(SNES_ERR_ARG, "tile beyond the image");
        if (tiles[j] == donors[j]) return fail(SNES_ERR_ARG, "a tile cannot be merged with itself");
        if (flips[j] > 3) return fail(SNES_ERR_ARG, "a flip is 0 .. 3 (bit 0 horizontal, bit 1 vertical)");
        if (char_pinned(c, tiles[j]) || char_pinned(c, donors[j])) return fail(SNES_ERR_ARG, "a tile with a transparent pixel is pinned: it is neither changed nor copied");
        keys[j] = ((unsigned long long)tiles[j] << 12) | ((unsigned long long)donors[j] << 2) | flips[j];
    }
    CHECK(set_device(c));
    uint32_t group = tile_group(c) < kTileGroup ? tile_group(c) : kTileGroup;
    if (n < group) group = n;
    CHECK(char_alloc(c));
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, group, &base_map, true));
    snesimage_tilework &t = *c->tile;
    for (uint32_t c0 = 0; c0 < n; c0 += group) {
        const uint32_t nc = n - c0 < group ? n - c0 : group;
        HIPCHK(hipMemcpyAsync(c->chr->keys, keys.data() + c0, sizeof(unsigned long long) * nc, hipMemcpyHostToDevice, c->stream));
        CHECK(char_score_group(c, nc, t.errs));
        HIPCHK(hipMemcpyAsync(errors + c0, t.errs, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
        if (maps_out) HIPCHK(hipMemcpyAsync(maps_out + (size_t)c0 * c->npx, t.lmaps, c->npx * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

int32_t snesimage_reduce_characters(snesimage_ctx *c, uint32_t max_unique, uint32_t shortlist, snesimage_merge_result *log, uint32_t log_cap, uint32_t *merges, uint32_t *unique) {
    CHECK(char_check(c));
    if (max_unique == 0) return fail(SNES_ERR_ARG, "a budget of no characters cannot be met");
    CHECK(char_shortlist_len(&shortlist));
    CHECK(set_device(c));
    CHECK(ensure_map(c));
    CHECK(ensure_tables(c));
    CHECK(char_alloc(c));
    snesimage_charwork &w = *c->chr;
    CHECK(char_shortlist(c, shortlist));
    snes::CharInfo info{};
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint32_t done = 0;
    if (!(info.unique > max_unique && info.nshort > 0)) { // the budget is met, or nothing can be merged: nothing of the scorer is touched
        if (merges) *merges = 0;
        if (unique) *unique = info.unique;
        return SNES_OK;
    }
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, shortlist, &base_map, true)); // (every allocation comes before the first commit)
    snesimage_tilework &t = *c->tile;
    // One step.  From the launch of the commit on the stored map may be the candidate's: the flags say "a stored map of unknown
    // error" (as after snesimage_set_palette_map) before anything can fail, and the error is taken as known once the record is read.
    auto step = [&]() -> int32_t {
        if (info.nshort > shortlist) return fail(SNES_ERR_HIP, "character reduction: bad shortlist count");
        CHECK(char_score_group(c, info.nshort, t.errs));
        c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
        c->map_synced = false; c->map_pending = false; c->inc_valid = false; c->best_valid = false;
        hipLaunchKernelGGL(k_merge_commit, dim3(1), dim3(64), 0, c->stream, (const double *)t.errs, (const unsigned long long *)w.keys, (int)info.nshort, (const uint8_t *)t.lmaps, (int)c->npx,
                           (int)c->W, c->d_map, c->d_inc_err, w.log);
        HIPCHK(hipGetLastError());
        CHECK(char_shortlist(c, shortlist)); // of the map the commit leaves: what the next step scores
        snes::MergeLog rec{};
        snes::CharInfo next{};
        HIPCHK(hipMemcpyAsync(&rec, w.log, sizeof(rec), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&next, w.info, sizeof(next), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream)); // the one synchronisation of the step
        if (rec.rank == 255) return fail(SNES_ERR_HIP, "character reduction: no candidate of the shortlist has a finite error"); // (nothing was committed)
        c->inc_valid = true;
        info = next;
        rec.unique = (uint16_t)info.unique;
        if (log && done < log_cap) memcpy(log + done, &rec, sizeof(rec));
        done++;
        return SNES_OK;
    };
    while (info.unique > max_unique && info.nshort > 0) {
        const int32_t rc = step();
        if (rc != SNES_OK) { // the steps taken so far stand: report them (after a failed step *unique is the count before it)
            if (merges) *merges = done;
            if (unique) *unique = info.unique;
            return rc;
        }
    }
    if (merges) *merges = done;
    if (unique) *unique = info.unique;
    return SNES_OK;
}

int32_t snesimage_character_fits(snesimage_ctx *c, uint16_t *reps, uint16_t *members, uint64_t *gains, uint8_t *fits, uint32_t *n) {
    CHECK(char_check(c));
    CHECK(set_device(c));
    CHECK(ensure_map(c));
    CHECK(ensure_tables(c));
    CHECK(char_alloc(c));
    CHECK(char_fits(c));
    const uint32_t ntile = char_ntile(c);
    std::vector<snes::RefitFit> fit;
    std::vector<uint8_t> all(fits ? 64 * (size_t)ntile : 0);
    if (fits) HIPCHK(hipMemcpyAsync(all.data(), c->chr->fits, all.size(), hipMemcpyDeviceToHost, c->stream));
    uint32_t unique = 0;
    CHECK(char_fits_read(c, fit, &unique));
    uint32_t k = 0;
    for (uint32_t r = 0; r < ntile; r++) {
        if (!fit[r].eligible) continue;
        if (reps) reps[k] = (uint16_t)r;
        if (members) members[k] = fit[r].members;
        if (gains) gains[k] = fit[r].gain;
        if (fits) memcpy(fits + 64 * (size_t)k, all.data() + 64 * (size_t)r, 64);
        k++;
    }
    if (n) *n = k;
    return SNES_OK;
}

int32_t snesimage_score_refits(snesimage_ctx *c, const uint16_t *reps, uint32_t n, double *errors, uint8_t *maps_out) {
    CHECK(char_check(c));
    if (!reps || !errors) return fail(SNES_ERR_ARG, "null pointer");
    if (n == 0) return SNES_OK;
    const uint32_t ntile = char_ntile(c);
    for (uint32_t j = 0; j < n; j++) if (reps[j] >= ntile) return fail(SNES_ERR_ARG, "tile beyond the image");
    CHECK(set_device(c));
    CHECK(ensure_map(c));
    CHECK(ensure_tables(c));
    CHECK(char_alloc(c));
    CHECK(char_fits(c));
    std::vector<snes::RefitFit> fit;
    uint32_t unique = 0;
    CHECK(char_fits_read(c, fit, &unique));
    for (uint32_t j = 0; j < n; j++)
        if (!fit[reps[j]].eligible) return fail(SNES_ERR_ARG, "not the representative of an eligible class (at least two tiles sharing a character, none of them pinned)");
    uint32_t group = tile_group(c) < kTileGroup ? tile_group(c) : kTileGroup;
    if (n < group) group = n;
    const uint8_t *base_map = nullptr;
    CHECK(tile_prepare(c, group, &base_map, true));
    snesimage_tilework &t = *c->tile;
    double inc = 0.0;
    HIPCHK(hipMemcpyAsync(&inc, c->d_inc_err, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    for (uint32_t c0 = 0; c0 < n; c0 += group) {
        const uint32_t nc = n - c0 < group ? n - c0 : group;
        HIPCHK(hipMemcpyAsync(c->chr->rcalls, reps + c0, sizeof(uint16_t) * nc, hipMemcpyHostToDevice, c->stream));
        CHECK(refit_score_group(c, nc, t.errs));
        HIPCHK(hipMemcpyAsync(errors + c0, t.errs, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
        if (maps_out) HIPCHK(hipMemcpyAsync(maps_out + (size_t)c0 * c->npx, t.lmaps, c->npx * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < n; j++) if (!fit[reps[j]].differs) errors[j] = inc; // the candidate is the stored map: a refit call would not score it
    return SNES_OK;
}

int32_t snesimage_refit_characters(snesimage_ctx *c, uint32_t window, snesimage_refit_result *log, uint32_t log_cap, uint32_t *calls, uint32_t *accepted, uint32_t *unique,
                                   snesimage_run_stats *stats) {
    CHECK(char_check(c));
    CHECK(set_device(c));
    CHECK(ensure_map(c));
    CHECK(ensure_tables(c));
    CHECK(char_alloc(c));
    CHECK(char_fits(c)); // the snapshot: w.rep, w.flip, w.fits and w.fit hold for the whole sweep
    snesimage_charwork &w = *c->chr;
    std::vector<snes::RefitFit> fit;
    uint32_t U = 0;
    CHECK(char_fits_read(c, fit, &U));
    const uint32_t ntile = char_ntile(c);
    std::vector<uint16_t> elig, todo; // the calls in order; those that are scored
    for (uint32_t r = 0; r < ntile; r++) if (fit[r].eligible) { elig.push_back((uint16_t)r); if (fit[r].differs) todo.push_back((uint16_t)r); }
    snesimage_run_stats S{};
    uint32_t n_acc = 0, done = 0; // done: calls logged so far
    auto report = [&]() { if (calls) *calls = (uint32_t)elig.size(); if (accepted) *accepted = n_acc; if (unique) *unique = U; if (stats) *stats = S; };
    if (elig.empty()) { report(); return SNES_OK; }
    uint32_t kmax = tile_group(c) < kTileGroup ? tile_group(c) : kTileGroup;
    if (kmax > todo.size()) kmax = (uint32_t)todo.size();
    if (window == 1) kmax = kmax ? 1 : 0; else if (window > 1 && window < kmax) kmax = window;
    if (kmax) { const uint8_t *base_map = nullptr; CHECK(tile_prepare(c, kmax, &base_map, true)); } // (every allocation comes before the first commit)
    else { CHECK(ensure_source(c)); CHECK(ensure_incumbent(c)); }                                   // nothing to score: the records still carry the incumbent
    double inc = 0.0;
    HIPCHK(hipMemcpyAsync(&inc, c->d_inc_err, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    auto put = [&](const snes::RefitLog &r) { if (log && done < log_cap) memcpy(log + done, &r, sizeof(r)); done++; S.calls++; };
    auto skip_until = [&](uint32_t rep_end) { // the skipped calls in front of class rep_end: not scored, the record's error is the incumbent
        while (done < elig.size() && elig[done] < rep_end) {
            const snes::RefitFit &f = fit[elig[done]];
            snes::RefitLog r{}; r.error = inc; r.gain = f.gain; r.rep = elig[done]; r.members = f.members;
            put(r);
        }
    };
    uint32_t K = window == 0 ? (w.adapt < kmax ? w.adapt : kmax) : kmax;
    if (K < 1) K = 1;
    std::vector<unsigned char> h_res;
    auto run = [&]() -> int32_t {
        snesimage_tilework &t = *c->tile;
        uint32_t pos = 0;
        while (pos < todo.size()) {
            const uint32_t k = K < todo.size() - pos ? K : (uint32_t)(todo.size() - pos);
            HIPCHK(hipMemcpyAsync(w.rcalls, todo.data() + pos, sizeof(uint16_t) * k, hipMemcpyHostToDevice, c->stream));
            CHECK(refit_score_group(c, k, t.errs));
            hipLaunchKernelGGL(k_refit_commit, dim3(1), dim3(1024), 0, c->stream, (const double *)t.errs, (const uint16_t *)w.rcalls, (int)k, (const snes::RefitFit *)w.fit, (const uint8_t *)t.lmaps,
                               (int)c->npx, c->d_map, c->d_inc_err, reinterpret_cast<snes::RefitLog *>(w.rresult + 16), reinterpret_cast<snes::RefitWinRes *>(w.rresult));
            HIPCHK(hipGetLastError());
            h_res.resize(16 + sizeof(snes::RefitLog) * (size_t)k);
            HIPCHK(hipMemcpyAsync(h_res.data(), w.rresult, h_res.size(), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream)); // the one synchronisation of the window
            snes::RefitWinRes res; memcpy(&res, h_res.data(), sizeof(res));
            const uint32_t used = (uint32_t)res.consumed;
            if (used < 1 || used > k || res.accepted >= (int32_t)used) return fail(SNES_ERR_HIP, "refit window: bad commit record");
            for (uint32_t i = 0; i < used; i++) {
                snes::RefitLog r; memcpy(&r, h_res.data() + 16 + sizeof(r) * i, sizeof(r));
                skip_until(todo[pos + i]);
                put(r);
            }
            S.windows += 1; S.scored += k; S.useful += used;
            if (res.accepted >= 0) { // as snesimage_reduce_characters leaves it: a stored map whose error is known
                snes::RefitLog r; memcpy(&r, h_res.data() + 16 + sizeof(r) * (size_t)res.accepted, sizeof(r));
                inc = r.error;
                n_acc++; S.accepted += 1;
                c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
                c->map_synced = false; c->map_pending = false; c->inc_valid = true; c->best_valid = false;
            }
            pos += used;
            if (window == 0) { K = w.policy.next(used, res.accepted >= 0 ? 1u : 0u, kmax < 2 ? kmax : 2u, kmax, 1, k, 0.2); if (K > kmax) K = kmax; if (K < 1) K = 1; w.adapt = K; }
        }
        return SNES_OK;
    };
    int32_t rc = kmax ? run() : SNES_OK;
    if (rc != SNES_OK) { // a window failed: what it left in the map is unknown, the calls accepted before it stand
        c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
        c->map_synced = false; c->map_pending = false; c->inc_valid = false; c->best_valid = false;
        report();
        return rc;
    }
    skip_until(ntile);
    if (n_acc) { // two classes may have become equal: U of the map as it is now
        snes::CharInfo info{};
        rc = char_classes(c);
        if (rc == SNES_OK) {
            if (hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(SNES_ERR_HIP, "refit sweep: the character count could not be read");
            else U = info.unique;
        }
    }
    report();
    return rc;
}

// keys sorted, no spaces, as snesimage_as_json: character, characters, hflip, palette, vflip
int64_t snesimage_as_tilemap_json(snesimage_ctx *c, char *out, int64_t cap) {
    { const int32_t rc = char_check(c); if (rc != SNES_OK) return rc; }
    const uint32_t ntile = char_ntile(c);
    std::vector<uint16_t> rep(ntile); std::vector<uint8_t> flip(ntile), chars(64 * (size_t)ntile), tp(1024);
    uint32_t unique = 0;
    { const int32_t rc = snesimage_characters(c, &unique, rep.data(), flip.data(), chars.data()); if (rc != SNES_OK) return rc; }
    { const int32_t rc = snesimage_get_tile_palettes(c, tp.data()); if (rc != SNES_OK) return rc; }
    std::vector<uint32_t> pos(ntile, 0); // a representative's position in "characters"
    uint32_t nclass = 0;
    for (uint32_t t = 0; t < ntile; t++) if (rep[t] == t) pos[t] = nclass++;
    std::string s = "{\"character\":[";
    for (uint32_t t = 0; t < ntile; t++) { if (t) s += ','; s += std::to_string(pos[rep[t]]); }
    s += "],\"characters\":[";
    for (uint32_t t = 0, k = 0; t < ntile; t++) {
        if (rep[t] != t) continue;
        if (k++) s += ',';
        s += '[';
        for (uint32_t p = 0; p < 64; p++) { if (p) s += ','; s += std::to_string((unsigned)chars[64 * (size_t)t + p]); }
        s += ']';
    }
    s += "],\"hflip\":[";
    for (uint32_t t = 0; t < ntile; t++) { if (t) s += ','; s += (flip[t] & 1) ? '1' : '0'; }
    s += "],\"palette\":[";
    for (uint32_t t = 0; t < ntile; t++) { if (t) s += ','; s += std::to_string((unsigned)tp[t]); }
    s += "],\"vflip\":[";
    for (uint32_t t = 0; t < ntile; t++) { if (t) s += ','; s += (flip[t] & 2) ? '1' : '0'; }
    s += "]}";
    const int64_t need = (int64_t)s.size() + 1;
    if (out && cap > 0) { const int64_t m = cap - 1 < (int64_t)s.size() ? cap - 1 : (int64_t)s.size(); memcpy(out, s.data(), (size_t)m); out[m] = 0; }
    return need;
}

} // extern "C"
