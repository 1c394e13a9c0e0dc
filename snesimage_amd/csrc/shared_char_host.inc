// snesimage_amd/csrc/shared_char_host.inc — the character budget across the members of a shared-palette set:
// snesimage_shared_characters, snesimage_shared_merge_shortlist, snesimage_shared_score_merges,
// snesimage_shared_reduce_characters, snesimage_shared_as_tilemap_json (definition: include/snesimage_hip.h; kernels:
// kernels_char_set.hpp, and k_char_classes of kernels_char.hpp as it is).
//
// As in char_host.inc nothing is cached between calls or steps: characters, classes and the proxy shortlist are recomputed
// from the members' stored maps whenever they are asked for.  The set-wide kernels run on the set's stream and read the
// members through a device table (snes::SetMember).  A member's share of the shortlist is scored on that member: its maps go
// into the member's own tile workspace (ks_merge_maps) between tile_score_head and tile_score_tail, unchanged.  While a call
// scores, every member's launches are put on the set's stream, so a step is one chain: the members' shares, ks_merge_commit,
// the next step's characters and shortlist, then one synchronisation that reads the record, U and the per-member counts.
// Included by capi.hip behind char_host.inc and tile_host.inc.

struct snesimage_sharedchar {
    bool ready = false;
    uint32_t G = 0, F = 0;
    uint8_t *chars = nullptr, *pinned = nullptr, *flip = nullptr, *spos = nullptr;
    uint16_t *rep = nullptr, *csize = nullptr;
    unsigned long long *part = nullptr, *skeys = nullptr, *mkeys = nullptr; // part: a list of kCharShort keys per global tile; skeys: the shortlist; mkeys: kCharShort keys per member
    uint32_t *mcount = nullptr;
    snes::CharInfo *info = nullptr; snes::SetMergeLog *log = nullptr; snes::SetMember *tab = nullptr;
    std::vector<snes::SetMember> h_tab; // (kept here: the copy to the device may still read it when the filling function returns)
    // the refit across members (shared_refit_host.inc), made on first use: fits[g * 64 + q] and fit[g] of the class global tile g
    // represents; a window's calls, slots and the members' candidate lists (kCharShort each); its result (RefitWinRes, 16 bytes, then kCharShort records)
    bool refit_ready = false;
    uint8_t *rfits = nullptr; snes::SetRefitFit *rfit = nullptr; snes::SetRefitCall *rcalls = nullptr; snes::SetRefitSlot *rslots = nullptr; uint16_t *rmreps = nullptr; unsigned char *rresult = nullptr;
    WindowPolicy rpolicy; uint32_t radapt = 4;
};

namespace {

static_assert(sizeof(snes::SetMergeLog) == sizeof(snesimage_shared_merge_result) && sizeof(snes::SetMergeLog) == 40, "the log record is copied out as it is");

void shared_refit_release(snesimage_sharedchar *w) {
    dfree(w->rfits); dfree(w->rfit); dfree(w->rcalls); dfree(w->rslots); dfree(w->rmreps); dfree(w->rresult);
    w->refit_ready = false;
}
void shared_char_release(snesimage_sharedchar *w) {
    shared_refit_release(w);
    dfree(w->chars); dfree(w->pinned); dfree(w->flip); dfree(w->spos); dfree(w->rep); dfree(w->csize); dfree(w->part); dfree(w->skeys); dfree(w->mkeys); dfree(w->mcount);
    dfree(w->info); dfree(w->log); dfree(w->tab);
    w->ready = false;
}
void shared_char_free(snesimage_sharedchar *w) { shared_char_release(w); delete w; }

uint32_t sc_ntile(snesimage_shared *s) { return char_ntile(members(s)[0]); }

// Null set, a retired set, or more global tiles than the packed key orders: before anything is touched.  (A destroyed member
// stays in the set's list as a dangling pointer: no member is read before this has looked at `dead`.)
int32_t sc_check(snesimage_shared *s) {
    if (!s) return fail(SNES_ERR_ARG, "null set");
    if (s->b->dead) return fail(SNES_ERR_STATE, "a member context of this set was destroyed");
    if ((uint64_t)members(s).size() * sc_ntile(s) > (uint64_t)snes::kSetTiles)
        return fail(SNES_ERR_UNSUPPORTED, "the character budget of a set takes at most 8192 tiles in all (eight frames of 256 x 256, nine of 256 x 224)");
    return SNES_OK;
}

// all or nothing: a failed allocation releases everything (set and members hold nothing of this)
int32_t sc_alloc(snesimage_shared *s) {
    if (!s->chr) s->chr = new snesimage_sharedchar();
    snesimage_sharedchar &w = *s->chr;
    if (w.ready) return SNES_OK;
    const uint32_t F = (uint32_t)members(s).size(), G = F * sc_ntile(s);
    hipStream_t st = s->b->stream;
    auto body = [&]() -> int32_t {
        HIPCHK(dmalloc(&w.chars, 64 * (size_t)G)); HIPCHK(dmalloc(&w.pinned, G)); HIPCHK(dmalloc(&w.flip, G)); HIPCHK(dmalloc(&w.spos, kCharShort));
        HIPCHK(dmalloc(&w.rep, sizeof(uint16_t) * G)); HIPCHK(dmalloc(&w.csize, sizeof(uint16_t) * G));
        HIPCHK(dmalloc(&w.part, sizeof(unsigned long long) * (size_t)G * kCharShort)); HIPCHK(dmalloc(&w.skeys, sizeof(unsigned long long) * kCharShort));
        HIPCHK(dmalloc(&w.mkeys, sizeof(unsigned long long) * (size_t)F * kCharShort)); HIPCHK(dmalloc(&w.mcount, sizeof(uint32_t) * F));
        HIPCHK(dmalloc(&w.info, sizeof(snes::CharInfo))); HIPCHK(dmalloc(&w.log, sizeof(snes::SetMergeLog))); HIPCHK(dmalloc(&w.tab, sizeof(snes::SetMember) * F));
        if (g_poison_alloc.load()) { // whatever is read must have been written by the call's own kernels
            HIPCHK(hipMemsetAsync(w.chars, 0xff, 64 * (size_t)G, st)); HIPCHK(hipMemsetAsync(w.pinned, 0xff, G, st)); HIPCHK(hipMemsetAsync(w.flip, 0xff, G, st));
            HIPCHK(hipMemsetAsync(w.rep, 0xff, sizeof(uint16_t) * G, st)); HIPCHK(hipMemsetAsync(w.csize, 0xff, sizeof(uint16_t) * G, st));
            HIPCHK(hipMemsetAsync(w.part, 0x5a, sizeof(unsigned long long) * (size_t)G * kCharShort, st)); HIPCHK(hipMemsetAsync(w.skeys, 0x5a, sizeof(unsigned long long) * kCharShort, st));
            HIPCHK(hipMemsetAsync(w.mkeys, 0x5a, sizeof(unsigned long long) * (size_t)F * kCharShort, st)); HIPCHK(hipMemsetAsync(w.mcount, 0xff, sizeof(uint32_t) * F, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return SNES_OK;
    };
    const int32_t rc = body();
    if (rc != SNES_OK) { shared_char_release(&w); return rc; }
    w.G = G; w.F = F; w.ready = true;
    return SNES_OK;
}

// What every call starts with: the set intact and idle (the merged maps of an earlier reduction stay), an optimize() still
// owed run on every member, the palette tables, and the members' own streams idle.
int32_t sc_enter(snesimage_shared *s, bool tables) {
    CHECK(shared_enter(s, true, true));
    for (auto *c : members(s)) {
        CHECK(ensure_map(c));
        if (tables) CHECK(ensure_tables(c));
    }
    for (auto *c : members(s)) HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

// the members' pointers for the kernels; work: with the members' tile workspaces (after tile_prepare on each)
int32_t sc_table(snesimage_shared *s, bool work) {
    snesimage_sharedchar &w = *s->chr;
    auto &M = members(s);
    w.h_tab.resize(M.size());
    for (size_t i = 0; i < M.size(); i++) {
        snesimage_ctx *c = M[i];
        w.h_tab[i] = snes::SetMember{c->d_orig, c->d_map, c->d_tile_pal, c->d_inc_err, work ? c->tile->errs : nullptr, work ? c->tile->lmaps : nullptr};
    }
    HIPCHK(hipMemcpyAsync(w.tab, w.h_tab.data(), sizeof(snes::SetMember) * M.size(), hipMemcpyHostToDevice, s->b->stream));
    return SNES_OK;
}

// characters, classes and U of the members' stored maps (info->unique), on the set's stream
int32_t sc_classes(snesimage_shared *s) {
    snesimage_sharedchar &w = *s->chr;
    snesimage_ctx *c0 = members(s)[0];
    hipStream_t st = s->b->stream;
    hipLaunchKernelGGL(ks_char_build, dim3(w.G), dim3(64), 0, st, (const snes::SetMember *)w.tab, (int)sc_ntile(s), (int)c0->W, w.chars, w.pinned);
    hipLaunchKernelGGL(k_char_classes, dim3(w.G), dim3(256), 0, st, (const uint8_t *)w.chars, w.rep, w.flip);
    hipLaunchKernelGGL(ks_char_count, dim3(1), dim3(1024), 0, st, (const uint16_t *)w.rep, (int)w.G, w.csize, w.info);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}
// and the K lowest candidates of the proxy into w.skeys (info->nshort), split by recipient member into w.mkeys / w.mcount
int32_t sc_shortlist(snesimage_shared *s, uint32_t k) {
    CHECK(sc_classes(s));
    snesimage_sharedchar &w = *s->chr;
    snesimage_ctx *c0 = members(s)[0];
    hipStream_t st = s->b->stream;
    hipLaunchKernelGGL(ks_merge_proxy, dim3(w.G), dim3(256), sizeof(uint32_t) * 64 * (size_t)c0->sub_size, st, (const snes::SetMember *)w.tab, (int)sc_ntile(s), (int)c0->W, (const uint8_t *)w.chars,
                       (const uint8_t *)w.pinned, (const uint16_t *)w.rep, (const uint16_t *)w.csize, (const uint32_t *)c0->d_pal_rgb8, (int)c0->sub_size, (int)w.G, (int)k, w.part);
    hipLaunchKernelGGL(ks_merge_topk, dim3(1), dim3(1024), 0, st, (const unsigned long long *)w.part, (int)w.G, (int)sc_ntile(s), (int)w.F, (int)k, w.skeys, w.spos, w.mkeys, w.mcount, w.info);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

// While it lives every member's launches go to the set's stream (the members' own streams are idle: sc_enter, sc_prepare).
struct ScStreams {
    snesimage_shared *s; std::vector<hipStream_t> saved;
    explicit ScStreams(snesimage_shared *s_) : s(s_) { for (auto *c : members(s)) { saved.push_back(c->stream); c->stream = s->b->stream; } }
    ~ScStreams() { (void)hipStreamSynchronize(s->b->stream); size_t i = 0; for (auto *c : members(s)) c->stream = saved[i++]; } // (idle already unless a step failed half-way)
};

// every member ready to score `need` candidates from its stored map, its incumbent known; then the table with the workspaces
int32_t sc_prepare(snesimage_shared *s, uint32_t need) {
    for (auto *c : members(s)) { const uint8_t *base_map = nullptr; CHECK(tile_prepare(c, need, &base_map, true)); }
    for (auto *c : members(s)) HIPCHK(hipStreamSynchronize(c->stream));
    return sc_table(s, true);
}

// member m's nc candidates at w.mkeys[m * 64 ..]: maps into the member's lmaps, errors into its errs[0, nc).  Under ScStreams.
int32_t sc_score_member(snesimage_shared *s, uint32_t m, uint32_t nc) {
    snesimage_sharedchar &w = *s->chr;
    snesimage_ctx *c = members(s)[m];
    snesimage_tilework &t = *c->tile;
    tile_score_head(c, nc);
    hipLaunchKernelGGL(ks_merge_maps, dim3(nc), dim3(256), 0, c->stream, (const unsigned long long *)(w.mkeys + (size_t)m * kCharShort), (const snes::SetMember *)w.tab, (int)m, (int)sc_ntile(s),
                       (int)w.F, (int)c->W, (int)c->npx, t.lmaps, t.tiles, t.subs);
    return tile_score_tail(c, nc, t.errs, tile_geom(c));
}

} // namespace

extern "C" {

int32_t snesimage_shared_characters(snesimage_shared *s, uint32_t *unique, uint16_t *rep, uint8_t *flip, uint8_t *chars) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_characters"));
    CHECK(sc_check(s));
    CHECK(sc_enter(s, false));
    CHECK(sc_alloc(s));
    CHECK(sc_table(s, false));
    CHECK(sc_classes(s));
    snesimage_sharedchar &w = *s->chr;
    hipStream_t st = s->b->stream;
    snes::CharInfo info{};
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, st));
    if (rep) HIPCHK(hipMemcpyAsync(rep, w.rep, sizeof(uint16_t) * w.G, hipMemcpyDeviceToHost, st));
    if (flip) HIPCHK(hipMemcpyAsync(flip, w.flip, w.G, hipMemcpyDeviceToHost, st));
    if (chars) HIPCHK(hipMemcpyAsync(chars, w.chars, 64 * (size_t)w.G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (unique) *unique = info.unique;
    return SNES_OK;
}

int32_t snesimage_shared_merge_shortlist(snesimage_shared *s, uint32_t k, uint16_t *mem, uint16_t *tiles, uint16_t *donor_members, uint16_t *donors, uint8_t *flips, uint64_t *costs,
                                         uint32_t *n) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_merge_shortlist"));
    if (!s || !n) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(char_shortlist_len(&k));
    CHECK(sc_check(s));
    CHECK(sc_enter(s, true));
    CHECK(sc_alloc(s));
    CHECK(sc_table(s, false));
    CHECK(sc_shortlist(s, k));
    snesimage_sharedchar &w = *s->chr;
    hipStream_t st = s->b->stream;
    snes::CharInfo info{};
    unsigned long long keys[kCharShort];
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(keys, w.skeys, sizeof(keys), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (info.nshort > k) return fail(SNES_ERR_HIP, "merge shortlist of the set: bad count");
    const uint32_t ntile = sc_ntile(s);
    for (uint32_t j = 0; j < info.nshort; j++) {
        const uint32_t gt = (uint32_t)((keys[j] >> 15) & 8191u), gb = (uint32_t)((keys[j] >> 2) & 8191u);
        if (mem) mem[j] = (uint16_t)(gt / ntile);
        if (tiles) tiles[j] = (uint16_t)(gt % ntile);
        if (donor_members) donor_members[j] = (uint16_t)(gb / ntile);
        if (donors) donors[j] = (uint16_t)(gb % ntile);
        if (flips) flips[j] = (uint8_t)(keys[j] & 3u);
        if (costs) costs[j] = keys[j] >> 28;
    }
    *n = info.nshort;
    return SNES_OK;
}

int32_t snesimage_shared_score_merges(snesimage_shared *s, const uint16_t *mem, const uint16_t *tiles, const uint16_t *donor_members, const uint16_t *donors, const uint8_t *flips, uint32_t n,
                                      double *errors, uint8_t *maps_out) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_score_merges"));
    if (!s || !mem || !tiles || !donor_members || !donors || !flips || !errors) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(sc_check(s));
    CHECK(shared_enter(s, true, true)); // (the set intact before a member is asked which of its tiles are pinned)
    if (n == 0) return SNES_OK;
    auto &M = members(s);
    const uint32_t ntile = sc_ntile(s), F = (uint32_t)M.size();
    std::vector<std::vector<uint32_t>> share(F); // each member's candidates, in the order given
    std::vector<unsigned long long> keys(n);
    for (uint32_t j = 0; j < n; j++) {
        if (mem[j] >= F || donor_members[j] >= F) return fail(SNES_ERR_ARG, "member beyond the set");
        if (tiles[j] >= ntile || donors[j] >= ntile) return fail(SNES_ERR_ARG, "tile beyond the image");
        const uint32_t gt = mem[j] * ntile + tiles[j], gb = donor_members[j] * ntile + donors[j];
        if (gt == gb) return fail(SNES_ERR_ARG, "a tile cannot be merged with itself");
        if (flips[j] > 3) return fail(SNES_ERR_ARG, "a flip is 0 .. 3 (bit 0 horizontal, bit 1 vertical)");
        if (char_pinned(M[mem[j]], tiles[j]) || char_pinned(M[donor_members[j]], donors[j])) return fail(SNES_ERR_ARG, "a tile with a transparent pixel is pinned: it is neither changed nor copied");
        keys[j] = ((unsigned long long)gt << 15) | ((unsigned long long)gb << 2) | flips[j];
        share[mem[j]].push_back(j);
    }
    CHECK(sc_enter(s, true));
    CHECK(sc_alloc(s));
    uint32_t group = tile_group(M[0]) < (uint32_t)kCharShort ? tile_group(M[0]) : (uint32_t)kCharShort; // a member's row of w.mkeys
    if (n < group) group = n;
    CHECK(sc_prepare(s, group));
    snesimage_sharedchar &w = *s->chr;
    hipStream_t st = s->b->stream;
    ScStreams on_set(s);
    std::vector<unsigned long long> h_keys;
    for (uint32_t m = 0; m < F; m++) {
        snesimage_ctx *c = M[m];
        for (size_t c0 = 0; c0 < share[m].size(); c0 += group) {
            const uint32_t nc = (uint32_t)(share[m].size() - c0 < group ? share[m].size() - c0 : group);
            h_keys.resize(nc);
            for (uint32_t i = 0; i < nc; i++) h_keys[i] = keys[share[m][c0 + i]];
            HIPCHK(hipMemcpyAsync(w.mkeys + (size_t)m * kCharShort, h_keys.data(), sizeof(unsigned long long) * nc, hipMemcpyHostToDevice, st));
            CHECK(sc_score_member(s, m, nc));
            for (uint32_t i = 0; i < nc; i++) { // (the candidates come back in the caller's order)
                const uint32_t j = share[m][c0 + i];
                HIPCHK(hipMemcpyAsync(errors + j, c->tile->errs + i, sizeof(double), hipMemcpyDeviceToHost, st));
                if (maps_out) HIPCHK(hipMemcpyAsync(maps_out + (size_t)j * c->npx, c->tile->lmaps + (size_t)i * c->npx, c->npx, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipStreamSynchronize(st)); // h_keys is free again
        }
    }
    return SNES_OK;
}

int32_t snesimage_shared_reduce_characters(snesimage_shared *s, uint32_t max_unique, uint32_t shortlist, snesimage_shared_merge_result *log, uint32_t log_cap, uint32_t *merges,
                                           uint32_t *unique) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_reduce_characters"));
    if (!s) return fail(SNES_ERR_ARG, "null set");
    if (max_unique == 0) return fail(SNES_ERR_ARG, "a budget of no characters cannot be met");
    CHECK(char_shortlist_len(&shortlist));
    CHECK(sc_check(s));
    CHECK(sc_enter(s, true));
    CHECK(sc_alloc(s));
    CHECK(sc_table(s, false));
    snesimage_sharedchar &w = *s->chr;
    auto &M = members(s);
    const uint32_t F = (uint32_t)M.size();
    hipStream_t st = s->b->stream;
    CHECK(sc_shortlist(s, shortlist));
    snes::CharInfo info{};
    std::vector<uint32_t> mcount(F), next_count(F);
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mcount.data(), w.mcount, sizeof(uint32_t) * F, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint32_t done = 0;
    auto report = [&]() { if (merges) *merges = done; if (unique) *unique = info.unique; };
    if (!(info.unique > max_unique && info.nshort > 0)) { report(); return SNES_OK; } // the budget is met, or nothing can be merged: nothing of the scorer is touched
    CHECK(sc_prepare(s, shortlist)); // (every allocation comes before the first commit)
    ScStreams on_set(s);
    struct Flags { bool pack_valid, plist_valid, map_synced, map_pending, inc_valid, best_valid, epoch_by_commit; };
    std::vector<Flags> saved(F);
    // One step.  From the launch of the commit on, the stored map of any member with a candidate may be the candidate's: their
    // flags say "a stored map of unknown error" before anything can fail.  Once the record is read the winner's member keeps
    // that state with its error known and its new epoch recorded in the set; the others are as they were.
    auto step = [&]() -> int32_t {
        uint32_t total = 0;
        for (uint32_t m = 0; m < F; m++) total += mcount[m];
        if (info.nshort > shortlist || total != info.nshort) return fail(SNES_ERR_HIP, "character reduction of the set: bad shortlist count");
        for (uint32_t m = 0; m < F; m++) if (mcount[m]) CHECK(sc_score_member(s, m, mcount[m]));
        for (uint32_t m = 0; m < F; m++) {
            if (!mcount[m]) continue;
            snesimage_ctx *c = M[m];
            saved[m] = Flags{c->pack_valid, c->sp.plist_valid, c->map_synced, c->map_pending, c->inc_valid, c->best_valid, c->epoch_by_commit};
            c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
            c->map_synced = false; c->map_pending = false; c->inc_valid = false; c->best_valid = false;
            s->epoch[m] = c->epoch; // (the set did this: it stays intact whatever follows)
        }
        s->reduced = true;
        hipLaunchKernelGGL(ks_merge_commit, dim3(1), dim3(64), 0, st, (const unsigned long long *)w.skeys, (const uint8_t *)w.spos, (int)info.nshort, (const snes::SetMember *)w.tab, (int)sc_ntile(s),
                           (int)F, (int)M[0]->npx, (int)M[0]->W, w.log);
        HIPCHK(hipGetLastError());
        CHECK(sc_shortlist(s, shortlist)); // of the maps the commit leaves: what the next step scores
        snes::SetMergeLog rec{};
        snes::CharInfo next{};
        HIPCHK(hipMemcpyAsync(&rec, w.log, sizeof(rec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&next, w.info, sizeof(next), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(next_count.data(), w.mcount, sizeof(uint32_t) * F, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st)); // the one synchronisation of the step
        const bool won = rec.rank != 255 && rec.member < F && mcount[rec.member] > 0;
        for (uint32_t m = 0; m < F; m++) {
            if (!mcount[m]) continue;
            snesimage_ctx *c = M[m];
            if (won && m == rec.member) { c->inc_valid = true; continue; }
            const Flags &f = saved[m]; // nothing of this member changed
            c->pack_valid = f.pack_valid; c->sp.plist_valid = f.plist_valid; c->map_synced = f.map_synced; c->map_pending = f.map_pending; c->inc_valid = f.inc_valid; c->best_valid = f.best_valid;
            c->epoch_by_commit = f.epoch_by_commit; c->epoch--; s->epoch[m] = c->epoch;
        }
        if (!won) return fail(SNES_ERR_HIP, "character reduction of the set: no candidate of the shortlist has a finite error"); // (nothing was committed)
        info = next; mcount.swap(next_count);
        rec.unique = (uint16_t)info.unique;
        if (log && done < log_cap) memcpy(log + done, &rec, sizeof(rec));
        done++;
        return SNES_OK;
    };
    while (info.unique > max_unique && info.nshort > 0) {
        const int32_t rc = step();
        if (rc != SNES_OK) { report(); return rc; } // the steps taken so far stand (after a failed step *unique is the count before it)
    }
    report();
    return SNES_OK;
}

// keys sorted, no spaces: character, hflip, palette, vflip as lists of F lists in member order; characters one list for the set
int64_t snesimage_shared_as_tilemap_json(snesimage_shared *s, char *out, int64_t cap) {
    { const int32_t rc = shared_refuse_backdrop(s, "snesimage_shared_as_tilemap_json"); if (rc != SNES_OK) return rc; }
    { const int32_t rc = sc_check(s); if (rc != SNES_OK) return rc; }
    auto &M = members(s);
    const uint32_t ntile = sc_ntile(s), F = (uint32_t)M.size(), G = F * ntile;
    std::vector<uint16_t> rep(G); std::vector<uint8_t> flip(G), chars(64 * (size_t)G), tp(1024 * (size_t)F);
    uint32_t unique = 0;
    { const int32_t rc = snesimage_shared_characters(s, &unique, rep.data(), flip.data(), chars.data()); if (rc != SNES_OK) return rc; }
    for (uint32_t i = 0; i < F; i++) { const int32_t rc = snesimage_get_tile_palettes(M[i], tp.data() + 1024 * (size_t)i); if (rc != SNES_OK) return rc; }
    std::vector<uint32_t> pos(G, 0); // a representative's position in "characters"
    uint32_t nclass = 0;
    for (uint32_t g = 0; g < G; g++) if (rep[g] == g) pos[g] = nclass++;
    auto per_member = [&](std::string &s_, auto value) {
        for (uint32_t i = 0; i < F; i++) {
            s_ += i ? ",[" : "[";
            for (uint32_t t = 0; t < ntile; t++) { if (t) s_ += ','; s_ += std::to_string(value(i, i * ntile + t, t)); }
            s_ += ']';
        }
    };
    std::string j = "{\"character\":[";
    per_member(j, [&](uint32_t, uint32_t g, uint32_t) { return (unsigned)pos[rep[g]]; });
    j += "],\"characters\":[";
    for (uint32_t g = 0, k = 0; g < G; g++) {
        if (rep[g] != g) continue;
        if (k++) j += ',';
        j += '[';
        for (uint32_t p = 0; p < 64; p++) { if (p) j += ','; j += std::to_string((unsigned)chars[64 * (size_t)g + p]); }
        j += ']';
    }
    j += "],\"hflip\":[";
    per_member(j, [&](uint32_t, uint32_t g, uint32_t) { return (unsigned)(flip[g] & 1); });
    j += "],\"palette\":[";
    per_member(j, [&](uint32_t i, uint32_t, uint32_t t) { return (unsigned)tp[1024 * (size_t)i + t]; });
    j += "],\"vflip\":[";
    per_member(j, [&](uint32_t, uint32_t g, uint32_t) { return (unsigned)((flip[g] >> 1) & 1); });
    j += "]}";
    const int64_t need = (int64_t)j.size() + 1;
    if (out && cap > 0) { const int64_t m = cap - 1 < (int64_t)j.size() ? cap - 1 : (int64_t)j.size(); memcpy(out, j.data(), (size_t)m); out[m] = 0; }
    return need;
}

} // extern "C"
