// snesimage_amd/csrc/shared_refit_host.inc — the refit of shared characters across the members of a shared-palette set:
// snesimage_shared_character_fits, snesimage_shared_score_refits, snesimage_shared_refit_characters (definition:
// include/snesimage_hip.h, "refit across the members of a set"; kernels: kernels_char_set.hpp).
//
// A sweep takes the set-wide classes and their fits once (sc_classes, ks_refit_fit: they depend on the snapshot, the members'
// originals and the palette, not on the maps) and reads them back; the host then knows every class's touched members and builds
// the tables of each window itself: call -> (member, candidate number in that member's tile workspace).  A window is the
// members' shares (ks_refit_maps between tile_score_head and tile_score_tail, unchanged, every launch on the set's stream),
// ks_refit_commit, and one synchronisation that reads the records.  A window holds at most kCharShort calls: a member's
// workspace then holds at most that many candidates, as for the set's merges.
// Included by capi.hip behind shared_char_host.inc, whose workspace, member table and stream handling it uses.

namespace {

static_assert(sizeof(snes::SetRefitLog) == sizeof(snesimage_shared_refit_result) && sizeof(snes::SetRefitLog) == 24, "the log record is copied out as it is");
static_assert(sizeof(snes::SetRefitFit) == 16 && sizeof(snes::SetRefitCall) == 8 && sizeof(snes::SetRefitSlot) == 4, "the layout of the set's refit workspace");

// all or nothing, behind sc_alloc: a failed allocation releases the refit's arrays (set and members hold nothing of this)
int32_t sr_alloc(snesimage_shared *s) {
    snesimage_sharedchar &w = *s->chr;
    if (w.refit_ready) return SNES_OK;
    const size_t G = w.G, F = w.F, res_bytes = 16 + sizeof(snes::SetRefitLog) * kCharShort;
    hipStream_t st = s->b->stream;
    auto body = [&]() -> int32_t {
        HIPCHK(dmalloc(&w.rfits, 64 * G)); HIPCHK(dmalloc(&w.rfit, sizeof(snes::SetRefitFit) * G)); HIPCHK(dmalloc(&w.rcalls, sizeof(snes::SetRefitCall) * kCharShort));
        HIPCHK(dmalloc(&w.rslots, sizeof(snes::SetRefitSlot) * kCharShort * F)); HIPCHK(dmalloc(&w.rmreps, sizeof(uint16_t) * kCharShort * F)); HIPCHK(dmalloc(&w.rresult, res_bytes));
        if (g_poison_alloc.load()) { // whatever is read must have been written by the call's own kernels and copies
            HIPCHK(hipMemsetAsync(w.rfits, 0xff, 64 * G, st)); HIPCHK(hipMemsetAsync(w.rfit, 0xff, sizeof(snes::SetRefitFit) * G, st));
            HIPCHK(hipMemsetAsync(w.rcalls, 0xff, sizeof(snes::SetRefitCall) * kCharShort, st)); HIPCHK(hipMemsetAsync(w.rslots, 0xff, sizeof(snes::SetRefitSlot) * kCharShort * F, st));
            HIPCHK(hipMemsetAsync(w.rmreps, 0xff, sizeof(uint16_t) * kCharShort * F, st)); HIPCHK(hipMemsetAsync(w.rresult, 0xff, res_bytes, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return SNES_OK;
    };
    const int32_t rc = body();
    if (rc != SNES_OK) { shared_refit_release(&w); return rc; }
    w.refit_ready = true;
    return SNES_OK;
}

// the snapshot and the fits of a sweep: classes of the members' stored maps, then every eligible class's fit (w.rfits, w.rfit)
int32_t sr_fits(snesimage_shared *s) {
    CHECK(sc_classes(s));
    snesimage_sharedchar &w = *s->chr;
    snesimage_ctx *c0 = members(s)[0];
    hipLaunchKernelGGL(ks_refit_fit, dim3(w.G), dim3(256), 0, s->b->stream, (const snes::SetMember *)w.tab, (int)sc_ntile(s), (int)c0->W, (const uint8_t *)w.pinned, (const uint16_t *)w.rep,
                       (const uint8_t *)w.flip, (const uint16_t *)w.csize, (const uint32_t *)c0->d_pal_rgb8, (int)c0->sub_size, c0->ncol, (int)w.G, (int)w.F, w.rfits, w.rfit);
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

// ... as the host sees them: fit[G], rep[G], U, and every eligible class's touched members in ascending order
struct SrSnapshot { std::vector<snes::SetRefitFit> fit; std::vector<uint16_t> rep; std::vector<std::vector<uint16_t>> touched; uint32_t unique = 0; };
int32_t sr_read(snesimage_shared *s, SrSnapshot &snap) {
    snesimage_sharedchar &w = *s->chr;
    hipStream_t st = s->b->stream;
    const uint32_t ntile = sc_ntile(s);
    snes::CharInfo info{};
    snap.fit.resize(w.G); snap.rep.resize(w.G); snap.touched.assign(w.G, {});
    HIPCHK(hipMemcpyAsync(snap.fit.data(), w.rfit, sizeof(snes::SetRefitFit) * w.G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(snap.rep.data(), w.rep, sizeof(uint16_t) * w.G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    snap.unique = info.unique;
    for (uint32_t g = 0; g < w.G; g++) {
        const uint32_t r = snap.rep[g];
        if (r >= w.G || !snap.fit[r].eligible) continue;
        auto &t = snap.touched[r];
        const uint16_t m = (uint16_t)(g / ntile);
        if (t.empty() || t.back() != m) t.push_back(m); // (g ascends: so do the members)
    }
    for (uint32_t r = 0; r < w.G; r++)
        if (snap.fit[r].eligible && (snap.touched[r].size() != snap.fit[r].touched || snap.rep[r] != r)) return fail(SNES_ERR_HIP, "refit of the set: the fits do not match the classes");
    return SNES_OK;
}

// The tables of one launch set: calls[i] = class reps[i], scored as candidate slots[first + j].slot of member slots[first + j].member
// for each touched member; mreps[m * kCharShort + slot] = the class of member m's candidate `slot`; mcount[m] = member m's candidates.
struct SrWindow { std::vector<snes::SetRefitCall> calls; std::vector<snes::SetRefitSlot> slots; std::vector<uint16_t> mreps; std::vector<uint32_t> mcount; };
void sr_build(const SrSnapshot &snap, const uint16_t *reps, uint32_t k, uint32_t F, SrWindow &win) {
    win.calls.clear(); win.slots.clear(); win.mreps.assign((size_t)F * kCharShort, 0); win.mcount.assign(F, 0);
    for (uint32_t i = 0; i < k; i++) {
        const auto &t = snap.touched[reps[i]];
        win.calls.push_back(snes::SetRefitCall{reps[i], (uint16_t)win.slots.size(), (uint16_t)t.size(), 0});
        for (uint16_t m : t) {
            const uint32_t slot = win.mcount[m]++; // (k <= kCharShort: so is every member's count)
            win.mreps[(size_t)m * kCharShort + slot] = reps[i];
            win.slots.push_back(snes::SetRefitSlot{m, (uint16_t)slot});
        }
    }
}
// ... uploaded, and every member's share scored: maps into the member's lmaps, errors into its errs.  Under ScStreams; `win`
// stays as it is until the set's stream has been synchronised.
int32_t sr_enqueue(snesimage_shared *s, const SrWindow &win) {
    snesimage_sharedchar &w = *s->chr;
    auto &M = members(s);
    hipStream_t st = s->b->stream;
    HIPCHK(hipMemcpyAsync(w.rcalls, win.calls.data(), sizeof(snes::SetRefitCall) * win.calls.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.rslots, win.slots.data(), sizeof(snes::SetRefitSlot) * win.slots.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.rmreps, win.mreps.data(), sizeof(uint16_t) * win.mreps.size(), hipMemcpyHostToDevice, st));
    for (uint32_t m = 0; m < w.F; m++) {
        const uint32_t nc = win.mcount[m];
        if (!nc) continue;
        snesimage_ctx *c = M[m];
        snesimage_tilework &t = *c->tile;
        tile_score_head(c, nc);
        hipLaunchKernelGGL(ks_refit_maps, dim3(nc), dim3(256), 0, c->stream, (const uint16_t *)(w.rmreps + (size_t)m * kCharShort), (const snes::SetMember *)w.tab, (int)m, (int)sc_ntile(s), (int)w.G,
                           (int)c->W, (int)c->npx, (const uint16_t *)w.rep, (const uint8_t *)w.flip, (const uint8_t *)w.rfits, t.lmaps, t.tiles, t.subs);
        CHECK(tile_score_tail(c, nc, t.errs, tile_geom(c)));
    }
    return SNES_OK;
}

uint32_t sr_group(snesimage_shared *s) { const uint32_t g = tile_group(members(s)[0]); return g < (uint32_t)kCharShort ? g : (uint32_t)kCharShort; }

// what every entry point starts with: the snapshot and the fits, read back.  State unchanged.
int32_t sr_snapshot(snesimage_shared *s, SrSnapshot &snap) {
    CHECK(sc_enter(s, true));
    CHECK(sc_alloc(s));
    CHECK(sr_alloc(s));
    CHECK(sc_table(s, false));
    CHECK(sr_fits(s));
    return sr_read(s, snap);
}

// the members' incumbents (known: sc_prepare, or ensure_incumbent) and E, summed in member order as snesimage_shared_error sums
int32_t sr_incumbents(snesimage_shared *s, std::vector<double> &inc, double *E) {
    auto &M = members(s);
    hipStream_t st = s->b->stream;
    inc.assign(M.size(), 0.0);
    for (size_t i = 0; i < M.size(); i++) HIPCHK(hipMemcpyAsync(&inc[i], M[i]->d_inc_err, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double e = 0.0;
    for (size_t i = 0; i < M.size(); i++) e = i == 0 ? inc[i] : e + inc[i];
    *E = e;
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_shared_character_fits(snesimage_shared *s, uint16_t *reps, uint16_t *mem, uint64_t *gains, uint8_t *fits, uint32_t *n) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_character_fits"));
    CHECK(sc_check(s));
    SrSnapshot snap;
    CHECK(sr_snapshot(s, snap));
    snesimage_sharedchar &w = *s->chr;
    std::vector<uint8_t> all(fits ? 64 * (size_t)w.G : 0);
    if (fits) {
        HIPCHK(hipMemcpyAsync(all.data(), w.rfits, all.size(), hipMemcpyDeviceToHost, s->b->stream));
        HIPCHK(hipStreamSynchronize(s->b->stream));
    }
    uint32_t k = 0;
    for (uint32_t r = 0; r < w.G; r++) {
        if (!snap.fit[r].eligible) continue;
        if (reps) reps[k] = (uint16_t)r;
        if (mem) mem[k] = snap.fit[r].members;
        if (gains) gains[k] = snap.fit[r].gain;
        if (fits) memcpy(fits + 64 * (size_t)k, all.data() + 64 * (size_t)r, 64);
        k++;
    }
    if (n) *n = k;
    return SNES_OK;
}

int32_t snesimage_shared_score_refits(snesimage_shared *s, const uint16_t *reps, uint32_t n, double *errors, double *member_errors, uint8_t *maps_out) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_score_refits"));
    if (!s) return fail(SNES_ERR_ARG, "null set");
    if (!reps || !errors) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(sc_check(s));
    CHECK(shared_enter(s, true, true));
    if (n == 0) return SNES_OK;
    auto &M = members(s);
    const uint32_t F = (uint32_t)M.size(), G = F * sc_ntile(s);
    for (uint32_t j = 0; j < n; j++) if (reps[j] >= G) return fail(SNES_ERR_ARG, "tile beyond the set");
    SrSnapshot snap;
    CHECK(sr_snapshot(s, snap));
    for (uint32_t j = 0; j < n; j++)
        if (!snap.fit[reps[j]].eligible) return fail(SNES_ERR_ARG, "not the representative of an eligible class (at least two tiles of the set sharing a character, none of them pinned)");
    uint32_t group = sr_group(s);
    if (n < group) group = n;
    CHECK(sc_prepare(s, group));
    std::vector<double> inc, e((size_t)n * F);
    double E = 0.0;
    CHECK(sr_incumbents(s, inc, &E));
    hipStream_t st = s->b->stream;
    const size_t npx = M[0]->npx;
    for (uint32_t j = 0; j < n; j++)
        for (uint32_t m = 0; m < F; m++) { // an untouched member, and a class whose fit equals its character: the incumbent and the stored map
            e[(size_t)j * F + m] = inc[m];
            if (maps_out) HIPCHK(hipMemcpyAsync(maps_out + ((size_t)j * F + m) * npx, M[m]->d_map, npx, hipMemcpyDeviceToHost, st));
        }
    ScStreams on_set(s);
    SrWindow win;
    std::vector<uint16_t> chunk;
    for (uint32_t c0 = 0; c0 < n; c0 += group) {
        const uint32_t nc = n - c0 < group ? n - c0 : group;
        chunk.clear();
        std::vector<uint32_t> which; // the chunk's classes that are scored, in the caller's order
        for (uint32_t j = c0; j < c0 + nc; j++) if (snap.fit[reps[j]].differs) { chunk.push_back(reps[j]); which.push_back(j); }
        if (chunk.empty()) continue;
        sr_build(snap, chunk.data(), (uint32_t)chunk.size(), F, win);
        CHECK(sr_enqueue(s, win));
        for (size_t i = 0; i < chunk.size(); i++) {
            const snes::SetRefitCall &call = win.calls[i];
            for (uint32_t k = 0; k < call.count; k++) {
                const snes::SetRefitSlot sl = win.slots[call.first + k];
                const size_t at = (size_t)which[i] * F + sl.member;
                HIPCHK(hipMemcpyAsync(&e[at], M[sl.member]->tile->errs + sl.slot, sizeof(double), hipMemcpyDeviceToHost, st));
                if (maps_out) HIPCHK(hipMemcpyAsync(maps_out + at * npx, M[sl.member]->tile->lmaps + (size_t)sl.slot * npx, npx, hipMemcpyDeviceToHost, st));
            }
        }
        HIPCHK(hipStreamSynchronize(st)); // the tables are free again
    }
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t j = 0; j < n; j++) {
        double sum = 0.0;
        for (uint32_t m = 0; m < F; m++) { const double v = e[(size_t)j * F + m]; sum = m == 0 ? v : sum + v; } // member order, as ks_refit_commit sums
        errors[j] = snap.fit[reps[j]].differs ? sum : E;
    }
    if (member_errors) memcpy(member_errors, e.data(), sizeof(double) * e.size());
    return SNES_OK;
}

int32_t snesimage_shared_refit_characters(snesimage_shared *s, uint32_t window, snesimage_shared_refit_result *log, uint32_t log_cap, uint32_t *calls, uint32_t *accepted, uint32_t *unique,
                                          snesimage_run_stats *stats) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_refit_characters"));
    if (!s) return fail(SNES_ERR_ARG, "null set");
    CHECK(sc_check(s));
    SrSnapshot snap; // holds for the whole sweep, as w.rep, w.flip, w.rfits and w.rfit do
    CHECK(sr_snapshot(s, snap));
    snesimage_sharedchar &w = *s->chr;
    auto &M = members(s);
    const uint32_t F = w.F, G = w.G;
    hipStream_t st = s->b->stream;
    std::vector<uint16_t> elig, todo; // the calls in order; those that are scored
    for (uint32_t r = 0; r < G; r++) if (snap.fit[r].eligible) { elig.push_back((uint16_t)r); if (snap.fit[r].differs) todo.push_back((uint16_t)r); }
    snesimage_run_stats S{};
    uint32_t n_acc = 0, done = 0, U = snap.unique; // done: calls logged so far
    auto report = [&]() { if (calls) *calls = (uint32_t)elig.size(); if (accepted) *accepted = n_acc; if (unique) *unique = U; if (stats) *stats = S; };
    if (elig.empty()) { report(); return SNES_OK; }
    uint32_t kmax = sr_group(s);
    if (kmax > todo.size()) kmax = (uint32_t)todo.size();
    if (window == 1) kmax = kmax ? 1 : 0; else if (window > 1 && window < kmax) kmax = window;
    if (kmax) { CHECK(sc_prepare(s, kmax)); } // (every allocation comes before the first commit)
    else { // nothing to score: the records still carry E
        for (auto *c : M) { CHECK(ensure_source(c)); CHECK(ensure_incumbent(c)); }
        for (auto *c : M) HIPCHK(hipStreamSynchronize(c->stream));
    }
    std::vector<double> inc;
    double E = 0.0;
    CHECK(sr_incumbents(s, inc, &E));
    auto put = [&](const snes::SetRefitLog &r) { if (log && done < log_cap) memcpy(log + done, &r, sizeof(r)); done++; S.calls++; };
    auto skip_until = [&](uint32_t rep_end) { // the skipped calls in front of class rep_end: not scored, the record's error is E
        while (done < elig.size() && elig[done] < rep_end) {
            const snes::SetRefitFit &f = snap.fit[elig[done]];
            snes::SetRefitLog r{}; r.error = E; r.gain = f.gain; r.rep = elig[done]; r.members = f.members; r.touched = f.touched;
            put(r);
        }
    };
    if (!kmax) { skip_until(G); report(); return SNES_OK; }
    uint32_t K = window == 0 ? (w.radapt < kmax ? w.radapt : kmax) : kmax;
    if (K < 1) K = 1;
    const bool was_reduced = s->reduced;
    struct Flags { bool pack_valid, plist_valid, map_synced, map_pending, inc_valid, best_valid, epoch_by_commit; };
    std::vector<Flags> saved(F);
    std::vector<unsigned char> h_res;
    SrWindow win;
    ScStreams on_set(s);
    // One window.  From the launch of the commit on, the stored map of any member touched by a call of the window may be a
    // candidate's: their flags say "a stored map of unknown error" before anything can fail.  Once the records are read the
    // members touched by the accepted call keep that state with their error known and their new epoch recorded in the set; the
    // others are as they were.
    auto run = [&]() -> int32_t {
        uint32_t pos = 0;
        while (pos < todo.size()) {
            const uint32_t k = K < todo.size() - pos ? K : (uint32_t)(todo.size() - pos);
            sr_build(snap, todo.data() + pos, k, F, win);
            CHECK(sr_enqueue(s, win));
            for (uint32_t m = 0; m < F; m++) {
                if (!win.mcount[m]) continue;
                snesimage_ctx *c = M[m];
                saved[m] = Flags{c->pack_valid, c->sp.plist_valid, c->map_synced, c->map_pending, c->inc_valid, c->best_valid, c->epoch_by_commit};
                c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
                c->map_synced = false; c->map_pending = false; c->inc_valid = false; c->best_valid = false;
                s->epoch[m] = c->epoch; // (the set did this: it stays intact whatever follows)
            }
            s->reduced = true;
            hipLaunchKernelGGL(ks_refit_commit, dim3(1), dim3(1024), 0, st, (const snes::SetRefitCall *)w.rcalls, (const snes::SetRefitSlot *)w.rslots, (int)k, (const snes::SetRefitFit *)w.rfit,
                               (const snes::SetMember *)w.tab, (int)F, (int)M[0]->npx, reinterpret_cast<snes::SetRefitLog *>(w.rresult + 16), reinterpret_cast<snes::RefitWinRes *>(w.rresult));
            HIPCHK(hipGetLastError());
            h_res.resize(16 + sizeof(snes::SetRefitLog) * (size_t)k);
            HIPCHK(hipMemcpyAsync(h_res.data(), w.rresult, h_res.size(), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st)); // the one synchronisation of the window
            snes::RefitWinRes res; memcpy(&res, h_res.data(), sizeof(res));
            const uint32_t used = (uint32_t)res.consumed;
            if (used < 1 || used > k || res.accepted >= (int32_t)used) return fail(SNES_ERR_HIP, "refit window of the set: bad commit record");
            std::vector<bool> keeps(F, false); // the members the accepted call touched
            if (res.accepted >= 0) for (uint16_t m : snap.touched[todo[pos + (uint32_t)res.accepted]]) keeps[m] = true;
            for (uint32_t m = 0; m < F; m++) {
                if (!win.mcount[m]) continue;
                snesimage_ctx *c = M[m];
                if (keeps[m]) { c->inc_valid = true; continue; }
                const Flags &f = saved[m]; // nothing of this member changed
                c->pack_valid = f.pack_valid; c->sp.plist_valid = f.plist_valid; c->map_synced = f.map_synced; c->map_pending = f.map_pending; c->inc_valid = f.inc_valid; c->best_valid = f.best_valid;
                c->epoch_by_commit = f.epoch_by_commit; c->epoch--; s->epoch[m] = c->epoch;
            }
            for (uint32_t i = 0; i < used; i++) {
                snes::SetRefitLog r; memcpy(&r, h_res.data() + 16 + sizeof(r) * i, sizeof(r));
                skip_until(todo[pos + i]);
                put(r);
            }
            S.windows += 1; S.scored += k; S.useful += used;
            if (res.accepted >= 0) {
                snes::SetRefitLog r; memcpy(&r, h_res.data() + 16 + sizeof(r) * (size_t)res.accepted, sizeof(r));
                E = r.error;
                n_acc++; S.accepted += 1;
            } else if (!n_acc) s->reduced = was_reduced; // nothing was committed so far: the set is as it was
            pos += used;
            if (window == 0) { K = w.rpolicy.next(used, res.accepted >= 0 ? 1u : 0u, kmax < 2 ? kmax : 2u, kmax, 1, k, 0.2); if (K > kmax) K = kmax; if (K < 1) K = 1; w.radapt = K; }
        }
        return SNES_OK;
    };
    int32_t rc = run();
    if (rc != SNES_OK) { report(); return rc; } // a window failed: the calls accepted before it stand; the members it touched hold "a stored map of unknown error"
    skip_until(G);
    if (n_acc) { // two classes may have become equal: U of the maps as they are now
        snes::CharInfo info{};
        rc = sc_classes(s);
        if (rc == SNES_OK) {
            if (hipMemcpyAsync(&info, w.info, sizeof(info), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = fail(SNES_ERR_HIP, "refit sweep of the set: the character count could not be read");
            else U = info.unique;
        }
    }
    report();
    return rc;
}

} // extern "C"
