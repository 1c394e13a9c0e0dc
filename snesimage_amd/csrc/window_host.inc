// snesimage_amd/csrc/window_host.inc — speculative multi-slot stepping: the reference's own optimizer loop
// (lib.rs:888-933 calling lib.rs:191-240 with 64 candidates, lib.rs:286-328 with 32), several calls per launch.
//
// One call of that loop is 64 (32, 56) candidates: ~1 % of what fills the chip, and ~20 dependent launches of
// single-wave chains.  But call j+1 sees exactly the state call j saw whenever call j accepted nothing — the usual case
// once the optimizer has run for a while (lib.rs:216-219: strict <) — and then its result does not depend on call j at
// all.  A *window* scores the next K calls of the schedule against the current palette in one set of batched launches
// (kernels_batch.hpp: blockIdx.z = call; every call has its own slot context — pack, base image B, candidate storage —
// while the source pyramid, the palette and its tables are the parent's), commits them in order on the device and stops
// behind the first call that changed the state (kw_commit).  The calls behind it were scored against a palette that no
// longer exists: they are discarded and re-run in the next window.  Results are bit-identical to stepping call by call,
// for every K; K follows the acceptance rate seen in the recent windows.
//
// Across GPUs the calls of a window are dealt to the ranks in short runs of consecutive calls (each its own B, its own candidates); the
// only exchange is one min-all-reduce over the window's K x n error vector, after which every rank commits identically.
// Included by capi.hip after batch_host.inc, whose argument blocks and launch sequence it reuses.

// The next window's size: with acceptance rate p a window of K calls gets (1 - (1 - p)^K) / p of them through before the
// first acceptance voids the rest, and costs about t0 + t1 K (a chain of ~25 launches whatever it holds, then ~31 us per
// 64-candidate call: t0 / t1 ~ 15 per rank).  p is estimated from the recent windows (older ones fade by 0.85 per window); the
// size that gets most calls through per unit of time is taken.  Results do not depend on it, only speed does.
struct WindowPolicy {
    double calls = 0.0, accepts = 0.0;
    // weight: what one call of the window costs in units of a single image's call (a set of F members scores every call F times);
    // sizes below 4 (a set whose storage holds few calls) double instead of stepping by 4
    uint32_t next(uint32_t used, uint32_t acc, uint32_t lo, uint32_t hi, uint32_t ranks, uint32_t taken, double weight = 1.0) {
        calls = 0.85 * calls + used; accepts = 0.85 * accepts + acc;
        const double p = (accepts + 0.5) / (calls + 8.0);
        double best = -1.0; uint32_t best_k = lo;
        for (uint32_t k = lo; k <= hi; k = k < 4 ? 2 * k : k + (k < 32 * ranks ? 4 : 8) * ranks) {
            const double through = (1.0 - std::pow(1.0 - p, (double)k)) / p, rate = through / (15.0 + weight * (double)k / ranks);
            if (rate > best) { best = rate; best_k = k; }
        }
        if (!acc && used == taken) { const uint32_t twice = 2 * taken > hi ? hi : 2 * taken; if (twice > best_k) best_k = twice; } // a clean window: at least twice as many next (the estimate takes a few windows to forget a phase of frequent acceptances)
        return best_k;
    }
};

struct WindowRec { // one window in flight: its argument blocks, candidate lists, error vector and result
    // argument blocks and call records of the window: ONE pinned block and ONE device block (the calls' records first, the
    // members' argument blocks behind them), so that a window costs one host-to-device copy
    unsigned char *h_blob = nullptr, *d_blob = nullptr;
    snes::BatchArgs *h_args = nullptr, *d_args = nullptr;   // into the blobs: set per window
    snes::WindowSlot *h_slots = nullptr, *d_slots = nullptr;
    snes::WindowResult *h_res = nullptr, *d_res = nullptr;
    snes::StepResult *h_log = nullptr, *d_log = nullptr;
    uint8_t *d_cand = nullptr; double *d_errs = nullptr;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, args = nullptr, done = nullptr; // [4..6]: the hand-offs of the candidates' second stream (BatchSide::aux) // // B's side-stream hand-offs; argument blocks in place; result on the host
    uint32_t K = 0, stride = 0; bool logged = false;
    int seq = 0, base = 0; // this window's number, and the number of the oldest window in flight when it was enqueued (SNES_BATCH_IMG)
};

struct snesimage_window {
    // slot contexts: own pack + group-sparse storage, everything else borrowed from the parent.  Two sets: the B phase of a
    // window (pack, contested list, B's downscale and sweeps: ~a third of its work, latency-bound) runs on the side stream one
    // window AHEAD — beside the previous window's candidates, which read the other set — on the assumption that the previous
    // window accepts nothing; if it does, the window is void anyway.  (The split-phase API uses set 0 alone.)
    std::vector<snesimage_ctx *> child[2];
    hipEvent_t ev_ready = nullptr; // the main stream has caught up (nothing in flight): the side stream may read the palette and the parent's pack
    uint32_t cap = 0;                   // calls the argument arrays of a window hold
    // The host runs ahead of the device: while window w executes, window w+1 — built on the assumption that w accepts
    // nothing — is already enqueued.  If w does accept, its commit raises *d_dead and every kernel of w+1 leaves at once.
    static constexpr int kRing = 3;
    WindowRec rec[kRing];
    int *d_dead = nullptr; int seq_next = 1; // *d_dead: number of the last window whose commit changed the palette (0: none yet); numbers start at 1 and only grow
    hipStream_t aux = nullptr; bool use_aux = true; // scale 0's H and V passes of a long window beside the rest of it (SNES_WINDOW_AUX=0: one stream)
    bool side_borrowed = false;
    hipStream_t side = nullptr; bool use_side = true; // B's sweeps beside the candidates' first stages (SNES_WINDOW_SIDE=0: in line)
    uint32_t depth = 2;                 // windows in flight (SNES_WINDOW_DEPTH; 1 = a window's B phase in line with its own candidates)
    uint32_t adapt = 8;                 // next window's size when the caller leaves it to the library
    WindowPolicy policy;                // acceptance rate of the recent windows -> size of the next one
    uint32_t clean_streak = 0;          // windows in a row that accepted nothing
    // guided windows (guided_window_host.inc) size themselves: a guided run between two scheduled runs leaves the launch sets of those as they were
    uint32_t g_adapt = 8; WindowPolicy g_policy; uint32_t g_clean_streak = 0;
    // ... and their generator's workspace, for window_max() calls: per call the pixel list, and the counts in front of the cost tables
    snes::GuidePixel *g_list = nullptr; unsigned long long *g_tab = nullptr;
};

namespace {

constexpr uint32_t kWindowMin = 8;
constexpr uint32_t kMemberCand = 96; // candidates a slot context holds: one call of 64, or the three channel calls of an entry (3 x 32)
uint32_t window_max() { // most calls per window (every call keeps ~0.3 GB of candidate storage)
    static uint32_t v = [] { uint32_t m = 64; if (const char *e = getenv("SNES_WINDOW_MAX")) { int x = atoi(e); if (x >= 1 && x <= snes::kMaxWindow) m = (uint32_t)x; } return m; }();
    return v;
}

// What a window can speculate on: the group-sparse path (the batched kernels cover nothing else).
// the scheduler a context's runs follow
void ctx_schedule_next(const snesimage_ctx *c, int nes, uint32_t *palette, uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t *method) {
    if (c->backdrop) snesimage_schedule_next_backdrop(c->sub_count, c->user_size, nes, palette, index, channel, step, method);
    else snesimage_schedule_next(c->sub_count, c->sub_size, nes, palette, index, channel, step, method);
}
bool window_capable(const snesimage_ctx *c) { return c->sp.enabled && !c->owner && !(c->dither && c->sub_size == 1); } // (one-entry subpalettes with --dither: dense path, see score_list)

// A window whose calls are not the scheduler's: the caller of window_enqueue names the slot order and writes the candidate
// lists itself.  next: the slot behind (*palette, *index); generate: n candidates for each of the window's K calls (r.d_slots:
// their slots) into r.d_cand and the errors preset to +inf, on the context's main stream, where kw_gen_candidates runs.
struct WindowGen {
    uint32_t n;
    void (*next)(const snesimage_ctx *c, uint32_t *palette, uint32_t *index);
    int32_t (*generate)(snesimage_ctx *c, WindowRec &r, uint32_t K, uint32_t n, double *d_errors);
};

void window_release_child(snesimage_ctx *k) {
    // borrowed from the parent: not ours to free
    k->d_orig = nullptr; k->d_tile_pal = nullptr; k->d_colors = nullptr; k->d_map = nullptr; k->d_eotf = nullptr; k->d_lab_eotf = nullptr;
    k->d_pal_rgb8 = nullptr; k->d_pal_lin = nullptr; k->d_pal_xyb = nullptr; k->d_pal_lab = nullptr; k->d_lin0 = nullptr; k->d_img1 = nullptr; k->d_img1T = nullptr; k->d_mu1 = nullptr; k->d_sd1 = nullptr;
    k->d_a1 = nullptr; k->d_a1R4 = nullptr; k->d_r1 = nullptr; k->d_r1R4 = nullptr; k->d_img1C4 = nullptr; k->d_mu1R4 = nullptr; k->d_sd1R4 = nullptr; k->d_labpx = nullptr; k->d_labpxT = nullptr; k->d_target = nullptr; k->d_labpx_t = nullptr; k->d_labpxT_t = nullptr;
    k->d_inc_err = nullptr; k->d_last = nullptr; k->d_scratch_err = nullptr; k->d_dummy_cand = nullptr;
    if (k->pack_borrowed) { k->d_pack = nullptr; k->d_packC4 = nullptr; k->d_packR4 = nullptr; k->d_subC4 = nullptr; k->d_subR4 = nullptr; }
    k->stream = nullptr; k->own_stream = nullptr;
    snesimage_destroy(k);
}

// A slot context: the parent's geometry and read-only planes, its own pack (three layouts: the transposed copy feeds the
// general H pass only) and group-sparse storage for one call's candidates plus B.
int32_t window_make_child(snesimage_ctx *c, snesimage_ctx **out) {
    std::unique_ptr<snesimage_ctx, void (*)(snesimage_ctx *)> k(new snesimage_ctx(), window_release_child);
    k->device = c->device; k->W = c->W; k->H = c->H; k->sub_count = c->sub_count; k->sub_size = c->sub_size; k->user_size = c->sub_size; k->flags = c->flags; /* (a slot context scores regular slots of the expanded context: no backdrop of its own) */ k->ncol = c->ncol;
    k->dither_rec = c->dither_rec; k->dither4 = c->dither4; k->dither4_max = c->dither4_max; k->ditherw = c->ditherw; k->sp.ahead.on = false; // (slot contexts take the batched launches: their base images come a window ahead, not a call ahead)
    k->dither = c->dither; k->perceptual = c->perceptual; k->nes = c->nes; k->G = c->G; k->K = c->K; k->npx = c->npx; k->src_floats = c->src_floats; k->fast_mask = c->fast_mask;
    k->chunk = kMemberCand; k->nlanes = 1;
    k->sp.enabled = true; k->sp.side = false; k->sp.lpt = c->sp.lpt; k->sp.down1 = c->sp.down1; k->sp.h2q_max = c->sp.h2q_max; k->sp.scan4_max = c->sp.scan4_max; k->sp.vsplit = c->sp.vsplit; k->sp.down_tiles = c->sp.down_tiles; k->sp.tiles_grid = c->sp.tiles_grid; k->sp.h0_min = c->sp.h0_min; k->sp.hgrid = c->sp.hgrid; k->sp.min_n = 1;
    k->sp.weight_mask = c->sp.weight_mask; k->sp.h_planes = c->sp.h_planes; k->sp.v2_pair = c->sp.v2_pair; k->sp.h_forms = c->sp.h_forms; k->sp.debug_poison = c->sp.debug_poison; // (a slot context reads no environment: the parent's switches, or SNES_H_PLANES=0 would not reach a window)
    k->d_orig = c->d_orig; k->d_tile_pal = c->d_tile_pal; k->d_colors = c->d_colors; k->d_map = c->d_map; k->d_eotf = c->d_eotf; k->d_lab_eotf = c->d_lab_eotf;
    k->d_pal_rgb8 = c->d_pal_rgb8; k->d_pal_lin = c->d_pal_lin; k->d_pal_xyb = c->d_pal_xyb; k->d_pal_lab = c->d_pal_lab;
    k->d_img1C4 = c->d_img1C4; k->d_mu1R4 = c->d_mu1R4; k->d_sd1R4 = c->d_sd1R4; k->d_a1R4 = c->d_a1R4; k->d_r1R4 = c->d_r1R4; k->d_labpx = c->d_labpx; k->d_labpxT = c->d_labpxT; k->d_target = c->d_target; k->d_labpx_t = c->d_labpx_t; k->d_labpxT_t = c->d_labpxT_t; k->od_n = c->od_n; memcpy(k->od_tab, c->od_tab, sizeof k->od_tab);
    k->d_inc_err = c->d_inc_err; k->d_last = c->d_last;
    k->stream = c->stream; // (only sparse_alloc's housekeeping runs on it; the window's launches name their stream themselves)
    k->tables_valid = true; k->src_valid = true;
    if (c->dither) { // the pack does not depend on the slot then (mode 1: transparency marker + stored map): one for all calls, the parent's
        k->pack_borrowed = true;
        k->d_pack = c->d_pack; k->d_packC4 = c->d_packC4; k->d_packR4 = c->d_packR4; k->d_subC4 = c->d_subC4; k->d_subR4 = c->d_subR4;
    } else {
        HIPCHK(dmalloc(&k->d_pack, c->npx * 8));
        HIPCHK(dmalloc(&k->d_packC4, c->npx * 8));
        HIPCHK(dmalloc(&k->d_packR4, c->npx * 8));
    }
    CHECK(sparse_alloc(k.get(), kMemberCand));
    *out = k.release();
    return SNES_OK;
}

size_t window_slots_bytes(uint32_t K) { return (sizeof(snes::WindowSlot) * (size_t)K + 15) & ~(size_t)15; } // the calls' records, padded: the argument blocks follow
size_t window_blob_bytes(uint32_t cap) { return window_slots_bytes(cap) + sizeof(snes::BatchArgs) * (size_t)cap; }
void window_rec_free(WindowRec &r) {
    if (r.h_blob) (void)hipHostFree(r.h_blob); if (r.h_res) (void)hipHostFree(r.h_res); if (r.h_log) (void)hipHostFree(r.h_log);
    r.h_blob = nullptr; r.h_args = nullptr; r.h_slots = nullptr; r.h_res = nullptr; r.h_log = nullptr; r.d_args = nullptr; r.d_slots = nullptr;
    dfree(r.d_blob); dfree(r.d_res); dfree(r.d_log); dfree(r.d_cand); dfree(r.d_errs);
}

void window_free(snesimage_window *w) {
    if (!w) return;
    for (auto &set : w->child) for (auto *k : set) window_release_child(k);
    if (w->ev_ready) (void)hipEventDestroy(w->ev_ready);
    if (w->side) { (void)hipStreamSynchronize(w->side); if (!w->side_borrowed) (void)hipStreamDestroy(w->side); }
    if (w->aux) { (void)hipStreamSynchronize(w->aux); (void)hipStreamDestroy(w->aux); }
    for (auto &r : w->rec) { window_rec_free(r); for (auto &e : r.ev) if (e) (void)hipEventDestroy(e); if (r.done) (void)hipEventDestroy(r.done); if (r.args) (void)hipEventDestroy(r.args); }
    dfree(w->d_dead); dfree(w->g_list); dfree(w->g_tab);
    delete w;
}

// grow-only: slot contexts for `own` calls, argument arrays for windows of K calls (of up to 64 candidates)
int32_t window_reserve(snesimage_ctx *c, uint32_t K, uint32_t own, int set = 0) {
    if (!c->win) {
        c->win = new snesimage_window();
        if (const char *e = getenv("SNES_WINDOW_SIDE")) c->win->use_side = atoi(e) != 0;
        if (const char *e = getenv("SNES_WINDOW_AUX")) c->win->use_aux = atoi(e) != 0;
        if (const char *e = getenv("SNES_WINDOW_DEPTH")) { int v = atoi(e); if (v >= 1) c->win->depth = v > 2 ? 2u : (uint32_t)v; } // (two sets of slot contexts: a window ahead, not two)
    }
    snesimage_window *w = c->win;
    if (!w->d_dead) {
        HIPCHK(dmalloc(&w->d_dead, sizeof(int)));
        HIPCHK(hipMemsetAsync(w->d_dead, 0, sizeof(int), c->stream));
        static const bool borrow = [] { const char *e = getenv("SNES_WINDOW_BORROW"); return !e || atoi(e) != 0; }();
        if (borrow && c->sp.base_stream) { w->side = c->sp.base_stream; w->side_borrowed = true; } // (the parent's stream for its own base images: idle while windows run; one stream fewer)
        else HIPCHK(hipStreamCreateWithFlags(&w->side, hipStreamNonBlocking)); // (a higher or lower priority than the main stream's: within 1-2 % either way)
        for (auto &r : w->rec) { for (auto &e : r.ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&r.done, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&r.args, hipEventDisableTiming)); }
        HIPCHK(hipEventCreateWithFlags(&w->ev_ready, hipEventDisableTiming));
    }
    if (K > w->cap) {
        HIPCHK(hipStreamSynchronize(c->stream));
        w->cap = 0;
        uint32_t cap = 16; while (cap < K) cap *= 2;
        for (auto &r : w->rec) {
            window_rec_free(r);
            HIPCHK(hipHostMalloc(&r.h_blob, window_blob_bytes(cap)));
            HIPCHK(hipHostMalloc(&r.h_log, sizeof(snes::StepResult) * cap));
            HIPCHK(hipHostMalloc(&r.h_res, sizeof(snes::WindowResult)));
            HIPCHK(dmalloc(&r.d_blob, window_blob_bytes(cap)));
            HIPCHK(dmalloc(&r.d_log, sizeof(snes::StepResult) * cap));
            HIPCHK(dmalloc(&r.d_res, sizeof(snes::WindowResult)));
            HIPCHK(dmalloc(&r.d_cand, 3 * 64 * (size_t)cap));
            HIPCHK(dmalloc(&r.d_errs, sizeof(double) * 64 * (size_t)cap));
        }
        w->cap = cap;
    }
    while (w->child[set].size() < own) {
        snesimage_ctx *k = nullptr;
        CHECK(window_make_child(c, &k)); // (sparse_alloc ends with a synchronisation of the stream its clears were queued on — the parent's: a window ahead may use the context on the side stream at once)
        w->child[set].push_back(k);
    }
    return SNES_OK;
}

// Enqueue the scoring of one window: the next calls of the schedule from (palette, index, channel, step) on — at most
// n_slots, cut where the method changes (every call of a window has the same number of candidates) — against the palette
// as it stands when the launches reach the device.  d_errors == nullptr: the record's own vector.
int32_t window_enqueue(snesimage_ctx *c, WindowRec &r, uint32_t n_slots, uint64_t seed, uint64_t first_step_id, uint32_t palette, uint32_t index, uint32_t channel, uint32_t step, uint32_t n_random,
                       uint32_t shard_rank, uint32_t shard_count, double *d_errors, int set = 0, bool ahead = false, const WindowGen *gen = nullptr) {
    snesimage_window *w = c->win;
    struct Call { uint32_t method, palette, index, channel; } calls[snes::kMaxWindow];
    uint32_t K = 0;
    { uint32_t p = palette, i = index, ch = channel, st = step, m = 0, m0 = 0;
      while (K < n_slots) {
          const uint32_t cp = p, ci = i, cc = ch;
          if (c->backdrop && cp == c->sub_count) break; // a window ends in front of a backdrop call (snesimage_run_slots steps it on its own)
          if (gen) { gen->next(c, &p, &i); calls[K++] = Call{SNES_METHOD_RANDOM, cp, ci, 0u}; continue; } // the caller's slot order; committed by the random method's rule
          ctx_schedule_next(c, c->nes ? 1 : 0, &p, &i, &ch, &st, &m);
          if (K == 0) m0 = m; else if (m != m0) break;
          calls[K++] = Call{m, cp, ci, cc};
      } }
    const uint32_t method = calls[0].method, n = gen ? gen->n : method_count(method, n_random);
    if (n > 64) return fail(SNES_ERR_ARG, "a slot window holds at most 64 candidates per call");
    // The window's calls are dealt to the ranks in runs of `deal` consecutive calls, round robin (neighbouring calls walk the
    // entries of one subpalette — the same tiles, much the same contested pixels: a run shares what it reads — while the
    // subpalettes differ in cost by ~10 %: dealt in a few large blocks, the ranks would finish as far apart)
    static const uint32_t deal = [] { uint32_t v = 6; if (const char *e = getenv("SNES_WINDOW_DEAL")) { int x = atoi(e); if (x >= 1) v = (uint32_t)x; } return v; }();
    uint32_t ownj[snes::kMaxWindow], own = 0;
    for (uint32_t j = 0; j < K; j++) if ((j / deal) % shard_count == shard_rank) ownj[own++] = j;
    CHECK(window_reserve(c, K, own, set)); // (slot contexts only: the argument arrays were sized by the caller, never under a window in flight)
    if (!d_errors) d_errors = r.d_errs;
    hipStream_t st = c->stream;
    const size_t args_off = window_slots_bytes(K);
    r.h_slots = reinterpret_cast<snes::WindowSlot *>(r.h_blob); r.d_slots = reinterpret_cast<snes::WindowSlot *>(r.d_blob);
    r.h_args = reinterpret_cast<snes::BatchArgs *>(r.h_blob + args_off); r.d_args = reinterpret_cast<snes::BatchArgs *>(r.d_blob + args_off);
    for (uint32_t j = 0; j < K; j++) {
        snes::WindowSlot &s = r.h_slots[j];
        s.method = (int)calls[j].method; s.n = (int)n; s.slot = (int)(calls[j].palette * c->sub_size + calls[j].index); s.channel = (int)calls[j].channel;
        s.nes = method == SNES_METHOD_NES ? 1 : 0; s.member = -1; s.cand0 = 0; s.pad = 0;
        s.key = mix64(seed ^ ((first_step_id + j) * 0x9E3779B97F4A7C15ull) ^ 0xD1B54A32D192ED03ull);
    }
    // A *member* of the batched launches = this rank's consecutive calls on one palette entry: one call, or — in the channel
    // sweeps, where an entry's three channels follow each other (lib.rs:917-919) — up to three, which share the pack and
    // the base image B (they differ in their candidate lists only): 96 candidates behind one B instead of 32.
    uint32_t members = 0, n_max = 0;
    uint32_t merge_cap = kMemberCand; // (SNES_DEBUG_MEMBER_CAND: tests make the merge rule outgrow the storage to see fill_batch_args refuse it)
    if (const char *e = getenv("SNES_DEBUG_MEMBER_CAND")) { const int v = atoi(e); if (v > 0) merge_cap = (uint32_t)v; }
    for (uint32_t o = 0; o < own;) {
        const uint32_t j = ownj[o];
        uint32_t len = 1;
        while (o + len < own && ownj[o + len] == j + len && n * (len + 1) <= merge_cap && calls[j + len].palette == calls[j].palette && calls[j + len].index == calls[j].index) len++; // (--nes repeats an entry three times too, with 56 candidates each: those stay apart)
        snes::BatchArgs &a = r.h_args[members];
        CHECK(fill_batch_args(a, w->child[set][members], n * len, method, calls[j].palette, calls[j].index, calls[j].channel, r.h_slots[j].key));
        a.dead_base = r.base;
        a.cand = r.d_cand + 3 * (size_t)j * n; a.errors = d_errors + (size_t)j * n; // the calls' lists and errors follow each other in the window's vectors
        for (uint32_t l = 0; l < len; l++) { r.h_slots[j + l].member = (int)members; r.h_slots[j + l].cand0 = (int)(l * n); }
        if (n * len > n_max) n_max = n * len;
        members++; o += len;
    }
    // ahead: argument blocks and B phase on the side stream (it may be running the previous window's B sweeps, or be idle,
    // while the main stream is still busy with the previous window's candidates); the main stream picks up at the events
    const bool whole = ahead && w->use_side;
    hipStream_t as = whole ? w->side : st;
    HIPCHK(hipMemcpyAsync(r.d_blob, r.h_blob, args_off + sizeof(snes::BatchArgs) * members, hipMemcpyHostToDevice, as));
    if (whole) { HIPCHK(hipEventRecord(r.args, as)); HIPCHK(hipStreamWaitEvent(st, r.args, 0)); }
    if (gen) CHECK(gen->generate(c, r, K, n, d_errors)); // the caller's lists in the random candidates' place
    else hipLaunchKernelGGL(kw_gen_candidates, dim3((n + 63) / 64, K), dim3(64), 0, st, r.d_slots, c->d_colors, r.d_cand, d_errors, (int)n, (const int *)w->d_dead, r.base);
    if (members) {
        // B's single-image sweeps (latency-bound: a few waves per call) on a side stream beside the candidates' scan and downscale
        BatchSide bs{w->use_side ? w->side : nullptr, r.ev[0], r.ev[1], r.ev[2], r.ev[3], whole};
        // the second stream exists from the first window that is long enough to use it (enqueue_batched_scoring: 1,024 candidates
        // and more): a stream that merely EXISTS costs the short windows ~90 us each (3.9 k -> 2.9 k calls/s call by call)
        if (w->use_aux && !w->aux && (size_t)n_max * members >= w->child[set][0]->sp.h0_min && w->child[set][0]->sp.h0_min > 0) HIPCHK(hipStreamCreateWithFlags(&w->aux, hipStreamNonBlocking));
        if (w->use_aux && w->aux) { bs.aux = w->aux; bs.a_scan = r.ev[4]; bs.a_h0 = r.ev[5]; bs.a_v0 = r.ev[6]; }
        CHECK(enqueue_batched_scoring(st, r.d_args, members, n_max, w->child[set][0], &bs, w->d_dead));
    }
    HIPCHK(hipGetLastError());
    r.K = K; r.stride = n;
    return SNES_OK;
}

// The window's decisions in schedule order (kw_commit) and its result on its way to the host.
int32_t window_enqueue_commit(snesimage_ctx *c, WindowRec &r, const double *d_errors, bool want_log) {
    snesimage_window *w = c->win;
    if (!d_errors) d_errors = r.d_errs;
    hipStream_t st = c->stream;
    PaletteTables T{};
    T.eotf = c->d_eotf; T.lab_eotf = c->d_lab_eotf; T.rgb8 = c->d_pal_rgb8; T.lin = c->d_pal_lin; T.xyb = c->d_pal_xyb; T.lab = c->perceptual ? c->d_pal_lab : nullptr;
    hipLaunchKernelGGL(kw_commit, dim3(1), dim3(1024), 0, st, r.d_slots, (int)r.K, (int)r.stride, d_errors, r.d_cand, c->d_colors, c->d_inc_err, c->d_last, T, r.d_res, r.d_log, w->d_dead, r.base, r.seq);
    HIPCHK(hipGetLastError());
    if (c->dither) { // lib.rs:237: optimize() of the committed palette — the winner's own resumed run where this rank scored it
        CHECK(alloc_workspace(c, 1)); // (d_skip)
        hipLaunchKernelGGL(kw_take_map, dim3(1), dim3(1024), 0, st, r.d_args, r.d_slots, r.d_res, r.d_log, c->d_map, (int)c->npx, c->d_skip);
        HIPCHK(hipGetLastError());
        CHECK(do_optimize(c, true));
    }
    HIPCHK(hipMemcpyAsync(r.h_res, r.d_res, sizeof(snes::WindowResult), hipMemcpyDeviceToHost, st));
    r.logged = want_log;
    if (want_log) HIPCHK(hipMemcpyAsync(r.h_log, r.d_log, sizeof(snes::StepResult) * r.K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(r.done, st));
    // what snesimage_step_async leaves behind: the palette may have changed, the map of the committed state is owed
    c->pack_valid = false; c->sp.plist_valid = false; c->epoch++; c->epoch_by_commit = false;
    c->map_pending = !c->dither; c->map_synced = true; c->inc_valid = true; c->best_valid = false;
    return SNES_OK;
}

int32_t window_collect(snesimage_ctx *c, WindowRec &r, uint32_t *consumed, uint32_t *accepted, snesimage_call_result *log) {
    HIPCHK(hipEventSynchronize(r.done));
    const uint32_t done = (uint32_t)r.h_res->consumed;
    if (consumed) *consumed = done;
    if (accepted) *accepted = (uint32_t)r.h_res->accepted;
    if (log && r.logged) for (uint32_t j = 0; j < done; j++) { log[j].error = r.h_log[j].error; log[j].best_k = r.h_log[j].best_k; memcpy(log[j].rgb5, r.h_log[j].rgb5, 3); log[j].changed = r.h_log[j].changed; }
    return SNES_OK;
}

int32_t window_prepare(snesimage_ctx *c, uint32_t method) {
    CHECK(ensure_tables(c));
    CHECK(ensure_source(c));
    if (method != SNES_METHOD_NES) CHECK(ensure_incumbent(c)); // lib.rs:199, 294
    if (c->dither) CHECK(run_prep(c, 1, -1, -1)); // the slot contexts read this pack
    return SNES_OK;
}

} // namespace

extern "C" {

// Storage for windows of up to n_slots calls now rather than on first use (~0.3 GB per call).
int32_t snesimage_slots_reserve(snesimage_ctx *c, uint32_t n_slots) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (!window_capable(c)) return SNES_OK; // such a context steps call by call: nothing to reserve
    CHECK(set_device(c));
    if (n_slots > window_max()) n_slots = window_max();
    if (n_slots == 0) n_slots = 1;
    CHECK(window_reserve(c, n_slots, n_slots, 0));
    return c->win->depth > 1 ? window_reserve(c, n_slots, n_slots, 1) : SNES_OK; // (windows in flight alternate between two sets of slot contexts)
}

// Phase 1 of a window, for callers that run the exchange between the ranks themselves.
int32_t snesimage_slots_begin(snesimage_ctx *c, uint32_t n_slots, uint64_t seed, uint64_t first_step_id, uint32_t palette, uint32_t index, uint32_t channel, uint32_t step,
                              uint32_t n_random, uint32_t shard_rank, uint32_t shard_count, double *d_errors, uint32_t *n_taken, uint32_t *stride_out) {
    CHECK(check_slot(c, palette, index));
    if (channel > 2 || n_slots == 0 || shard_count == 0 || shard_rank >= shard_count) return fail(SNES_ERR_ARG, "bad slots_begin arguments");
    if (!window_capable(c)) return fail(SNES_ERR_UNSUPPORTED, "slot windows cover the group-sparse path (not with SNES_SPARSE=0), with --dither subpalettes of two entries and more, and not a context lent to a batch");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending");
    if (c->backdrop) return fail(SNES_ERR_UNSUPPORTED, kBackdropRefused);
    CHECK(set_device(c));
    { uint32_t cap = window_max() * shard_count; if (cap > (uint32_t)snes::kMaxWindow) cap = snes::kMaxWindow; // a rank scores at most SNES_WINDOW_MAX calls of a window
      if (n_slots > cap) n_slots = cap; }
    CHECK(window_prepare(c, c->nes ? SNES_METHOD_NES : SNES_METHOD_RANDOM));
    CHECK(window_reserve(c, n_slots, 0));
    snesimage_window *w = c->win;
    w->rec[0].seq = w->seq_next++; w->rec[0].base = w->rec[0].seq; // nothing else in flight
    CHECK(window_enqueue(c, w->rec[0], n_slots, seed, first_step_id, palette, index, channel, step, n_random, shard_rank, shard_count, d_errors));
    c->win_pend = true;
    if (n_taken) *n_taken = w->rec[0].K;
    if (stride_out) *stride_out = w->rec[0].stride;
    return SNES_OK;
}

// Phase 2: *consumed calls took effect (the last of them changed the state if *accepted), the rest of the window is void.
// log (host, optional): one record per consumed call.
int32_t snesimage_slots_commit(snesimage_ctx *c, const double *d_errors, uint32_t *consumed, uint32_t *accepted, snesimage_call_result *log) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    snesimage_window *w = c->win;
    if (c->backdrop) return fail(SNES_ERR_UNSUPPORTED, kBackdropRefused);
    if (!w || !c->win_pend) return fail(SNES_ERR_STATE, "slots_commit without slots_begin");
    CHECK(set_device(c));
    c->win_pend = false;
    CHECK(window_enqueue_commit(c, w->rec[0], d_errors, log != nullptr));
    return window_collect(c, w->rec[0], consumed, accepted, log);
}

// The reference's loop for n_calls calls from scheduler state (*palette, *index, *channel, *step), call j drawing its
// random candidates from stream (seed, first_step_id + j): equivalent, bit for bit, to snesimage_schedule_next +
// snesimage_step per call.  window = calls scored per launch set (0: adaptive).
int32_t snesimage_run_slots(snesimage_ctx *c, uint32_t n_calls, uint64_t seed, uint64_t first_step_id, uint32_t *palette, uint32_t *index, uint32_t *channel, uint32_t *step, uint32_t n_random, uint32_t window,
                            snesimage_call_result *log, snesimage_run_stats *stats) {
    if (!c || !palette || !index || !channel || !step) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(check_slot(c, *palette, *index));
    if (*channel > 2) return fail(SNES_ERR_ARG, "bad channel");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending");
    CHECK(set_device(c));
    snesimage_run_stats S{};
    const int nes = c->nes ? 1 : 0;
    uint32_t done = 0, method = 0;
    const bool windows = window_capable(c) && window != 1 && n_random <= 64;
    struct Flight { int rec; uint32_t first, taken, p, i, ch, st; }; // a window in flight and the scheduler state it starts from
    Flight fl[snesimage_window::kRing]; uint32_t nfl = 0; int next_rec = 0; uint32_t win_seq = 0;
    uint32_t q_done = 0, qp = *palette, qi = *index, qch = *channel, qst = *step; // where the next window to enqueue starts if all in flight stay clean
    while (done < n_calls) {
        if (!windows || !c->map_synced || (c->backdrop && nfl == 0 && *palette == c->sub_count)) {
            // One call on its own: configurations the windows do not cover, and a first call that starts from a palette_map
            // which is not optimize() of the palette (it changes the map even if it accepts nothing: lib.rs:237)
            uint32_t p = *palette, i = *index, ch = *channel;
            ctx_schedule_next(c, nes, palette, index, channel, step, &method);
            CHECK(snesimage_step_async(c, method, p, i, ch, seed, first_step_id + done, n_random));
            snes::StepResult r;
            HIPCHK(hipMemcpyAsync(&r, c->d_last, sizeof(r), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (log) { log[done].error = r.error; log[done].best_k = r.best_k; memcpy(log[done].rgb5, r.rgb5, 3); log[done].changed = r.changed; }
            const uint32_t n = method_count(method, n_random);
            S.calls++; S.windows++; S.scored += n; S.useful += n; if (r.changed) S.accepted++;
            done++;
            q_done = done; qp = *palette; qi = *index; qch = *channel; qst = *step;
            continue;
        }
        CHECK(window_reserve(c, window_max(), 0)); // (argument arrays are never regrown while windows are in flight)
        snesimage_window *w = c->win;
        // keep `depth` windows in flight
        // a window ahead only while windows come back clean: behind an acceptance the B phase computed ahead is thrown away
        // (measured right after the k-means start, 23 % acceptance: 0.34 -> 0.28 M useful cand/s with a window always ahead)
        const uint32_t eff_depth = (w->depth > 1 && w->clean_streak >= 2) ? w->depth : 1;
        while (nfl < eff_depth && q_done < n_calls && !(c->backdrop && qp == c->sub_count)) { // (a backdrop call is stepped on its own once the windows in front of it are in)
            uint32_t K = window ? window : w->adapt;
            if (K > n_calls - q_done) K = n_calls - q_done;
            if (K > window_max()) K = window_max();
            const bool ahead = eff_depth > 1;
            if (nfl == 0) {
                CHECK(window_prepare(c, nes ? SNES_METHOD_NES : SNES_METHOD_RANDOM));
                if (ahead && w->use_side) { HIPCHK(hipEventRecord(w->ev_ready, c->stream)); HIPCHK(hipStreamWaitEvent(w->side, w->ev_ready, 0)); } // the palette as the last commit left it, the parent's pack, the flag cleared
            }
            WindowRec &r = w->rec[next_rec];
            r.seq = w->seq_next++; r.base = nfl ? w->rec[fl[0].rec].seq : r.seq; // void once a window in flight before it has accepted
            CHECK(window_enqueue(c, r, K, seed, first_step_id + q_done, qp, qi, qch, qst, n_random, 0, 1, nullptr, ahead ? (int)(win_seq & 1) : 0, ahead));
            win_seq++;
            CHECK(window_enqueue_commit(c, r, nullptr, log != nullptr));
            fl[nfl++] = Flight{next_rec, q_done, r.K, qp, qi, qch, qst};
            next_rec = (next_rec + 1) % snesimage_window::kRing;
            for (uint32_t j = 0; j < r.K; j++) ctx_schedule_next(c, nes, &qp, &qi, &qch, &qst, &method);
            q_done += r.K;
        }
        // the oldest window's result
        const Flight f = fl[0];
        for (uint32_t k = 1; k < nfl; k++) fl[k - 1] = fl[k];
        nfl--;
        WindowRec &r = w->rec[f.rec];
        uint32_t used = 0, acc = 0;
        CHECK(window_collect(c, r, &used, &acc, log ? log + f.first : nullptr));
        *palette = f.p; *index = f.i; *channel = f.ch; *step = f.st;
        for (uint32_t j = 0; j < used; j++) ctx_schedule_next(c, nes, palette, index, channel, step, &method);
        done = f.first + used;
        S.calls += used; S.windows++; S.scored += (uint64_t)f.taken * r.stride; S.useful += (uint64_t)used * r.stride; S.accepted += acc;
        if (acc) { // the windows behind it were built for the old palette: the device has voided them, collect and forget them
            for (uint32_t k = 0; k < nfl; k++) { uint32_t u = 0, a = 0; CHECK(window_collect(c, w->rec[fl[k].rec], &u, &a, nullptr)); S.voided++; }
            nfl = 0;
            q_done = done; qp = *palette; qi = *index; qch = *channel; qst = *step;
        }
        // the next window: twice as long after a clean one, else about the run of calls this one got through
        if (!acc) w->clean_streak++; else w->clean_streak = 0;
        w->adapt = w->policy.next(used, acc, kWindowMin, window_max(), 1, f.taken);
    }
    if (stats) *stats = S;
    return SNES_OK;
}

} // extern "C"
