// snesimage_amd/csrc/batch_host.inc — many images, one launch per stage of an optimizer call (kernels_batch.hpp).
// Included by capi.hip after the single-image host code, whose helpers it reuses.  A batch borrows its contexts: it
// enqueues their optimizer calls on its own stream and keeps their cache flags consistent; any call on a member
// context first waits for the batch's stream (set_device -> batch_quiesce).

struct snesimage_batch {
    std::vector<snesimage_ctx *> ctx;
    int device = 0;
    hipStream_t stream = nullptr;
    static constexpr int kRing = 4; // argument blocks in flight (the host runs ahead of the device by up to kRing calls)
    snes::BatchArgs *h_args[kRing] = {nullptr, nullptr, nullptr, nullptr}, *d_args[kRing] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t used[kRing] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t calls = 0;
    bool busy = false, dead = false; // dead: a member context was destroyed under the batch
};

namespace {

int32_t batch_quiesce(snesimage_batch *b) {
    if (b && b->busy) { HIPCHK(hipStreamSynchronize(b->stream)); b->busy = false; }
    return SNES_OK;
}

snes::PrepParams make_prep(snesimage_ctx *c, int mode, int sp, int si) {
    snes::PrepParams P{};
    P.orig = c->d_target; P.tile_pal = c->d_tile_pal; P.pal_rgb8 = c->d_pal_rgb8; P.map = c->d_map; P.pack = c->d_pack; P.packT = c->d_packT; P.packC4 = c->d_packC4; P.packR4 = c->d_packR4;
    P.subC4 = c->d_subC4; P.subR4 = c->d_subR4; P.labpx = c->d_labpx_t; P.pal_lab = c->d_pal_lab;
    P.W = (int)c->W; P.H = (int)c->H; P.sub_size = (int)c->sub_size; P.ncol = c->ncol; P.mode = mode; P.sp = sp; P.si = si; P.perceptual = c->perceptual ? 1 : 0;
    return P;
}

// Arguments of one member's optimizer call on slot (palette, index): candidates in the member's storage lane 0, B in its own.
int32_t fill_batch_args(snes::BatchArgs &a, snesimage_ctx *c, uint32_t n, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel, unsigned long long key) {
    // the member's storage holds sp.cap candidates (and its list d_cand as many as cand_cap): more would be written past them on the device
    if (n == 0 || n > c->sp.cap) return fail(SNES_ERR_STATE, "a batched call of " + std::to_string(n) + " candidates on a context whose storage holds " + std::to_string(c->sp.cap));
    if (c->dither) c->sp.slot_ci = palette * c->sub_size + index;
    a.Pc = sparse_params(c, 0); a.Pc.is_base = 0; a.Pc.ncand = (int)n; a.Pc.k0 = 0; a.Pc.order = c->sp.lpt ? c->sp.order : nullptr;
    a.Pb = sparse_params(c, c->nlanes); a.Pb.is_base = 1; a.Pb.ncand = 1; a.Pb.k0 = a.Pb.base;
    a.prep = make_prep(c, 2, (int)palette, (int)index);
    a.prep.zero = c->sp.plist_count; a.prep.nzero = 1; // the slot's contested-pixel count (B's work items are published once: sparse_alloc)
    a.key = key;
    a.colors_in = c->d_colors; a.colors = c->d_colors; a.cand = c->d_cand; a.eotf = c->d_eotf; a.cand_tab = c->sp.cand_tab;
    a.part = c->sp.part; a.errors = c->d_errs; a.inc_err = c->d_inc_err; a.last = c->d_last;
    a.T.eotf = c->d_eotf; a.T.lab_eotf = c->d_lab_eotf; a.T.rgb8 = c->d_pal_rgb8; a.T.lin = c->d_pal_lin; a.T.xyb = c->d_pal_xyb; a.T.lab = c->perceptual ? c->d_pal_lab : nullptr;
    a.lab_eotf = c->d_lab_eotf; a.cand_lab = c->sp.cand_lab;
    a.dead_base = 0; a.win_pack = nullptr; a.bcolor = nullptr; a.btab = nullptr; a.zero = nullptr; a.nzero = 0; a.Db = DitherParams{}; a.Dc = DitherParams{}; a.map = c->d_map;
    if (c->dither) { // (the caller has set c->sp.slot_ci, which sparse_params hands to the bodies)
        auto &sp = c->sp;
        const uint32_t j0 = c->sub_size > 1 ? (index + 1u) % c->sub_size : index;
        a.bcolor = c->d_colors + 3 * (size_t)(palette * c->sub_size + j0); a.btab = sp.cand_tab + 8 * (size_t)(sp.lanes * sp.cap);
        a.win_pack = sp.dpack; a.zero = sp.plist_count; a.nzero = 1;
        DitherParams D{};
        D.orig = c->d_orig; D.tile_pal = c->d_tile_pal; D.pal_rgb8 = c->d_pal_rgb8; D.W = (int)c->W; D.H = (int)c->H; D.sub_size = (int)c->sub_size; D.ncol = c->ncol; D.slot_ci = sp.slot_ci;
        a.Db = D; a.Db.cand_tab = a.btab; a.Db.maps = sp.bmap; a.Db.mapsC4 = sp.bmapC4; a.Db.rec_pack = sp.dpack; a.Db.ck_out = sp.ckd;
        a.Db.excl_sub = (int)palette; a.Db.excl_si = (int)index; a.Db.excl_j0 = (int)j0;
        a.Dc = D; a.Dc.cand_tab = sp.cand_tab; a.Dc.maps = const_cast<uint8_t *>(a.Pc.maps); a.Dc.mapsC4 = const_cast<uint8_t *>(a.Pc.mapsC4);
        a.Dc.first_group = sp.first; a.Dc.first_k0 = 0; a.Dc.rec_in = c->dither_rec ? sp.dpack : nullptr; a.Dc.ck_in = sp.ckd; a.Dc.bmap = sp.bmap; a.Dc.bmapC4 = sp.bmapC4; a.Dc.order = sp.lpt ? sp.order : nullptr;
        if (c->perceptual) { // CIEDE2000: the stand-in's Lab in B's row of the candidates' Lab table, B's record in distance bits, the targets' Lab beside it
            a.Db.pal_lab = c->d_pal_lab; a.Db.cand_lab = sp.cand_lab + 3 * (size_t)(sp.lanes * sp.cap); a.Db.lab_eotf = c->d_lab_eotf; a.Db.perceptual = 1; a.Db.rec_lab = sp.rec_lab;
            a.Dc.pal_lab = c->d_pal_lab; a.Dc.cand_lab = sp.cand_lab; a.Dc.lab_eotf = c->d_lab_eotf; a.Dc.perceptual = 1;
        }
    }
    a.method = (int)method; a.n = (int)n; a.slot = (int)(palette * c->sub_size + index); a.channel = (int)channel; a.nes = method == SNES_METHOD_NES ? 1 : 0; a.npx = (int)c->npx;
    return SNES_OK;
}

// The scoring launches of one optimizer call for K members at once (blockIdx.z = member; the members' arguments sit in
// the device array A): pack of the slot, base image B, the candidates' group-sparse pipeline, errors.  The candidate
// lists must already be (or be about to be, earlier on `st`) in place.  Shared by the image batches and the slot windows.
// With a side stream B's H and V sweeps — single-image chains, a few waves per member — run there, beside the candidates'
// scan and downscale (which need B's linear rows only); the candidates' H pass waits for B's H checkpoints, their V pass
// for B's V checkpoints, their narrow-scale V pass for B's narrow sweeps.
struct BatchSide { hipStream_t stream; hipEvent_t in, h, v, narrow; bool whole; hipStream_t aux = nullptr; hipEvent_t a_scan = nullptr, a_h0 = nullptr, a_v0 = nullptr; }; // aux (slot windows): scale 0's H and V passes of a long window on a stream of their own, beside the downscale and the other scales (as sparse_score_chunk does) // // whole: the side stream runs the members' whole B phase — pack, contested list, B's downscale and sweeps — and none of it looks at `dead` (slot windows: it belongs to the NEXT window and runs beside the current one's candidates)
int32_t enqueue_batched_scoring(hipStream_t st, const snes::BatchArgs *A, uint32_t K, uint32_t n, snesimage_ctx *c0, const BatchSide *side = nullptr, const int *dead = nullptr, bool member_packs = false) {
    const Geom &G = c0->G;
    const unsigned npx_blocks = (unsigned)((c0->npx + 255) / 256);
    const int s_first = sparse_params(c0, 0).s_first; // first narrow scale: the wide ones run the bodies of kernels_sparse2.hpp
    hipStream_t bs = side && side->stream ? side->stream : st;
    const bool split = bs != st;
    const bool dith = c0->dither;
    const bool sub16 = c0->sub_size == 16; // (15 + the backdrop)
    const bool sub15 = c0->sub_size == 15; // the 15-colour subpalettes of the SNES 4bpp modes get a fully unrolled entry search
    const bool whole = split && side->whole;
    hipStream_t ps = whole ? bs : st;              // stream of the pack, the contested list and B's downscale
    const int *bdead = whole ? nullptr : dead;     // (see BatchSide::whole)
    if (!dith) hipLaunchKernelGGL(kb_prep, dim3(npx_blocks, 1, K), dim3(256), 0, ps, A, bdead);                 // pack of the slot; clears B's counters
    else { // --dither: the pack is mode 1 (transparency marker and stored map) — the parent's for the calls of a slot window, every image's own (member_packs) in an image batch; B is the image dithered with the slot's entry out of play
        if (member_packs) hipLaunchKernelGGL(kb_prep, dim3(npx_blocks, 1, K), dim3(256), 0, ps, A, bdead);
        hipLaunchKernelGGL(kb_dither_prep, dim3(1, 1, K), dim3(64), 0, ps, A, bdead);
        if (c0->perceptual) hipLaunchKernelGGL(kb_dither_base_lab, dim3(1, 1, K), dim3(512), 0, ps, A, bdead);
        else if (sub15) hipLaunchKernelGGL(kb_dither_base<15>, dim3(1, 1, K), dim3(512), 0, ps, A, bdead);
        else if (sub16) hipLaunchKernelGGL(kb_dither_base<16>, dim3(1, 1, K), dim3(512), 0, ps, A, bdead);
        else hipLaunchKernelGGL(kb_dither_base<0>, dim3(1, 1, K), dim3(512), 0, ps, A, bdead);
    }
    hipLaunchKernelGGL(kb_build_plist, dim3(npx_blocks, 1, K), dim3(256), 0, ps, A, bdead);
    hipLaunchKernelGGL(kb_base_down, dim3(down_grid(G), 1, K), dim3(256), 0, ps, A, bdead);
    if (split) { HIPCHK(hipEventRecord(side->in, ps)); HIPCHK(hipStreamWaitEvent(whole ? st : bs, side->in, 0)); } // the other stream goes on from here
    // (B's work items are in place since every member's sparse_alloc)
    const bool quad = (size_t)n * K <= c0->sp.h2q_max; // few candidates in all: the H passes with a quad of lanes per row (as score_list does for short lists)
    if (quad) hipLaunchKernelGGL(kb_sparse_h2q_base, dim3((unsigned)((G.sh[0] / 4 * 3 + 3) / 4), (unsigned)(s_first * kColBuckets), K), dim3(64), h2_lds(c0), bs, A, bdead);
    else hipLaunchKernelGGL(kb_sparse_h2_base, dim3((unsigned)((G.sh[0] / 4 * 3 + 15) / 16), (unsigned)(s_first * kColBuckets), K), dim3(64), h2_lds(c0), bs, A, bdead);
    if (split) HIPCHK(hipEventRecord(side->h, bs));
    if (s_first > 0 && c0->sp.vsplit) hipLaunchKernelGGL(kb_sparse_v_base_split, dim3((unsigned)(G.W >> 6), (unsigned)(3 * s_first), K), dim3(128), 0, bs, A, bdead); // recurrences | maps and sums on two waves per 64 columns
    else if (s_first > 0) hipLaunchKernelGGL(kb_sparse_v_base, dim3(3, (unsigned)s_first, K), dim3(256), 0, bs, A, bdead);
    if (split) HIPCHK(hipEventRecord(side->v, bs));
    if (s_first < G.nscales) hipLaunchKernelGGL(kb_sparse_h, dim3((unsigned)((G.sh[s_first] / 4 * 3 + 15) / 16), (unsigned)((G.nscales - s_first) * kColBuckets), K), dim3(64), 0, bs, A, 1, bdead);
    if (s_first < G.nscales) hipLaunchKernelGGL(kb_sparse_v_base_narrow, dim3(3, (unsigned)(G.nscales - s_first), K), dim3(256), 0, bs, A, bdead);
    if (split) HIPCHK(hipEventRecord(side->narrow, bs));
    if (c0->sp.debug_poison) hipLaunchKernelGGL(kb_poison_store, dim3(256, 1, K), dim3(256), 0, st, A, dead); // SNES_DEBUG_POISON: ahead of everything the call's candidates write
    hipLaunchKernelGGL(kb_candidate_tables, dim3((n + 63) / 64, 1, K), dim3(64), 0, st, A, dead);
    if (dith && c0->perceptual) { // --dither --perceptual-palettes: as below with the CIEDE2000 kernels
        hipLaunchKernelGGL(kb_candidate_lab, dim3((n + 63) / 64, 1, K), dim3(64), 0, st, A, dead);
        hipLaunchKernelGGL(kb_dither_first_lab, dim3(n, 1, K), dim3(256), 0, st, A, dead);
        if (c0->sp.lpt) hipLaunchKernelGGL(kb_sparse_order, dim3(1, 1, K), dim3(1024), 0, st, A, dead);
        if (c0->dither4 && (size_t)n * K <= c0->dither4_max) hipLaunchKernelGGL(kb_dither_run4_lab, dim3(n, 1, K), dim3(512), 0, st, A, dead);
        else hipLaunchKernelGGL(kb_dither_run_lab, dim3(n, 1, K), dim3(128), 0, st, A, dead);
        hipLaunchKernelGGL(kb_dither_diff, dim3((n + 3) / 4, 1, K), dim3(1024), 0, st, A, dead);
    } else
    if (c0->perceptual) { // CIEDE2000 win tests once per contested pixel into the candidates' bitmaps
        hipLaunchKernelGGL(kb_candidate_lab, dim3((n + 63) / 64, 1, K), dim3(64), 0, st, A, dead);
        hipLaunchKernelGGL(kb_clear_bitmaps, dim3(64, 1, K), dim3(256), 0, st, A, dead);
        hipLaunchKernelGGL(kb_sparse_scan_lab, dim3(n, 1, K), dim3(256), 0, st, A, dead);
    } else if (dith) { // first pixel each candidate takes from B, its own Floyd-Steinberg run from that 4-row group on (longest first), what changed
        hipLaunchKernelGGL(kb_dither_first, dim3((n + 15) / 16, 1, K), dim3(1024), 0, st, A, dead);
        if (c0->sp.lpt) hipLaunchKernelGGL(kb_sparse_order, dim3(1, 1, K), dim3(1024), 0, st, A, dead);
        const bool quad_fs = c0->dither4 && (size_t)n * K <= c0->dither4_max;
        if (quad_fs && sub15) hipLaunchKernelGGL(kb_dither_run4<15>, dim3(n, 1, K), dim3(512), 0, st, A, dead);
        else if (quad_fs && sub16) hipLaunchKernelGGL(kb_dither_run4<16>, dim3(n, 1, K), dim3(512), 0, st, A, dead);
        else if (quad_fs) hipLaunchKernelGGL(kb_dither_run4<0>, dim3(n, 1, K), dim3(512), 0, st, A, dead);
        else if (c0->ditherw && sub15) hipLaunchKernelGGL(kb_dither_runw<15>, dim3((n + 3) / 4, 1, K), dim3(256), 0, st, A, dead);
        else if (c0->ditherw && sub16) hipLaunchKernelGGL(kb_dither_runw<16>, dim3((n + 3) / 4, 1, K), dim3(256), 0, st, A, dead);
        else if (c0->ditherw && c0->sub_size > 1) hipLaunchKernelGGL(kb_dither_runw<0>, dim3((n + 3) / 4, 1, K), dim3(256), 0, st, A, dead);
        else if (sub15) hipLaunchKernelGGL(kb_dither_run<15>, dim3(n, 1, K), dim3(128), 0, st, A, dead);
        else if (sub16) hipLaunchKernelGGL(kb_dither_run<16>, dim3(n, 1, K), dim3(128), 0, st, A, dead);
        else hipLaunchKernelGGL(kb_dither_run<0>, dim3(n, 1, K), dim3(128), 0, st, A, dead);
        hipLaunchKernelGGL(kb_dither_diff, dim3((n + 3) / 4, 1, K), dim3(1024), 0, st, A, dead);
    } else if ((size_t)n * K <= c0->sp.scan4_max) hipLaunchKernelGGL(kb_sparse_scan4, dim3((n + 3) / 4, 1, K), dim3(1024), 0, st, A, dead);
    else hipLaunchKernelGGL(kb_sparse_scan, dim3((n + 15) / 16, 1, K), dim3(1024), 0, st, A, 0, dead);
    const bool two = side && side->aux && !quad && (size_t)n * K >= c0->sp.h0_min && c0->sp.h0_min > 0 && s_first > 0 && c0->sp.down1 && G.nscales > 2;
    if (two) { // scale 0: H pass (it reads the pack and B's checkpoints, not the downscale), the V pass's order, V pass
        hipStream_t ax = side->aux;
        HIPCHK(hipEventRecord(side->a_scan, st)); HIPCHK(hipStreamWaitEvent(ax, side->a_scan, 0));
        if (split) HIPCHK(hipStreamWaitEvent(ax, side->h, 0));
        size_t gx = ((size_t)n * 8 * 3 + 15) / 16; if (gx > c0->sp.hgrid) gx = c0->sp.hgrid; if (gx < 8) gx = 8;
        hipLaunchKernelGGL(kb_sparse_h2_lists, dim3((unsigned)gx, (unsigned)kColBuckets, K), dim3(64), h2_lds(c0), ax, A, dead, 0);
        if (c0->sp.lpt) hipLaunchKernelGGL(kb_sparse_order, dim3(1, 1, K), dim3(1024), 0, ax, A, dead);
        HIPCHK(hipEventRecord(side->a_h0, ax));
        if (split) HIPCHK(hipStreamWaitEvent(ax, side->v, 0));
        hipLaunchKernelGGL(kb_sparse_v2_scales, dim3(n * 3, 1, K), dim3(256), 0, ax, A, dead, 0);
        HIPCHK(hipEventRecord(side->a_v0, ax));
    }
    if (c0->sp.down1 && G.nscales > 2) { // scale 1 one block per changed group, then the scales that depend on each other
        hipLaunchKernelGGL(kb_sparse_down1, dim3(n * 8, 1, K), dim3(256), 0, st, A, dead);
        if (c0->sp.down_tiles && G.nscales >= 4) {
            unsigned gt = (n * (unsigned)(G.sh[3] / 4) + SNES_DOWN_TILES_U - 1) / SNES_DOWN_TILES_U; if (gt > c0->sp.tiles_grid) gt = c0->sp.tiles_grid;
            hipLaunchKernelGGL(kb_sparse_down_tiles, dim3(gt, 1, K), dim3(256), 0, st, A, dead);
        } else
        hipLaunchKernelGGL(kb_sparse_down, dim3(n, 1, K), dim3(256), 0, st, A, -2, dead);
    } else hipLaunchKernelGGL(kb_sparse_down, dim3(n, 1, K), dim3(256), 0, st, A, 0, dead);
    if (split) HIPCHK(hipStreamWaitEvent(st, side->h, 0));
    // grid-stride over the item quads of each (image, list); the lists hold a tenth of the worst case on average and there
    // are K images x 12 lists of them: a grid sized for the worst case is mostly blocks that find nothing to do
    { size_t gx = ((size_t)n * 8 * 3 + 15) / 16; if (gx > c0->sp.hgrid) gx = c0->sp.hgrid; if (gx < 8) gx = 8;
      if (quad) hipLaunchKernelGGL(kb_sparse_h2q, dim3((unsigned)(gx * 4), (unsigned)(s_first * kColBuckets), K), dim3(64), h2_lds(c0), st, A, dead);
      else if (two && (c0->sp.h_forms & 1)) { if (s_first > 1) hipLaunchKernelGGL(kb_sparse_h2_from, dim3((unsigned)gx, (unsigned)((s_first - 1) * kColBuckets), K), dim3(64), h2_lds(c0), st, A, dead, (int)kColBuckets); }
      else if (two) { if (s_first > 1) hipLaunchKernelGGL(kb_sparse_h2_lists, dim3((unsigned)gx, (unsigned)((s_first - 1) * kColBuckets), K), dim3(64), h2_lds(c0), st, A, dead, (int)kColBuckets); }
      else hipLaunchKernelGGL(kb_sparse_h2, dim3((unsigned)gx, (unsigned)(s_first * kColBuckets), K), dim3(64), h2_lds(c0), st, A, dead);
      if (s_first < G.nscales) hipLaunchKernelGGL(kb_sparse_h, dim3((unsigned)((gx + 7) / 8), (unsigned)((G.nscales - s_first) * kColBuckets), K), dim3(64), 0, st, A, 0, dead); }
    if (two) { // the order comes from the other stream; the narrow scales first (latency-bound: not alone at the end), then scales 1..
        HIPCHK(hipStreamWaitEvent(st, side->a_h0, 0));
        if (split) { HIPCHK(hipStreamWaitEvent(st, side->v, 0)); HIPCHK(hipStreamWaitEvent(st, side->narrow, 0)); }
        if (s_first < G.nscales) hipLaunchKernelGGL(kb_sparse_v, dim3((n * 3 + 7) / 8, (unsigned)(G.nscales - s_first), K), dim3(256), 0, st, A, dead);
        if (s_first > 1) hipLaunchKernelGGL(kb_sparse_v2_scales, dim3(n * 3, (unsigned)(s_first - 1), K), dim3(256), 0, st, A, dead, 1);
        HIPCHK(hipStreamWaitEvent(st, side->a_v0, 0));
    } else {
    if (c0->sp.lpt) hipLaunchKernelGGL(kb_sparse_order, dim3(1, 1, K), dim3(1024), 0, st, A, dead); // longest column sweeps first
    if (split) HIPCHK(hipStreamWaitEvent(st, side->v, 0));
    hipLaunchKernelGGL(kb_sparse_v2, dim3(n * 3, (unsigned)s_first, K), dim3(256), 0, st, A, dead);
    if (split) HIPCHK(hipStreamWaitEvent(st, side->narrow, 0));
    if (s_first < G.nscales) hipLaunchKernelGGL(kb_sparse_v, dim3((n * 3 + 7) / 8, (unsigned)(G.nscales - s_first), K), dim3(256), 0, st, A, dead);
    }
    hipLaunchKernelGGL(kb_final_score, dim3((n + 3) / 4, 1, K), dim3(256), 0, st, A, dead);        // a wave per candidate; also clears the candidates' counters
    HIPCHK(hipGetLastError());
    return SNES_OK;
}

} // namespace

extern "C" {

// a member context is being destroyed while lent out: finish the batch's work and refuse further calls
void batch_forget(snesimage_batch *b, snesimage_ctx *c) {
    (void)batch_quiesce(b);
    for (auto *m : b->ctx) m->owner = nullptr;
    (void)c;
    b->dead = true;
}

} // extern "C"

namespace {
// snesimage_batch_create; backdrop_ok: the members may be SNES_BACKDROP contexts (a backdrop set, shared_host.inc, whose host
// carries the backdrop schedule: the batched launches only ever see the regular slots of the expanded contexts)
int32_t batch_create_members(snesimage_ctx **ctxs, uint32_t n, snesimage_batch **out, bool backdrop_ok) {
    if (!ctxs || !out || n == 0) return fail(SNES_ERR_ARG, "null pointer or empty batch");
    *out = nullptr;
    snesimage_ctx *c0 = ctxs[0];
    for (uint32_t i = 0; i < n; i++) {
        snesimage_ctx *c = ctxs[i];
        if (!c) return fail(SNES_ERR_ARG, "null context in batch");
        if (c->owner) return fail(SNES_ERR_STATE, "context already belongs to a batch");
        if (c->backdrop && !backdrop_ok) return fail(SNES_ERR_UNSUPPORTED, kBackdropRefused);
        if (c->od_L > 1) return fail(SNES_ERR_ARG, kLevelsRefused);
        if (blocked(c)) return fail(SNES_ERR_UNSUPPORTED, kBlockedRefused);
        if (c->device != c0->device || c->W != c0->W || c->H != c0->H || c->sub_count != c0->sub_count || c->sub_size != c0->sub_size || c->chunk != c0->chunk)
            return fail(SNES_ERR_ARG, "contexts of a batch must share device, image size, palette geometry and chunk");
        if (c->perceptual != c0->perceptual) return fail(SNES_ERR_ARG, "contexts of a batch must share their flags");
        if (!c->sp.enabled || (c->dither && c->sub_size == 1)) return fail(SNES_ERR_UNSUPPORTED, "batched calls cover the group-sparse path (not with SNES_SPARSE=0), and with --dither subpalettes of two entries and more");
        if (c->dither != c0->dither) return fail(SNES_ERR_ARG, "contexts of a batch must share their flags");
        if (!ordered_tables_equal(c, c0)) return fail(SNES_ERR_ARG, "contexts of a batch must share their ordered-dither table");
    }
    std::unique_ptr<snesimage_batch> b(new snesimage_batch());
    b->device = c0->device;
    HIPCHK(hipSetDevice(b->device));
    for (uint32_t i = 0; i < n; i++) { // everything a steady-state call takes for granted, enqueued on every image's own stream ...
        snesimage_ctx *c = ctxs[i];
        CHECK(alloc_workspace(c, 1));
        CHECK(ensure_tables(c));
        CHECK(ensure_source(c));
        CHECK(sparse_alloc(c, c->chunk)); // a batched call is one launch group per image: up to `chunk` candidates
        CHECK(ensure_cand_capacity(c, c->chunk));
        if (!c->map_synced) CHECK(do_optimize(c));
        CHECK(ensure_incumbent(c));
    }
    for (uint32_t i = 0; i < n; i++) HIPCHK(hipStreamSynchronize(ctxs[i]->stream)); // ... then awaited: the images' set-up work overlaps
    HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    for (int r = 0; r < snesimage_batch::kRing; r++) {
        HIPCHK(hipHostMalloc(&b->h_args[r], sizeof(snes::BatchArgs) * n));
        HIPCHK(hipMalloc(&b->d_args[r], sizeof(snes::BatchArgs) * n));
        HIPCHK(hipEventCreateWithFlags(&b->used[r], hipEventDisableTiming));
    }
    b->ctx.assign(ctxs, ctxs + n);
    for (auto *c : b->ctx) c->owner = b.get();
    *out = b.release();
    return SNES_OK;
}
} // namespace

extern "C" {

int32_t snesimage_batch_create(snesimage_ctx **ctxs, uint32_t n, snesimage_batch **out) { return batch_create_members(ctxs, n, out, false); }

void snesimage_batch_destroy(snesimage_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (!b->dead) for (auto *c : b->ctx) c->owner = nullptr;
    for (int r = 0; r < snesimage_batch::kRing; r++) {
        if (b->h_args[r]) (void)hipHostFree(b->h_args[r]);
        if (b->d_args[r]) (void)hipFree(b->d_args[r]);
        if (b->used[r]) (void)hipEventDestroy(b->used[r]);
    }
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int32_t snesimage_batch_sync(snesimage_batch *b) {
    if (!b) return fail(SNES_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    return batch_quiesce(b);
}

} // extern "C"

namespace {

// The launches of one optimizer call for every member of b, on the batch's stream: member i's candidate stream keyed
// (seeds[i], step_id).  joint == nullptr: every member commits its own call (kb_commit); otherwise the members share one
// palette (a set, shared_host.inc) and ks_commit decides once for all of them, its record going to *joint.
// gen: a generator in kb_gen_candidates' place (a set's guided call, shared_guide_host.inc): it enqueues on the batch's stream
// whatever writes the call's n candidates into every member's list; a call without one issues the launches it always did.
struct BatchGen { int32_t (*enqueue)(void *self, hipStream_t st, uint32_t palette, uint32_t index, uint32_t n); void *self; };
int32_t batch_call(snesimage_batch *b, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel, const uint64_t *seeds, uint64_t step_id, uint32_t n_random, snes::StepResult *joint,
                   const BatchGen *gen = nullptr) {
    snesimage_ctx *c0 = b->ctx[0];
    CHECK(check_slot(c0, palette, index));
    if (method > 2 || channel > 2) return fail(SNES_ERR_ARG, "bad method or channel");
    const uint32_t n = method_count(method, n_random);
    if (n > c0->chunk) return fail(SNES_ERR_ARG, "a batched call holds at most `chunk` candidates per image");
    HIPCHK(hipSetDevice(b->device));
    const uint32_t K = (uint32_t)b->ctx.size();
    const int r = (int)(b->calls % snesimage_batch::kRing);
    if (b->calls >= (uint64_t)snesimage_batch::kRing) HIPCHK(hipEventSynchronize(b->used[r])); // the device is done with this argument block
    snes::BatchArgs *ha = b->h_args[r];
    for (uint32_t i = 0; i < K; i++) {
        snesimage_ctx *c = b->ctx[i];
        if (!c->tables_valid || !c->src_valid || !c->inc_valid) return fail(SNES_ERR_STATE, "a member context was modified outside the batch; call snesimage_batch_sync and recreate the batch");
        CHECK(fill_batch_args(ha[i], c, n, method, palette, index, channel, mix64(seeds[i] ^ (step_id * 0x9E3779B97F4A7C15ull) ^ 0xD1B54A32D192ED03ull)));
        if (n > c->cand_cap) return fail(SNES_ERR_STATE, "a member's candidate list is smaller than the call");
        if (c->dither) { ha[i].prep = make_prep(c, 1, -1, -1); ha[i].prep.zero = nullptr; ha[i].prep.nzero = 0; } // the pack of the stored map (kb_dither_prep clears the counters)
    }
    hipStream_t st = b->stream;
    // Work a member queued on its own stream since the last batched call (snesimage_step_async, score_candidates_device:
    // they leave the cache flags valid) touches the same pack, palette and sparse storage: order the batch behind it.
    if (!b->busy) for (auto *c : b->ctx) {
        if (!c->ev_own) HIPCHK(hipEventCreateWithFlags(&c->ev_own, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_own, c->stream));
        HIPCHK(hipStreamWaitEvent(st, c->ev_own, 0));
    }
    const snes::BatchArgs *A = b->d_args[r];
    HIPCHK(hipMemcpyAsync(b->d_args[r], ha, sizeof(snes::BatchArgs) * K, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(b->used[r], st));
    if (gen) CHECK(gen->enqueue(gen->self, st, palette, index, n));
    else hipLaunchKernelGGL(kb_gen_candidates, dim3((n + 63) / 64, 1, K), dim3(64), 0, st, A, (const int *)nullptr);
    CHECK(enqueue_batched_scoring(st, A, K, n, c0, nullptr, nullptr, c0->dither)); // (one stream: with 128 images' working sets the second stream of the slot windows costs 12 %)
    if (joint) hipLaunchKernelGGL(ks_commit, dim3(1), dim3(256), 0, st, A, (int)K, joint);
    else hipLaunchKernelGGL(kb_commit, dim3(1, 1, K), dim3(256), 0, st, A, (const int *)nullptr);
    if (c0->dither) hipLaunchKernelGGL(kb_take_map, dim3(1, 1, K), dim3(1024), 0, st, A, (const int *)nullptr);
    HIPCHK(hipGetLastError());
    for (auto *c : b->ctx) { // what snesimage_step_async leaves behind in a context
        c->pack_valid = false; c->sp.plist_valid = false; c->sp.counters_cleared = false; c->epoch++; c->epoch_by_commit = false;
        c->map_pending = !c->dither; c->map_synced = true; c->inc_valid = true; c->best_valid = false;
    }
    b->calls++;
    b->busy = true;
    return SNES_OK;
}

} // namespace

extern "C" {

// snesimage_step_async for every image of the batch, slot and method shared, candidate streams keyed (seeds[i], step_id).
int32_t snesimage_batch_step_async(snesimage_batch *b, uint32_t method, uint32_t palette, uint32_t index, uint32_t channel, const uint64_t *seeds, uint64_t step_id, uint32_t n_random) {
    if (!b || !seeds) return fail(SNES_ERR_ARG, "null pointer");
    if (b->dead) return fail(SNES_ERR_STATE, "a member context of this batch was destroyed");
    return batch_call(b, method, palette, index, channel, seeds, step_id, n_random, nullptr);
}

} // extern "C"
