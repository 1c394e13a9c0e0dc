// snesimage_amd/csrc/ordered_host.inc — ordered dithering: a fixed threshold pattern added to the picture before the
// nearest-colour choice (DESIGN 5d).  NOT a reference mode: the reference dithers by Floyd-Steinberg error diffusion
// (lib.rs:425-501), a serial pass per candidate.  Here each pixel's remap target is orig + d[y % n][x % n], independent of every
// other pixel, so a context with a table runs every path of a context without --dither: the table only decides which image
// the context's d_target / d_labpx_t / d_labpxT_t name (k_build_target's output, or the original itself).
// Included by capi.hip last: the setter reaches into the slot windows and the tile workspace.

namespace {

// nothing of this context may still be reading the buffers that are about to change hands
int32_t ordered_quiesce(snesimage_ctx *c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &L : c->extra) if (L.stream) HIPCHK(hipStreamSynchronize(L.stream));
    if (c->sp.base_stream) HIPCHK(hipStreamSynchronize(c->sp.base_stream));
    for (auto &s : c->sp.h0_stream) if (s) HIPCHK(hipStreamSynchronize(s));
    if (c->win) { if (c->win->side) HIPCHK(hipStreamSynchronize(c->win->side)); if (c->win->aux) HIPCHK(hipStreamSynchronize(c->win->aux)); }
    return SNES_OK;
}

// what snesimage_set_palette_rgb5 invalidates (the palette's tables stay), and everything built from the target: the pack, the
// contested list, the tile workspace's planes, what the slot contexts borrowed.  The source pyramid and Lab(orig) stay valid.
void ordered_invalidate(snesimage_ctx *c) {
    c->pack_valid = false; c->inc_valid = false; c->map_synced = false; c->epoch++; c->epoch_by_commit = false;
    c->sp.plist_valid = false; c->sp.counters_cleared = false;
    if (c->tile) c->tile->planes_ready = false;
    if (c->win)
        for (auto &set : c->win->child)
            for (snesimage_ctx *k : set) {
                k->d_target = c->d_target; k->d_labpx_t = c->d_labpx_t; k->d_labpxT_t = c->d_labpxT_t; k->od_n = c->od_n; memcpy(k->od_tab, c->od_tab, sizeof k->od_tab);
                k->pack_valid = false; k->sp.plist_valid = false; k->sp.counters_cleared = false;
            }
}

// the setter behind its refusals (a set switches its members' tables off through this: shared_level_host.inc)
int32_t ordered_set_body(snesimage_ctx *c, const int8_t *offsets, uint32_t n) {
    CHECK(set_device(c));
    CHECK(ensure_map(c)); // the owed optimize() belongs to the state before this change
    uint8_t *t = nullptr; float *l = nullptr, *lT = nullptr;
    if (n && !c->d_target_own) { // (a failed allocation leaves the context as it was)
        bool ok = dmalloc(&t, c->npx * 4) == hipSuccess;
        if (ok && c->perceptual) ok = dmalloc(&l, c->npx * 3 * 4) == hipSuccess && dmalloc(&lT, c->npx * 3 * 4) == hipSuccess;
        if (!ok) { dfree(t); dfree(l); dfree(lT); return fail(SNES_ERR_HIP, "out of device memory for the target image"); }
    }
    CHECK(ordered_quiesce(c));
    if (t) { c->d_target_own = t; c->d_labpx_t_own = l; c->d_labpxT_t_own = lT; }
    if (n) {
        OrderedTable tab{};
        memcpy(tab.d, offsets, (size_t)n * n);
        hipLaunchKernelGGL(k_build_target, dim3((unsigned)((c->npx / 4 + 255) / 256)), dim3(256), 0, c->stream, c->d_orig, tab, (int)n, c->d_lab_eotf, (int)c->W, (int)c->H, c->d_target_own,
                           c->d_labpx_t_own, c->d_labpxT_t_own);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        memset(c->od_tab, 0, sizeof c->od_tab); memcpy(c->od_tab, offsets, (size_t)n * n);
        c->d_target = c->d_target_own; c->d_labpx_t = c->perceptual ? c->d_labpx_t_own : c->d_labpx; c->d_labpxT_t = c->perceptual ? c->d_labpxT_t_own : c->d_labpxT;
    } else {
        dfree(c->d_target_own); dfree(c->d_labpx_t_own); dfree(c->d_labpxT_t_own);
        memset(c->od_tab, 0, sizeof c->od_tab);
        c->d_target = c->d_orig; c->d_labpx_t = c->d_labpx; c->d_labpxT_t = c->d_labpxT;
    }
    c->od_n = n;
    // a plain table is a bank of one with every tile on it (level_host.inc)
    c->od_L = n ? 1 : 0; memset(c->od_bank, 0, sizeof c->od_bank); memcpy(c->od_bank, c->od_tab, sizeof c->od_tab); memset(c->od_level, 0, sizeof c->od_level);
    if (c->d_level) HIPCHK(hipMemsetAsync(c->d_level, 0, 1024, c->stream));
    ordered_invalidate(c);
    return SNES_OK;
}

} // namespace

extern "C" {

void snesimage_bayer_offsets(uint32_t n, uint32_t amplitude, int8_t *out) {
    if (!out || (n != 2 && n != 4 && n != 8 && n != 16) || amplitude < 1 || amplitude > 255) return;
    const long long den = 2ll * n * n;
    for (uint32_t y = 0; y < n; y++)
        for (uint32_t x = 0; x < n; x++) {
            long long m = 0; // M_2k = [[4M, 4M+2], [4M+3, 4M+1]]: the coarsest quadrant contributes the lowest two bits
            for (uint32_t half = n / 2, scale = 1; half >= 1; half /= 2, scale *= 4) {
                const bool right = (x / half) & 1, low = (y / half) & 1;
                m += (long long)scale * (low ? (right ? 1 : 3) : (right ? 2 : 0));
            }
            const long long num = (long long)amplitude * (2 * m + 1 - (long long)n * n), mag = (2 * (num < 0 ? -num : num) + den) / (2 * den);
            out[y * n + x] = (int8_t)(num < 0 ? -mag : mag);
        }
}

int32_t snesimage_set_ordered_dither(snesimage_ctx *c, const int8_t *offsets, uint32_t n) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (n != 0 && n != 2 && n != 4 && n != 8 && n != 16) return fail(SNES_ERR_ARG, "an ordered-dither table is 2, 4, 8 or 16 offsets wide (0 switches it off)");
    if (n && !offsets) return fail(SNES_ERR_ARG, "null table");
    if (n && c->dither) return fail(SNES_ERR_UNSUPPORTED, "the context was created with SNES_DITHER: error diffusion and ordered dithering are alternatives");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first (its candidates were scored against the current target image)");
    if (c->owner || c->group) return fail(SNES_ERR_STATE, "the context is lent to a batch, a set or a group, whose members share one table: destroy that first");
    return ordered_set_body(c, offsets, n);
}

int32_t snesimage_get_ordered_dither(snesimage_ctx *c, int8_t *out, uint32_t *n) {
    if (!c || !out || !n) return fail(SNES_ERR_ARG, "null pointer");
    if (c->od_L > 1) return fail(SNES_ERR_STATE, "the context holds a bank of several tables: read it with snesimage_get_ordered_dither_bank");
    memcpy(out, c->od_tab, 256); // (zeros behind the n * n offsets)
    *n = c->od_n;
    return SNES_OK;
}

int32_t snesimage_get_target_rgba(snesimage_ctx *c, uint8_t *out) {
    if (!c || !out) return fail(SNES_ERR_ARG, "null pointer");
    CHECK(set_device(c));
    HIPCHK(hipMemcpyAsync(out, c->d_target, c->npx * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

} // extern "C"
