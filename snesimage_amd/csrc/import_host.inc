// snesimage_amd/csrc/import_host.inc — the native import: snesimage_import_native and snesimage_shared_import_native
// (definition: include/snesimage_hip.h, "Native import"; kernels: kernels_import.hpp).
//
// All or nothing.  CGRAM, CHR and MAP go to the device, k_import_cgram and k_import_tiles decode them into STAGING buffers on
// the context's (the set's) stream, and the verdict word comes back with the call's one synchronisation.  Only an accepted
// import touches a context: palette, tile palettes [0, ntile) and map are then copied device-to-device, and the flags say what
// the four setters would have left — a stored map of unknown error, tables, packs and incumbent invalid, the epoch advanced,
// a pending optimize() dropped.  A refusal has changed nothing: no optimize() owed was run, no flag was written.
// The staging buffers live for the call.  Included by capi.hip behind export_host.inc (it uses export_layout).

namespace {

// the call's device buffers; freed when the call returns, however it returns
struct ImportWork {
    uint16_t *cgram = nullptr, *words = nullptr; uint8_t *chr = nullptr, *map = nullptr, *tp = nullptr, *colors = nullptr; unsigned int *verdict = nullptr; snes::SetMember *tab = nullptr;
    ~ImportWork() { dfree(cgram); dfree(words); dfree(chr); dfree(map); dfree(tp); dfree(colors); dfree(verdict); dfree(tab); }
    int32_t alloc(uint32_t G, uint32_t F, size_t npx, uint64_t chr_bytes, int ncol, bool table) {
        HIPCHK(dmalloc(&cgram, 512)); HIPCHK(dmalloc(&words, sizeof(uint16_t) * G)); HIPCHK(dmalloc(&chr, (size_t)chr_bytes)); HIPCHK(dmalloc(&map, npx * F)); HIPCHK(dmalloc(&tp, G));
        HIPCHK(dmalloc(&colors, 3 * (size_t)ncol)); HIPCHK(dmalloc(&verdict, sizeof(unsigned int)));
        if (table) HIPCHK(dmalloc(&tab, sizeof(snes::SetMember) * F));
        return SNES_OK;
    }
};

// the cells in chr, or the refusal of a ragged or empty or oversized chr
int32_t import_cells(const snes::NativeLayout &L, uint64_t chr_bytes, uint32_t *nchar) {
    const uint32_t cell = 8u * (uint32_t)L.bpp;
    const uint64_t n = chr_bytes / cell;
    if (n == 0 || chr_bytes % cell || n > 1024) return fail(SNES_ERR_ARG, "chr_bytes is not between 1 and 1024 characters of " + std::to_string(cell) + " bytes");
    *nchar = (uint32_t)n;
    return SNES_OK;
}

// The refusal a verdict word stands for.  where: "tile 5", or "tile 5 of member 1".
int32_t import_refusal(unsigned int verdict, const std::string &where, unsigned int word, const snes::NativeLayout &L, uint32_t nchar, uint32_t S, uint32_t C) {
    const std::string head = "native import: " + where + " (tilemap word " + std::to_string(word) + ") ";
    switch (verdict & 255u) {
    case snes::kImportBelow: return fail(SNES_ERR_ARG, head + "names character " + std::to_string(word & 1023u) + ", below char_base " + std::to_string(L.char_base));
    case snes::kImportPast: return fail(SNES_ERR_ARG, head + "names character " + std::to_string(word & 1023u) + ", past the " + std::to_string(nchar) + " characters at char_base " + std::to_string(L.char_base));
    case snes::kImportPalette: return fail(SNES_ERR_ARG, head + "selects palette " + std::to_string((word >> 10) & 7u) + ", outside the " + std::to_string(C) + " subpalettes at palette_base " + std::to_string(L.palette_base));
    case snes::kImportValue: return fail(SNES_ERR_ARG, head + "draws a character value above " + std::to_string(S) + ", the subpalette size");
    case snes::kImportOpaqueZero: return fail(SNES_ERR_ARG, head + "draws value 0 on an opaque pixel: only the backdrop colour shows there — create the context with SNES_BACKDROP to import such data");
    case snes::kImportClearValue: return fail(SNES_ERR_ARG, head + "draws a colour where the source is transparent: the library cannot draw it");
    }
    return fail(SNES_ERR_HIP, "native import: bad verdict");
}

// Everything up to the verdict, on stream st: the pieces to the device, the two kernels, one synchronisation.  c0: the context
// whose geometry is decoded for; h_tab: the members of a set (F of them), or null for c0 alone.  w keeps the staged state.
int32_t import_stage(snesimage_ctx *c0, hipStream_t st, const snes::NativeLayout &L, const snes::SetMember *h_tab, uint32_t F, const uint8_t *cgram, const uint8_t *chr, uint64_t chr_bytes,
                     uint32_t nchar, const uint16_t *words, ImportWork &w, unsigned int *verdict) {
    const uint32_t ntile = char_ntile(c0), G = F * ntile;
    CHECK(w.alloc(G, F, c0->npx, chr_bytes, c0->ncol, h_tab != nullptr));
    HIPCHK(hipMemcpyAsync(w.cgram, cgram, 512, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.chr, chr, (size_t)chr_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.words, words, sizeof(uint16_t) * G, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(w.verdict, 0xff, sizeof(unsigned int), st)); // kImportOk
    if (h_tab) HIPCHK(hipMemcpyAsync(w.tab, h_tab, sizeof(snes::SetMember) * F, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_import_cgram, dim3(1), dim3(256), 0, st, (const uint16_t *)w.cgram, (int)c0->sub_count, (int)c0->user_size, (int)c0->sub_size, L, w.colors);
    hipLaunchKernelGGL(k_import_tiles, dim3(G), dim3(64), 0, st, (const snes::SetMember *)w.tab, (const uint8_t *)c0->d_orig, (const uint8_t *)w.chr, (int)nchar, (const uint16_t *)w.words, (int)ntile,
                       (int)c0->W, (int)c0->npx, (int)c0->user_size, (int)c0->sub_count, c0->backdrop ? 1 : 0, L, w.map, w.tp, w.verdict);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(verdict, w.verdict, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one synchronisation before anything is touched
    return SNES_OK;
}

// member m of the staged state into context c (enqueued on st), and what the four setters would have left in its flags
int32_t import_apply(snesimage_ctx *c, hipStream_t st, const ImportWork &w, uint32_t m) {
    const uint32_t ntile = char_ntile(c);
    HIPCHK(hipMemcpyAsync(c->d_colors, w.colors, 3 * (size_t)c->ncol, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(c->d_tile_pal, w.tp + (size_t)m * ntile, ntile, hipMemcpyDeviceToDevice, st)); // (the entries below the image stay)
    HIPCHK(hipMemcpyAsync(c->d_map, w.map + (size_t)m * c->npx, c->npx, hipMemcpyDeviceToDevice, st));
    c->map_pending = false; // replaced wholesale, as snesimage_set_palette_map drops it
    c->tables_valid = false; c->pack_valid = false; c->sp.plist_valid = false; c->inc_valid = false; c->map_synced = false; c->best_valid = false; c->epoch++; c->epoch_by_commit = false;
    return SNES_OK;
}

void import_info(snesimage_native_info *info, const snes::NativeLayout &L, uint32_t nchar, uint64_t chr_bytes, uint32_t G) {
    if (info) { info->bpp = (uint32_t)L.bpp; info->unique = nchar; info->chr_bytes = (uint32_t)chr_bytes; info->map_words = G; }
}

} // namespace

extern "C" {

int32_t snesimage_import_native(snesimage_ctx *c, const snesimage_native_layout *layout, const uint8_t *cgram, const uint8_t *chr, uint64_t chr_bytes, const uint16_t *map, snesimage_native_info *info) {
    CHECK(char_check(c));
    if (blocked(c)) return fail(SNES_ERR_UNSUPPORTED, "snesimage_import_native: the context holds palette blocks (snesimage_set_palette_blocks) and native data carries a palette per tile; set 1 x 1 blocks first");
    if (!cgram || !chr || !map) return fail(SNES_ERR_ARG, "null pointer");
    snes::NativeLayout L{};
    CHECK(export_layout(layout, c->user_size, c->sub_count, &L));
    uint32_t nchar = 0;
    CHECK(import_cells(L, chr_bytes, &nchar));
    CHECK(set_device(c));
    const uint32_t ntile = char_ntile(c);
    unsigned int verdict = snes::kImportOk;
    ImportWork w;
    CHECK(import_stage(c, c->stream, L, nullptr, 1, cgram, chr, chr_bytes, nchar, map, w, &verdict));
    if (verdict != snes::kImportOk) {
        const uint32_t t = verdict >> 8;
        if (t >= ntile) return fail(SNES_ERR_HIP, "native import: bad verdict");
        return import_refusal(verdict, "tile " + std::to_string(t), map[t], L, nchar, c->user_size, c->sub_count);
    }
    CHECK(import_apply(c, c->stream, w, 0));
    HIPCHK(hipStreamSynchronize(c->stream)); // the staging buffers go with the call
    import_info(info, L, nchar, chr_bytes, ntile);
    return SNES_OK;
}

int32_t snesimage_shared_import_native(snesimage_shared *s, const snesimage_native_layout *layout, const uint8_t *cgram, const uint8_t *chr, uint64_t chr_bytes, const uint16_t *maps,
                                       snesimage_native_info *info) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_import_native"));
    CHECK(sc_check(s));
    if (!cgram || !chr || !maps) return fail(SNES_ERR_ARG, "null pointer");
    auto &M = members(s);
    snesimage_ctx *c0 = M[0];
    snes::NativeLayout L{};
    CHECK(export_layout(layout, c0->user_size, c0->sub_count, &L));
    uint32_t nchar = 0;
    CHECK(import_cells(L, chr_bytes, &nchar));
    CHECK(shared_enter(s, true, true)); // the set intact and its stream idle; the members' maps are about to be replaced, not read
    for (auto *c : M) HIPCHK(hipStreamSynchronize(c->stream));
    const uint32_t F = (uint32_t)M.size(), ntile = sc_ntile(s);
    std::vector<snes::SetMember> tab(F);
    for (uint32_t i = 0; i < F; i++) tab[i] = snes::SetMember{M[i]->d_orig, M[i]->d_map, M[i]->d_tile_pal, M[i]->d_inc_err, nullptr, nullptr};
    hipStream_t st = s->b->stream;
    unsigned int verdict = snes::kImportOk;
    ImportWork w;
    CHECK(import_stage(c0, st, L, tab.data(), F, cgram, chr, chr_bytes, nchar, maps, w, &verdict));
    if (verdict != snes::kImportOk) { // one verdict for all members, before any member is touched
        const uint32_t g = verdict >> 8;
        if (g >= F * ntile) return fail(SNES_ERR_HIP, "native import: bad verdict");
        return import_refusal(verdict, "tile " + std::to_string(g % ntile) + " of member " + std::to_string(g / ntile), maps[g], L, nchar, c0->user_size, c0->sub_count);
    }
    // What an accepted snesimage_shared_reduce_characters leaves: stored maps in the members, their new epochs recorded — the
    // set stays intact — and the set knows it holds maps that are no optimize() of the palette.  E is unknown.
    for (uint32_t i = 0; i < F; i++) { CHECK(import_apply(M[i], st, w, i)); s->epoch[i] = M[i]->epoch; }
    s->reduced = true;
    HIPCHK(hipStreamSynchronize(st)); // the staging buffers go with the call
    import_info(info, L, nchar, chr_bytes, F * ntile);
    return SNES_OK;
}

} // extern "C"
