// snesimage_amd/csrc/export_host.inc — the native export: snesimage_export_native, snesimage_shared_export_native and
// snesimage_render_native (definition: include/snesimage_hip.h, "Native export"; kernels: kernels_export.hpp).
//
// An export works as snesimage_characters does — characters and classes are recomputed from the stored map — and then packs
// CGRAM, CHR and MAP on the same stream.  U decides the size of CHR and whether char_base + U fits the tilemap word, and U is
// known only on the device: so the pieces are packed into buffers sized for the worst case, read back with CharInfo, and
// checked and handed over after the call's one synchronisation.  The buffers live for the call; nothing is kept in the
// context or the set, and no other entry point has anything to invalidate.
// The renderer takes bytes from anywhere: it reads the context's size, device and stream, and nothing else of it.
// Included by capi.hip behind char_host.inc and shared_char_host.inc.

namespace {

static_assert(sizeof(snesimage_native_layout) == 8 && sizeof(snesimage_native_info) == 16, "the layout of the export's structs");

// the call's device buffers; freed when the call returns, however it returns
struct ExportWork {
    uint16_t *pos = nullptr, *map = nullptr, *cgram = nullptr; uint8_t *chr = nullptr;
    ~ExportWork() { dfree(pos); dfree(map); dfree(cgram); dfree(chr); }
    int32_t alloc(uint32_t G, uint32_t bpp) {
        HIPCHK(dmalloc(&pos, sizeof(uint16_t) * G)); HIPCHK(dmalloc(&map, sizeof(uint16_t) * G)); HIPCHK(dmalloc(&cgram, 512)); HIPCHK(dmalloc(&chr, 8 * (size_t)bpp * G));
        return SNES_OK;
    }
};

// The layout checked and its depth resolved for subpalettes of S entries; count > 0: the export's conditions on `count`
// subpalettes as well (the renderer judges bytes from anywhere and passes 0).
int32_t export_layout(const snesimage_native_layout *in, uint32_t S, uint32_t count, snes::NativeLayout *L) {
    const snesimage_native_layout z{};
    const snesimage_native_layout &l = in ? *in : z;
    if (l.bpp != 0 && l.bpp != 2 && l.bpp != 4 && l.bpp != 8) return fail(SNES_ERR_ARG, "the depth of a native export is 0 (auto), 2, 4 or 8 bits per pixel");
    if (l.palette_base > 7 || l.priority > 1 || l.char_base > 1023) return fail(SNES_ERR_ARG, "native layout out of range: palette_base is 0..7, priority 0 or 1, char_base 0..1023");
    const uint32_t bpp = l.bpp ? l.bpp : (S <= 3 ? 2u : (S <= 15 ? 4u : 8u));
    if (count) {
        if (S > (1u << bpp) - 1) return fail(SNES_ERR_ARG, std::to_string(bpp) + "bpp characters hold values up to " + std::to_string((1u << bpp) - 1) + ": subpalettes of " + std::to_string(S) + " colours do not fit");
        if (bpp == 8 && (count != 1 || l.palette_base != 0))
            return fail(SNES_ERR_UNSUPPORTED, "an 8bpp export takes one subpalette at palette_base 0 (this geometry: " + std::to_string(count) + " subpalettes of " + std::to_string(S) +
                                              " colours, palette_base " + std::to_string((unsigned)l.palette_base) + "): the 8bpp tilemap word's palette bits do not select among 256-colour palettes");
        if (bpp != 8 && l.palette_base + count > 8) return fail(SNES_ERR_ARG, "palette_base + sub_count exceeds the 8 palettes a tilemap word selects (" + std::to_string((unsigned)l.palette_base) + " + " + std::to_string(count) + ")");
    }
    L->bpp = (int)bpp; L->palette_base = l.palette_base; L->priority = l.priority; L->char_base = l.char_base;
    return SNES_OK;
}

// Behind the classes (rep, flip, chars and info on the device, stream st): pack what was asked for, read it back with U,
// synchronise once, check and hand over.  c0: the context whose palette is exported; G = F * ntile global tiles.
int32_t export_finish(snesimage_ctx *c0, hipStream_t st, const snes::NativeLayout &L, const snes::SetMember *tab, const uint8_t *tile_pal, uint32_t ntile, uint32_t G, const uint8_t *chars,
                      const uint16_t *rep, const uint8_t *flip, const snes::CharInfo *d_info, const char *budget_calls, uint8_t *cgram, uint8_t *chr, uint64_t chr_cap, uint16_t *map,
                      snesimage_native_info *info) {
    const uint32_t cell = 8u * (uint32_t)L.bpp;
    std::vector<uint8_t> h_chr(chr ? (size_t)cell * G : 0), h_cgram(cgram ? 512 : 0);
    std::vector<uint16_t> h_map(map ? G : 0);
    snes::CharInfo ci{};
    ExportWork w; // (declared behind the host buffers: released, and with that the device idle, before they go)
    CHECK(w.alloc(G, (uint32_t)L.bpp));
    hipLaunchKernelGGL(k_export_pos, dim3(1), dim3(1024), 0, st, rep, (int)G, w.pos);
    if (cgram) hipLaunchKernelGGL(k_export_cgram, dim3(1), dim3(256), 0, st, (const uint8_t *)c0->d_colors, (int)c0->sub_count, (int)c0->user_size, (int)c0->sub_size, c0->backdrop ? 1 : 0, L, w.cgram);
    if (chr) hipLaunchKernelGGL(k_export_chr, dim3(G), dim3(64), 0, st, chars, rep, (const uint16_t *)w.pos, L.bpp, w.chr);
    if (map) hipLaunchKernelGGL(k_export_map, dim3((G + 255) / 256), dim3(256), 0, st, tab, tile_pal, (int)ntile, (int)G, rep, flip, (const uint16_t *)w.pos, L, w.map);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&ci, d_info, sizeof(ci), hipMemcpyDeviceToHost, st));
    if (cgram) HIPCHK(hipMemcpyAsync(h_cgram.data(), w.cgram, 512, hipMemcpyDeviceToHost, st));
    if (chr) HIPCHK(hipMemcpyAsync(h_chr.data(), w.chr, h_chr.size(), hipMemcpyDeviceToHost, st)); // (behind the U cells: never written, never handed over)
    if (map) HIPCHK(hipMemcpyAsync(h_map.data(), w.map, sizeof(uint16_t) * G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one synchronisation of the call
    const uint32_t U = ci.unique;
    if (U < 1 || U > G) return fail(SNES_ERR_HIP, "native export: bad character count");
    if ((uint32_t)L.char_base + U > 1024)
        return fail(SNES_ERR_ARG, "char_base + U exceeds the 1024 characters a tilemap word addresses: U = " + std::to_string(U) + " at char_base " + std::to_string(L.char_base) + " (lower U with " + budget_calls + ")");
    const uint64_t chr_bytes = (uint64_t)cell * U;
    if (chr && chr_cap < chr_bytes) return fail(SNES_ERR_ARG, "chr holds " + std::to_string(chr_cap) + " bytes, the characters take " + std::to_string(chr_bytes));
    if (cgram) memcpy(cgram, h_cgram.data(), 512);
    if (chr) memcpy(chr, h_chr.data(), (size_t)chr_bytes);
    if (map) memcpy(map, h_map.data(), sizeof(uint16_t) * G);
    if (info) { info->bpp = (uint32_t)L.bpp; info->unique = U; info->chr_bytes = (uint32_t)chr_bytes; info->map_words = G; }
    return SNES_OK;
}

} // namespace

extern "C" {

int32_t snesimage_export_native(snesimage_ctx *c, const snesimage_native_layout *layout, uint8_t *cgram, uint8_t *chr, uint64_t chr_cap, uint16_t *map, snesimage_native_info *info) {
    CHECK(char_check(c));
    snes::NativeLayout L{};
    CHECK(export_layout(layout, c->user_size, c->sub_count, &L));
    CHECK(set_device(c));
    CHECK(ensure_map(c)); // an optimize() still owed belongs to the state that is asked about
    CHECK(char_alloc(c));
    CHECK(char_classes(c));
    snesimage_charwork &w = *c->chr;
    const uint32_t ntile = char_ntile(c);
    return export_finish(c, c->stream, L, nullptr, c->d_tile_pal, ntile, ntile, w.chars, w.rep, w.flip, w.info, "snesimage_reduce_characters or snesimage_refit_characters", cgram, chr, chr_cap, map, info);
}

int32_t snesimage_shared_export_native(snesimage_shared *s, const snesimage_native_layout *layout, uint8_t *cgram, uint8_t *chr, uint64_t chr_cap, uint16_t *maps, snesimage_native_info *info) {
    CHECK(shared_refuse_backdrop(s, "snesimage_shared_export_native"));
    CHECK(sc_check(s));
    snesimage_ctx *c0 = members(s)[0];
    snes::NativeLayout L{};
    CHECK(export_layout(layout, c0->user_size, c0->sub_count, &L));
    CHECK(sc_enter(s, false));
    CHECK(sc_alloc(s));
    CHECK(sc_table(s, false));
    CHECK(sc_classes(s));
    snesimage_sharedchar &w = *s->chr;
    return export_finish(c0, s->b->stream, L, w.tab, nullptr, sc_ntile(s), w.G, w.chars, w.rep, w.flip, w.info, "snesimage_shared_reduce_characters or snesimage_shared_refit_characters", cgram, chr, chr_cap, maps,
                         info);
}

int32_t snesimage_render_native(snesimage_ctx *c, const snesimage_native_layout *layout, const uint8_t *cgram, const uint8_t *chr, uint64_t chr_bytes, const uint16_t *map, uint8_t *rgba) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    if (!cgram || !chr || !map || !rgba) return fail(SNES_ERR_ARG, "null pointer");
    snes::NativeLayout L{};
    CHECK(export_layout(layout, c->user_size, 0, &L));
    const uint32_t ntile = char_ntile(c), cell = 8u * (uint32_t)L.bpp;
    const uint64_t nchar = chr_bytes / cell;
    if (nchar == 0 || chr_bytes % cell || nchar > 1024) return fail(SNES_ERR_ARG, "chr_bytes is not between 1 and 1024 characters of " + std::to_string(cell) + " bytes");
    for (uint32_t t = 0; t < ntile; t++) { // before any launch: the kernel never reads outside chr
        const uint32_t n = map[t] & 1023u;
        if (n < (uint32_t)L.char_base || n - (uint32_t)L.char_base >= nchar)
            return fail(SNES_ERR_ARG, "tilemap word " + std::to_string(t) + " names character " + std::to_string(n) + ": outside the " + std::to_string(nchar) + " characters at char_base " + std::to_string(L.char_base));
    }
    HIPCHK(hipSetDevice(c->device));
    struct Work { uint16_t *cgram = nullptr, *map = nullptr; uint8_t *chr = nullptr, *rgba = nullptr; ~Work() { dfree(cgram); dfree(map); dfree(chr); dfree(rgba); } } w;
    HIPCHK(dmalloc(&w.cgram, 512)); HIPCHK(dmalloc(&w.map, sizeof(uint16_t) * ntile)); HIPCHK(dmalloc(&w.chr, (size_t)chr_bytes)); HIPCHK(dmalloc(&w.rgba, c->npx * 4));
    HIPCHK(hipMemcpyAsync(w.cgram, cgram, 512, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(w.map, map, sizeof(uint16_t) * ntile, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(w.chr, chr, (size_t)chr_bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_render_native, dim3((unsigned)((c->npx + 255) / 256)), dim3(256), 0, c->stream, (const uint16_t *)w.cgram, (const uint8_t *)w.chr, (int)nchar, (const uint16_t *)w.map, L, (int)c->W,
                       (int)c->npx, w.rgba);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rgba, w.rgba, c->npx * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

} // extern "C"
