// snesimage_amd/csrc/kernels_export.hpp — the native export: CGRAM, bitplane characters, tilemap words, and the renderer that
// reads them back as the PPU's background fetch does (export_host.inc; definition: include/snesimage_hip.h, "Native export").
//
// Everything is read from what the character budget leaves on the device: chars, rep and flip of k_char_build / k_char_classes
// (or their set-wide kin), tile_palettes and the palette.  Tiles are the global tiles g = member * ntile + tile of
// kernels_char_set.hpp; a single image is a set of one member.  All kernels are wave64 and take no scratch; only the renderer
// uses LDS (CGRAM, 512 bytes).
#pragma once
#include "kernels_char_set.hpp"

namespace snes {

// the layout as the kernels take it: bpp resolved (2, 4 or 8), the bases checked by the host
struct NativeLayout { int bpp, palette_base, priority, char_base; };

// pos[g] = the number of class representatives below g, for G <= kSetTiles: a representative's position in CHR.
// One block of 1024 threads, eight consecutive tiles per thread; the threads' counts are scanned per wave by shuffles, the
// sixteen wave totals through LDS.
__global__ __launch_bounds__(1024) void k_export_pos(const uint16_t *__restrict__ rep, int G, uint16_t *__restrict__ pos) {
    __shared__ unsigned int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int flags = 0, mine = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int g = tid * 8 + i;
        const bool is_rep = g < G && (int)rep[g < G ? g : 0] == g;
        flags |= is_rep ? 1u << i : 0u;
        mine += is_rep ? 1u : 0u;
    }
    unsigned int incl = mine; // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned int v = __shfl_up(incl, o, 64); incl += lane >= o ? v : 0u; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned int before = incl - mine;
    for (int w = 0; w < wave; w++) before += s_wave[w];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int g = tid * 8 + i;
        if (g < G) pos[g] = (uint16_t)before;
        before += (flags >> i) & 1u;
    }
}

// CGRAM: 256 words, one thread each.  colors: the context's raw 5-bit triples, entry p * row + i (row = S, or S + 1 with the
// backdrop colour B in entry S of every row).  Word 0 and every row's first word hold B (0 without a backdrop), entry i of
// row p sits at the row's start + 1 + i, everything else is 0.  At 8bpp the one row starts at word 0.
__global__ __launch_bounds__(256) void k_export_cgram(const uint8_t *__restrict__ colors, int C, int S, int row, int backdrop, NativeLayout L, uint16_t *__restrict__ cgram) {
    const int w = threadIdx.x;
    const int shift = L.bpp == 8 ? 8 : L.bpp;
    const int p = (w >> shift) - (L.bpp == 8 ? 0 : L.palette_base), i = w & ((1 << shift) - 1);
    const uint16_t b16 = backdrop ? rgb5_as_u16(colors[3 * S], colors[3 * S + 1], colors[3 * S + 2]) : (uint16_t)0;
    uint16_t v = 0;
    if (w == 0) v = b16;
    if (p >= 0 && p < C) {
        if (i == 0) v = b16;
        else if (i <= S) { const uint8_t *c = colors + 3 * (p * row + i - 1); v = rgb5_as_u16(c[0], c[1], c[2]); }
    }
    cgram[w] = v;
}

// CHR: the cell of every class representative at its position, 8 * bpp bytes.  grid = global tiles, block = one wave; a tile
// that is not its class's representative returns at once.  Lane q holds the value at (x, y) = (7 - (q & 7), q >> 3), so the
// ballot of bit p of the values is the eight row bytes of plane p in the hardware's bit order: row y is (mask >> 8y) & 255.
// Lane l < 8 * bpp stores byte l of the cell: plane pair l >> 4, row (l & 15) >> 1, plane 2 * (l >> 4) + (l & 1).
__global__ __launch_bounds__(64) void k_export_chr(const uint8_t *__restrict__ chars, const uint16_t *__restrict__ rep, const uint16_t *__restrict__ pos, int bpp, uint8_t *__restrict__ chr) {
    const int g = blockIdx.x, q = threadIdx.x;
    if ((int)rep[g] != g) return; // (the same for the whole wave)
    const unsigned int v = chars[(size_t)g * 64 + (q >> 3) * 8 + (7 - (q & 7))];
    const int plane = 2 * (q >> 4) + (q & 1), y = (q & 15) >> 1;
    unsigned long long mine = 0;
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const unsigned long long mask = __ballot((v >> p) & 1u);
        mine = plane == p ? mask : mine;
    }
    if (q < 8 * bpp) chr[(size_t)pos[g] * (8 * bpp) + q] = (uint8_t)((mine >> (8 * y)) & 255ull);
}

// MAP: one word per global tile, member after member: pos of the tile's representative, the subpalette (0 at 8bpp: the
// word's palette bits select nothing there), the priority, the two flips.  tile_palettes come from the members' table of a
// set (tab), or from tile_pal where tab is null (one image).
__global__ __launch_bounds__(256) void k_export_map(const SetMember *__restrict__ tab, const uint8_t *__restrict__ tile_pal, int ntile, int G, const uint16_t *__restrict__ rep,
                                                   const uint8_t *__restrict__ flip, const uint16_t *__restrict__ pos, NativeLayout L, uint16_t *__restrict__ map) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int m = g / ntile, t = g - m * ntile;
    int r = rep[g];
    r = r < G ? r : 0; // (k_char_classes writes rep[g] <= g)
    const unsigned int f = flip[g];
    const uint8_t *tp = tab ? tab[m].tile_pal : tile_pal;
    const unsigned int pal = L.bpp == 8 ? 0u : (unsigned)(L.palette_base + (int)tp[t]) & 7u;
    map[g] = (uint16_t)(((unsigned)(L.char_base + (int)pos[r]) & 1023u) | (pal << 10) | ((unsigned)L.priority << 13) | ((f & 1u) << 14) | (((f >> 1) & 1u) << 15));
}

// The background fetch: for every pixel the tilemap word, the flips, the plane bytes of its row, the index, CGRAM, the 5 -> 8
// bit expansion; alpha 255.  Index 0 reads CGRAM word 0 whatever the word's palette.  block 256 (a row of a 256-wide
// picture), grid = pixels / 256; CGRAM in LDS.  nchar: the cells in chr — the host has checked every word against it, the
// kernel clamps all the same and so never reads outside chr.
__global__ __launch_bounds__(256) void k_render_native(const uint16_t *__restrict__ cgram, const uint8_t *__restrict__ chr, int nchar, const uint16_t *__restrict__ map, NativeLayout L, int W, int npx,
                                                      uint8_t *__restrict__ rgba) {
    __shared__ uint16_t s_cgram[256];
    s_cgram[threadIdx.x] = cgram[threadIdx.x];
    __syncthreads();
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= npx) return;
    const int x = px % W, y = px / W;
    const unsigned int word = map[(y >> 3) * 32 + (x >> 3)];
    int ch = (int)(word & 1023u) - L.char_base;
    ch = ch < 0 ? 0 : (ch < nchar ? ch : nchar - 1);
    const int fx = (word & 0x4000u) ? 7 - (x & 7) : (x & 7), fy = (word & 0x8000u) ? 7 - (y & 7) : (y & 7);
    const uint8_t *cell = chr + (size_t)ch * (8 * L.bpp);
    unsigned int idx = 0;
    for (int k = 0; k < L.bpp / 2; k++) {
        const unsigned int b0 = cell[16 * k + 2 * fy], b1 = cell[16 * k + 2 * fy + 1];
        idx |= ((b0 >> (7 - fx)) & 1u) << (2 * k) | ((b1 >> (7 - fx)) & 1u) << (2 * k + 1);
    }
    const unsigned int at = idx == 0 ? 0u : (L.bpp == 8 ? idx : ((((word >> 10) & 7u) << L.bpp) + idx));
    const unsigned int c = s_cgram[at & 255u];
    const uint32_t v = rgb5_to_rgb8(c & 31u, (c >> 5) & 31u, (c >> 10) & 31u) | 0xff000000u;
    reinterpret_cast<uint32_t *>(rgba)[px] = v;
}

} // namespace snes
