// snesimage_amd/csrc/kernels_import.hpp — the native import: CGRAM, bitplane characters and tilemap words decoded into a state
// (import_host.inc; definition: include/snesimage_hip.h, "Native import").
//
// The inverse of kernels_export.hpp.  Both kernels write STAGING buffers only: the host reads the verdict word after one
// synchronisation and copies palette, tile palettes and maps into the context(s) only when nothing was refused.  Tiles are the
// global tiles g = member * ntile + tile of kernels_char_set.hpp; a single image is a set of one member and passes no table.
// Both kernels are wave64 and take neither scratch nor LDS.
#pragma once
#include "kernels_export.hpp"

namespace snes {

// why a tile was refused; the verdict word is the lowest (g << 8 | reason) over all tiles, kImportOk if none was
enum : unsigned int {
    kImportBelow = 1,     // the character number lies below char_base
    kImportPast = 2,      // ... or past the cells in chr
    kImportPalette = 3,   // the palette field names none of the C rows
    kImportValue = 4,     // a value above S
    kImportOpaqueZero = 5,// value 0 on an opaque pixel of a context without a backdrop colour
    kImportClearValue = 6 // a non-zero value where the source is transparent
};
constexpr unsigned int kImportOk = 0xffffffffu;

// One wave per global tile, lane q the screen pixel (q & 7, q >> 3) of the tile: the word's flips give the cell coordinate, the
// cell's bpp plane bytes of that row the value v (as k_render_native assembles it), v and the source alpha the staged map byte
// at the pixel's place in member m's map (map_out + m * npx).  Lane 0 stages the tile's subpalette.  The character number is
// judged before a cell byte is read, and clamped all the same: the kernel never reads outside chr.  A tile's reasons are
// gathered by ballot — the lowest one counts — and lane 0 alone issues the atomic.
// orig1: the source of a single image (tab == nullptr).  S: the user's subpalette size; backdrop: v == 0 on an opaque pixel is
// the tied entry S.
__global__ __launch_bounds__(64) void k_import_tiles(const SetMember *__restrict__ tab, const uint8_t *__restrict__ orig1, const uint8_t *__restrict__ chr, int nchar,
                                                     const uint16_t *__restrict__ words, int ntile, int W, int npx, int S, int C, int backdrop, NativeLayout L,
                                                     uint8_t *__restrict__ map_out, uint8_t *__restrict__ tp_out, unsigned int *__restrict__ verdict) {
    const int g = blockIdx.x, q = threadIdx.x, m = g / ntile, t = g - m * ntile;
    const uint8_t *orig = tab ? tab[m].orig : orig1;
    const unsigned int word = words[g];
    const int n = (int)(word & 1023u) - L.char_base;
    unsigned int tile_bad = n < 0 ? kImportBelow : (n >= nchar ? kImportPast : 0u); // (the same for the whole wave)
    const bool in_range = tile_bad == 0u;
    int p = 0;
    if (L.bpp != 8) {
        p = (int)((word >> 10) & 7u) - L.palette_base;
        if (p < 0 || p >= C) { tile_bad = tile_bad ? tile_bad : kImportPalette; p = 0; }
    }
    const int ch = n < 0 ? 0 : (n < nchar ? n : nchar - 1);
    const int x = q & 7, y = q >> 3;
    const int fx = (word & 0x4000u) ? 7 - x : x, fy = (word & 0x8000u) ? 7 - y : y;
    unsigned int v = 0;
    if (in_range) {
        const uint8_t *cell = chr + (size_t)ch * (8 * L.bpp);
        for (int k = 0; k < L.bpp / 2; k++) {
            const unsigned int b0 = cell[16 * k + 2 * fy], b1 = cell[16 * k + 2 * fy + 1];
            v |= ((b0 >> (7 - fx)) & 1u) << (2 * k) | ((b1 >> (7 - fx)) & 1u) << (2 * k + 1);
        }
    }
    const int px = tile_px(t, q, W);
    const bool clear = orig[4 * (size_t)px + 3] == 0;
    unsigned int mine = 0; // this pixel's lowest reason
    if (in_range) mine = v > (unsigned)S ? kImportValue : ((v == 0u && !clear && !backdrop) ? kImportOpaqueZero : ((v != 0u && clear) ? kImportClearValue : 0u));
    const unsigned long long b4 = __ballot(mine == kImportValue), b5 = __ballot(mine == kImportOpaqueZero), b6 = __ballot(mine == kImportClearValue);
    const unsigned int pixel_bad = b4 ? kImportValue : (b5 ? kImportOpaqueZero : (b6 ? kImportClearValue : 0u));
    const unsigned int reason = tile_bad ? tile_bad : pixel_bad;
    unsigned int value = 0; // transparent: nothing observable reads it
    if (v != 0u) value = (v <= (unsigned)S ? v : (unsigned)S) - 1u;
    else if (!clear && backdrop) value = (unsigned)S;
    map_out[(size_t)m * npx + px] = (uint8_t)value;
    if (q == 0) {
        tp_out[g] = (uint8_t)p;
        if (reason) atomicMin(verdict, ((unsigned)g << 8) | reason);
    }
}

// CGRAM words -> the staged device palette in the context's layout: entry p * row + i (row = S, or S + 1 with the backdrop
// colour in entry S of every row), three raw 5-bit bytes each, bit 15 dropped.  Entry i < S of row p comes from the word at
// the row's start + 1 + i, the tied entries from word 0 and from nothing else; the rows' first words and the words the
// geometry does not name are not read.  One block of 256 threads, one entry each (a context holds at most 253).
__global__ __launch_bounds__(256) void k_import_cgram(const uint16_t *__restrict__ cgram, int C, int S, int row, NativeLayout L, uint8_t *__restrict__ colors) {
    const int j = threadIdx.x;
    if (j >= C * row) return;
    const int p = j / row, i = j - p * row;
    const int start = L.bpp == 8 ? 0 : (L.palette_base + p) << L.bpp;
    const unsigned int w = cgram[i < S ? (start + 1 + i) & 255 : 0];
    colors[3 * j] = (uint8_t)(w & 31u); colors[3 * j + 1] = (uint8_t)((w >> 5) & 31u); colors[3 * j + 2] = (uint8_t)((w >> 10) & 31u);
}

} // namespace snes
