// snesimage_amd/csrc/kernels_tile.hpp — tile moves scored by the objective (tile_host.inc).
//
// A tile-move candidate is a (tile, subpalette) pair: the image as it stands with that one tile drawn from another
// subpalette, the palette untouched.  Every candidate gets its own palette_map (k_tile_remap, or a whole Floyd-Steinberg
// run with the tile's subpalette overridden: k_dither_tile), and the map-reading scorer of the --dither path takes them in
// one batch.  That scorer resolves a pixel as tile_pal[tile] * sub_size + map[px]; here it is handed a tile table of zeros
// and maps that hold the FULL colour index (<= 252 fits a byte), so the moved tile needs no special case and none of the
// scoring kernels is instantiated anew (k_tile_full writes those maps).  The in-order commit of a window of tile calls is
// k_tile_commit.
#pragma once
#include "kernels.hpp"
#include "kernels_opt.hpp"

namespace snes {

struct TileCall { uint32_t tile, first, count, cur; };                       // candidates [first, first + count) of the window's list, ascending subpalette; cur = the tile's subpalette
struct TileLog { double error; int32_t sub; uint8_t changed; uint8_t pad[3]; }; // = snesimage_tile_result
struct TileWinRes { int32_t consumed, accepted; };                           // calls that took effect; the one that accepted (-1: none)

// per candidate: the tile table with the candidate's tile moved (what its Floyd-Steinberg run reads)
__global__ __launch_bounds__(256) void k_tile_tabs(const uint8_t *__restrict__ tile_pal, const uint16_t *__restrict__ tiles, const uint8_t *__restrict__ subs, uint8_t *__restrict__ tabs) {
    const int cand = blockIdx.x, ct = tiles[cand];
    const uint8_t k = subs[cand];
    for (int i = threadIdx.x; i < 1024; i += 256) tabs[(size_t)cand * 1024 + i] = i == ct ? k : tile_pal[i];
}

struct TileRemapParams {
    const uint8_t *orig, *base_map, *tile_pal; const uint32_t *pal_rgb8; const float *pal_lab, *labpx;
    const uint16_t *tiles; const uint8_t *subs;
    uint8_t *lmaps; // [cand][W*H]: the candidate's palette_map
    int W, H, sub_size, perceptual;
};
// Without dither: the candidate's palette_map is the current one with the tile's 64 pixels remapped to the nearest entry of
// the candidate's subpalette — the search of prep_body (exact integer redmean key or CIEDE2000, strict <: lowest index).
__global__ __launch_bounds__(256) void k_tile_remap(TileRemapParams P) {
    const int cand = blockIdx.x, t = threadIdx.x;
    const int ct = P.tiles[cand], base = (int)P.subs[cand] * P.sub_size;
    const int npx = P.W * P.H;
    uint8_t mine = 0; int px = 0;
    if (t < 64) {
        const int x = (ct & 31) * 8 + (t & 7), y = (ct >> 5) * 8 + (t >> 3);
        px = y * P.W + x;
        const uint32_t o = reinterpret_cast<const uint32_t *>(P.orig)[px];
        if ((o >> 24) != 0) {
            const uint32_t rgb = o & 0x00ffffffu;
            int best = -1;
            if (!P.perceptual) {
                uint32_t bk = 0xffffffffu;
                for (int j = 0; j < P.sub_size; j++) {
                    const uint32_t k = red_mean_key(P.pal_rgb8[base + j], rgb);
                    if (best < 0 || k < bk) { bk = k; best = j; }
                }
            } else {
                Lab tl; tl.l = P.labpx[3 * px]; tl.a = P.labpx[3 * px + 1]; tl.b = P.labpx[3 * px + 2];
                float bd = 0.0f;
                for (int j = 0; j < P.sub_size; j++) {
                    Lab e; e.l = P.pal_lab[3 * (base + j)]; e.a = P.pal_lab[3 * (base + j) + 1]; e.b = P.pal_lab[3 * (base + j) + 2];
                    const float d = ciede2000(e, tl);
                    if (best < 0 || d < bd) { bd = d; best = j; }
                }
            }
            mine = (uint8_t)best;
        }
    }
    const uint4 *src = reinterpret_cast<const uint4 *>(P.base_map);
    uint4 *dst = reinterpret_cast<uint4 *>(P.lmaps + (size_t)cand * npx);
    for (int i = t; i < npx / 16; i += 256) dst[i] = src[i];
    __syncthreads(); // the copy of the tile's rows is in place before its 64 bytes are replaced
    if (t < 64) P.lmaps[(size_t)cand * npx + px] = mine;
}

// palette_map -> full colour indices (sub * sub_size + map, the candidate's tile under its new subpalette), row-major and C4.
// grid (W*H/1024, candidates); a thread takes the four pixels of one word.
__global__ __launch_bounds__(256) void k_tile_full(const uint8_t *__restrict__ lmaps, const uint8_t *__restrict__ tile_pal, const uint16_t *__restrict__ tiles, const uint8_t *__restrict__ subs,
                                                  int W, int H, int sub_size, uint8_t *__restrict__ maps, uint8_t *__restrict__ mapsC4) {
    const int cand = blockIdx.y, w = blockIdx.x * 256 + threadIdx.x; // word index
    if (w >= (W * H) >> 2) return;
    const int px = w << 2, x = px % W, y = px / W;
    const int tile = (x >> 3) + (y >> 3) * (W >> 3);
    const uint32_t sub = tile == (int)tiles[cand] ? (uint32_t)subs[cand] : (uint32_t)tile_pal[tile];
    const size_t cb = (size_t)cand * W * H;
    const uint32_t m = reinterpret_cast<const uint32_t *>(lmaps + cb)[w];
    const uint32_t full = m + sub * (uint32_t)sub_size * 0x01010101u; // every byte stays below 253: no carry
    reinterpret_cast<uint32_t *>(maps + cb)[w] = full;
    reinterpret_cast<uint32_t *>(mapsC4 + cb)[idx_c4(x, y, H) >> 2] = full;
}

// A candidate's whole Floyd-Steinberg run (MODE 0 of kernels_opt.hpp) under its own tile table: block = candidate.
template <bool PERC, int SUB>
__global__ __launch_bounds__(128) void k_dither_tile(DitherParams P, const uint8_t *__restrict__ tabs) {
    P.tile_pal = tabs + (size_t)blockIdx.x * 1024;
    dither_body<PERC, SUB, 0, 128>(P, (int)blockIdx.x);
}
template <int SUB, bool PERC>
__global__ __launch_bounds__(512) void k_dither4_tile(DitherParams P, const uint8_t *__restrict__ tabs) {
    P.tile_pal = tabs + (size_t)blockIdx.x * 1024;
    dither4_body<SUB, 0, PERC>(P, (int)blockIdx.x);
}

// The window's calls in order (lib.rs:216-219 per call: best := incumbent, ascending subpalette, strict <): every call up to
// and including the first that accepts is logged; that one's tile, map and error become the image's.  One block.
__global__ __launch_bounds__(1024) void k_tile_commit(const double *__restrict__ errs, const TileCall *__restrict__ calls, int ncalls, const uint8_t *__restrict__ subs,
                                                     const uint8_t *__restrict__ lmaps, int npx, uint8_t *__restrict__ tile_pal, uint8_t *__restrict__ map, double *__restrict__ inc_err,
                                                     TileLog *__restrict__ log, TileWinRes *__restrict__ res) {
    __shared__ int s_win, s_call;
    if (threadIdx.x == 0) {
        const double inc = *inc_err;
        int win = -1, used = ncalls, acc = -1;
        for (int i = 0; i < ncalls && win < 0; i++) {
            const TileCall c = calls[i];
            double best = inc; int bj = -1;
            for (uint32_t j = c.first; j < c.first + c.count; j++) { const double e = errs[j]; if (e < best) { best = e; bj = (int)j; } }
            TileLog r; r.error = best; r.sub = bj >= 0 ? (int32_t)subs[bj] : (int32_t)c.cur; r.changed = bj >= 0 ? 1 : 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
            log[i] = r;
            if (bj >= 0) { win = bj; acc = i; used = i + 1; }
        }
        res->consumed = used; res->accepted = acc;
        s_win = win; s_call = acc;
    }
    __syncthreads(); // the records are written before the state changes hands
    const int win = s_win;
    if (win < 0) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(lmaps + (size_t)win * npx);
    uint4 *dst = reinterpret_cast<uint4 *>(map);
    for (int i = threadIdx.x; i < npx / 16; i += 1024) dst[i] = src[i];
    if (threadIdx.x == 0) { tile_pal[calls[s_call].tile] = subs[win]; *inc_err = errs[win]; }
}

} // namespace snes
