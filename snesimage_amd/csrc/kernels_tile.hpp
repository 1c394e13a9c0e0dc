// snesimage_amd/csrc/kernels_tile.hpp — tile, block and level moves scored by the objective: the move family (tile_host.inc,
// block_host.inc, level_host.inc; DESIGN 4b''').
//
// A move candidate is a (block, subpalette) pair: the image as it stands with every tile of that block drawn from another
// subpalette, the palette untouched.  Blocks are bw x bh tiles with bw, bh in {1, 2, 4, 8}, passed as their logarithms
// (lbw, lbh); the image is 32 tiles wide, so block b = by * (32 >> lbw) + bx covers tiles tx >> lbw == bx, ty >> lbh == by.
// A tile move is the move of a 1 x 1 block: at lbw == lbh == 0 a block is a tile, and the tile entry points run these kernels.
// Every candidate gets its own palette_map (k_move_remap, or a whole Floyd-Steinberg run under the candidate's tile table:
// k_dither_tile), and the map-reading scorer of the --dither path takes them in one batch.  That scorer resolves a pixel as
// tile_pal[tile] * sub_size + map[px]; here it is handed a tile table of zeros and maps that hold the FULL colour index
// (<= 252 fits a byte), so the moved tiles need no special case and none of the scoring kernels is instantiated anew
// (k_move_full writes those maps).  The in-order commit of a window of calls is k_move_commit.
// Three device functions are shared with the level moves (kernels_level.hpp): nearest_entry (the search of every candidate
// remap), window_decide (the in-order decision of a window) and copy_map / copy_map_sync (kernels.hpp).
#pragma once
#include "kernels.hpp"
#include "kernels_opt.hpp"

namespace snes {

struct TileCall { uint32_t tile, first, count, cur; };                       // candidates [first, first + count) of the window's list, ascending option; tile = the call's tile or block, cur = its option now
struct TileLog { double error; int32_t sub; uint8_t changed; uint8_t pad[3]; }; // = snesimage_tile_result
struct TileWinRes { int32_t consumed, accepted; };                           // calls that took effect; the one that accepted (-1: none)
struct TileWin { int cand, call; };                                          // the candidate that won and its call (-1, -1: none)

// block b = by * nbx + bx with nbx = 32 >> lbw a power of two: bx and by are a mask and a shift
__device__ __forceinline__ int block_bx(int block, int lbw) { return block & ((32 >> lbw) - 1); }
__device__ __forceinline__ int block_by(int block, int lbw) { return block >> (5 - lbw); }
__device__ __forceinline__ bool tile_in_block(int tile, int block, int lbw, int lbh) {
    return ((tile & 31) >> lbw) == block_bx(block, lbw) && ((tile >> 5) >> lbh) == block_by(block, lbw);
}

// The nearest entry of the subpalette at `base` to the target pixel o (RGBA): the search of prep_body — exact integer redmean
// key, or CIEDE2000 against lab_of(), the pixel's Lab, which only an opaque pixel of a perceptual context asks for; strict <,
// so the lowest index wins a tie; 0 under alpha 0.
template <class LabOf>
__device__ __forceinline__ uint32_t nearest_entry(uint32_t o, LabOf lab_of, int perceptual, const uint32_t *__restrict__ pal_rgb8, const float *__restrict__ pal_lab, int base, int sub_size) {
    if ((o >> 24) == 0) return 0u;
    const uint32_t rgb = o & 0x00ffffffu;
    int best = -1;
    if (!perceptual) {
        uint32_t bk = 0xffffffffu;
        for (int j = 0; j < sub_size; j++) {
            const uint32_t k = red_mean_key(pal_rgb8[base + j], rgb);
            if (best < 0 || k < bk) { bk = k; best = j; }
        }
    } else {
        const Lab tl = lab_of();
        float bd = 0.0f;
        for (int j = 0; j < sub_size; j++) {
            Lab e; e.l = pal_lab[3 * (base + j)]; e.a = pal_lab[3 * (base + j) + 1]; e.b = pal_lab[3 * (base + j) + 2];
            const float d = ciede2000(e, tl);
            if (best < 0 || d < bd) { bd = d; best = j; }
        }
    }
    return (uint32_t)best;
}

// The window's calls in order (lib.rs:216-219 per call: best := incumbent, ascending option, strict <, so a NaN never wins):
// every call up to and including the first that accepts is logged, and the commit record written.  Every thread of the block
// calls it; thread 0 decides, reading the incumbent error from incumbent() and candidate j's from err(j), opts[j] its option;
// the barrier puts the records in front of whatever the caller then changes.  All threads get the winner.
template <class Incumbent, class Err>
__device__ __forceinline__ TileWin window_decide(Incumbent incumbent, Err err, const TileCall *__restrict__ calls, int ncalls, const uint8_t *__restrict__ opts, TileLog *__restrict__ log,
                                                 TileWinRes *__restrict__ res) {
    __shared__ int s_win, s_call;
    if (threadIdx.x == 0) {
        const double inc = incumbent();
        int win = -1, used = ncalls, acc = -1;
        for (int i = 0; i < ncalls && win < 0; i++) {
            const TileCall c = calls[i];
            double best = inc; int bj = -1;
            for (uint32_t j = c.first; j < c.first + c.count; j++) { const double e = err(j); if (e < best) { best = e; bj = (int)j; } }
            TileLog r; r.error = best; r.sub = bj >= 0 ? (int32_t)opts[bj] : (int32_t)c.cur; r.changed = bj >= 0 ? 1 : 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
            log[i] = r;
            if (bj >= 0) { win = bj; acc = i; used = i + 1; }
        }
        res->consumed = used; res->accepted = acc;
        s_win = win; s_call = acc;
    }
    __syncthreads(); // the records are written before the state changes hands
    return TileWin{s_win, s_call};
}

// per candidate: the tile table with the candidate's whole block moved (what its Floyd-Steinberg run reads)
__global__ __launch_bounds__(256) void k_move_tabs(const uint8_t *__restrict__ tile_pal, const uint16_t *__restrict__ blocks, const uint8_t *__restrict__ subs, int lbw, int lbh,
                                                  uint8_t *__restrict__ tabs) {
    const int cand = blockIdx.x, cb = blocks[cand];
    const uint8_t k = subs[cand];
    for (int i = threadIdx.x; i < 1024; i += 256) tabs[(size_t)cand * 1024 + i] = tile_in_block(i, cb, lbw, lbh) ? k : tile_pal[i];
}

struct MoveRemapParams {
    const uint8_t *orig, *base_map; const uint32_t *pal_rgb8; const float *pal_lab, *labpx;
    const uint16_t *blocks; const uint8_t *subs;
    uint8_t *lmaps; // [cand][W*H]: the candidate's palette_map
    int W, H, sub_size, perceptual, lbw, lbh;
};
// Without dither: the candidate's palette_map is the current one with the block's (8 << lbw) x (8 << lbh) pixels, 64 to 4,096,
// remapped to the nearest entry of the candidate's subpalette.  One workgroup per candidate; a thread takes every 256th pixel
// of the block, row by row: one wave and one search per lane for a tile, 16 searches per lane for an 8 x 8 block.
__global__ __launch_bounds__(256) void k_move_remap(MoveRemapParams P) {
    const int cand = blockIdx.x, t = threadIdx.x;
    const int cb = P.blocks[cand], base = (int)P.subs[cand] * P.sub_size;
    const int npx = P.W * P.H;
    const int x0 = block_bx(cb, P.lbw) << (3 + P.lbw), y0 = block_by(cb, P.lbw) << (3 + P.lbh);
    const int lrow = 3 + P.lbw, nblk = 64 << (P.lbw + P.lbh); // pixels per row of the block (log2); pixels of the block
    uint8_t *lmap = P.lmaps + (size_t)cand * npx;
    copy_map_sync<256>(lmap, P.base_map, npx);
    for (int i = t; i < nblk; i += 256) {
        const int y = y0 + (i >> lrow), px = y * P.W + x0 + (i & ((1 << lrow) - 1));
        if (y >= P.H) continue; // (a block never leaves the image: bh divides h/8)
        const uint32_t o = reinterpret_cast<const uint32_t *>(P.orig)[px];
        lmap[px] = (uint8_t)nearest_entry(o, [&]() { Lab tl; tl.l = P.labpx[3 * px]; tl.a = P.labpx[3 * px + 1]; tl.b = P.labpx[3 * px + 2]; return tl; },
                                          P.perceptual, P.pal_rgb8, P.pal_lab, base, P.sub_size);
    }
}

// palette_map -> full colour indices (sub * sub_size + map, the tiles of the candidate's block under its new subpalette),
// row-major and C4.  grid (W*H/1024, candidates); a thread takes the four pixels of one word.  The level moves hand in the
// tile with its own subpalette, which substitutes nothing.
__global__ __launch_bounds__(256) void k_move_full(const uint8_t *__restrict__ lmaps, const uint8_t *__restrict__ tile_pal, const uint16_t *__restrict__ blocks, const uint8_t *__restrict__ subs,
                                                  int W, int H, int sub_size, int lbw, int lbh, uint8_t *__restrict__ maps, uint8_t *__restrict__ mapsC4) {
    const int cand = blockIdx.y, w = blockIdx.x * 256 + threadIdx.x; // word index
    if (w >= (W * H) >> 2) return;
    const int px = w << 2, x = px % W, y = px / W;
    const int tile = (x >> 3) + (y >> 3) * (W >> 3);
    const uint32_t sub = tile_in_block(tile, (int)blocks[cand], lbw, lbh) ? (uint32_t)subs[cand] : (uint32_t)tile_pal[tile];
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

// The window's calls in order (window_decide; TileCall::tile holds the block): the accepting call's block (its
// (1 << lbw) x (1 << lbh) table entries), map and error become the image's.  One block.
__global__ __launch_bounds__(1024) void k_move_commit(const double *__restrict__ errs, const TileCall *__restrict__ calls, int ncalls, const uint8_t *__restrict__ subs,
                                                     const uint8_t *__restrict__ lmaps, int npx, int lbw, int lbh, uint8_t *__restrict__ tile_pal, uint8_t *__restrict__ map,
                                                     double *__restrict__ inc_err, TileLog *__restrict__ log, TileWinRes *__restrict__ res) {
    const TileWin w = window_decide([&]() { return *inc_err; }, [&](uint32_t j) { return errs[j]; }, calls, ncalls, subs, log, res);
    if (w.cand < 0) return;
    copy_map<1024>(map, lmaps + (size_t)w.cand * npx, npx);
    const int cb = (int)calls[w.call].tile, ntb = 1 << (lbw + lbh);
    if ((int)threadIdx.x < ntb) { // the block's tiles, at most 64
        const int tx = (block_bx(cb, lbw) << lbw) + ((int)threadIdx.x & ((1 << lbw) - 1)), ty = (block_by(cb, lbw) << lbh) + ((int)threadIdx.x >> lbw);
        tile_pal[ty * 32 + tx] = subs[w.cand];
    }
    if (threadIdx.x == 0) *inc_err = errs[w.cand];
}

// per-unit f32 sums in the reference's order with the block in place of the tile (lib.rs:91-116): the block's pixels x outer,
// y inner, one ordered chain per block
__global__ void k_unit_sums(const uint8_t *__restrict__ orig, const float *__restrict__ labpx, int W, int H, int perceptual, int lbw, int lbh, float *__restrict__ sums /*[blocks][3]*/,
                            int *__restrict__ counts) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int nbx = 32 >> lbw, nby = (H >> 3) >> lbh;
    if (b >= nbx * nby) return;
    const int x0 = block_bx(b, lbw) << (3 + lbw), y0 = block_by(b, lbw) << (3 + lbh), pw = 8 << lbw, ph = 8 << lbh;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f; int cnt = 0;
    for (int x = 0; x < pw; x++)
        for (int y = 0; y < ph; y++) {
            const size_t px = (size_t)(y0 + y) * W + x0 + x;
            const uint32_t o = reinterpret_cast<const uint32_t *>(orig)[px];
            if ((o >> 24) != 0) {
                if (perceptual) { s0 += labpx[3 * px]; s1 += labpx[3 * px + 1]; s2 += labpx[3 * px + 2]; }
                else { s0 += (float)(o & 0xff); s1 += (float)((o >> 8) & 0xff); s2 += (float)((o >> 16) & 0xff); }
                cnt++;
            }
        }
    sums[3 * b] = s0; sums[3 * b + 1] = s1; sums[3 * b + 2] = s2; counts[b] = cnt;
}

// The proxy reassignment over the costs of k_tile_costs: cost(b, p) = the binary64 sum, over the block's tiles in raster order,
// of cost[tile][p], tiles without an opaque pixel left out (for a tile, 0.0 + its cost: exact); a block with an opaque pixel
// moves as a whole to the strictly smallest cost, scanning upwards from the current subpalette's (ties keep the current one,
// then the lower index).  `moved` counts tiles.
__global__ void k_unit_move(const double *__restrict__ cost, const int *__restrict__ any, int H, int sub_count, int lbw, int lbh, uint8_t *__restrict__ tile_pal,
                            unsigned int *__restrict__ moved) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int nbx = 32 >> lbw, nby = (H >> 3) >> lbh;
    if (b >= nbx * nby) return;
    const int tx0 = block_bx(b, lbw) << lbw, ty0 = block_by(b, lbw) << lbh, tw = 1 << lbw, th = 1 << lbh;
    auto block_cost = [&](int p, bool &has) {
        double c = 0.0; has = false;
        for (int ty = ty0; ty < ty0 + th; ty++)
            for (int tx = tx0; tx < tx0 + tw; tx++) {
                const int tile = ty * 32 + tx;
                if (any[tile]) { c = c + cost[tile * sub_count + p]; has = true; }
            }
        return c;
    };
    const int cur = tile_pal[ty0 * 32 + tx0];
    bool has = false;
    double best_cost = block_cost(cur, has);
    if (!has) return;
    int best = cur;
    for (int p = 0; p < sub_count; p++) { const double c = block_cost(p, has); if (c < best_cost) { best_cost = c; best = p; } }
    if (best == cur) return;
    for (int ty = ty0; ty < ty0 + th; ty++)
        for (int tx = tx0; tx < tx0 + tw; tx++) tile_pal[ty * 32 + tx] = (uint8_t)best;
    atomicAdd(moved, (unsigned int)(tw * th));
}

} // namespace snes
