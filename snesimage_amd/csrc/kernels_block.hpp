// snesimage_amd/csrc/kernels_block.hpp — palette blocks: one subpalette per block of bw x bh tiles (block_host.inc).
//
// A block-move candidate is a (block, subpalette) pair: the image as it stands with every tile of that block drawn from
// another subpalette, the palette untouched.  The kernels mirror kernels_tile.hpp with "the candidate's tile" read as "a tile
// inside the candidate's block"; the scorer, its workspace and the Floyd-Steinberg kernels are the tile moves' own.
// Blocks are bw x bh tiles with bw, bh in {1, 2, 4, 8}, passed as their logarithms (lbw, lbh); the image is 32 tiles wide, so
// block b = by * (32 >> lbw) + bx covers tiles tx >> lbw == bx, ty >> lbh == by.  At lbw == lbh == 0 a block is a tile.
#pragma once
#include "kernels.hpp"
#include "kernels_opt.hpp"
#include "kernels_tile.hpp"

namespace snes {

// block b = by * nbx + bx with nbx = 32 >> lbw a power of two: bx and by are a mask and a shift
__device__ __forceinline__ int block_bx(int block, int lbw) { return block & ((32 >> lbw) - 1); }
__device__ __forceinline__ int block_by(int block, int lbw) { return block >> (5 - lbw); }
__device__ __forceinline__ bool tile_in_block(int tile, int block, int lbw, int lbh) {
    return ((tile & 31) >> lbw) == block_bx(block, lbw) && ((tile >> 5) >> lbh) == block_by(block, lbw);
}

// per candidate: the tile table with the candidate's whole block moved (what its Floyd-Steinberg run reads)
__global__ __launch_bounds__(256) void k_block_tabs(const uint8_t *__restrict__ tile_pal, const uint16_t *__restrict__ blocks, const uint8_t *__restrict__ subs, int lbw, int lbh,
                                                   uint8_t *__restrict__ tabs) {
    const int cand = blockIdx.x, cb = blocks[cand];
    const uint8_t k = subs[cand];
    for (int i = threadIdx.x; i < 1024; i += 256) tabs[(size_t)cand * 1024 + i] = tile_in_block(i, cb, lbw, lbh) ? k : tile_pal[i];
}

struct BlockRemapParams {
    const uint8_t *orig, *base_map; const uint32_t *pal_rgb8; const float *pal_lab, *labpx;
    const uint16_t *blocks; const uint8_t *subs;
    uint8_t *lmaps; // [cand][W*H]: the candidate's palette_map
    int W, H, sub_size, perceptual, lbw, lbh;
};
// the search of k_tile_remap for one pixel: exact integer redmean key or CIEDE2000, strict <: lowest index; 0 under alpha 0
__device__ __forceinline__ uint32_t block_search(const BlockRemapParams &P, int px, int base) {
    const uint32_t o = reinterpret_cast<const uint32_t *>(P.orig)[px];
    if ((o >> 24) == 0) return 0u;
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
    return (uint32_t)best;
}
// Without dither: the candidate's palette_map is the current one with the block's (8 << lbw) x (8 << lbh) pixels, up to 4,096,
// remapped to the nearest entry of the candidate's subpalette.  One workgroup per candidate; a thread takes the four pixels of
// a word (a block's rows are multiples of eight pixels, so a word never leaves the block).
__global__ __launch_bounds__(256) void k_block_remap(BlockRemapParams P) {
    const int cand = blockIdx.x, t = threadIdx.x;
    const int cb = P.blocks[cand], base = (int)P.subs[cand] * P.sub_size;
    const int npx = P.W * P.H;
    const int x0 = block_bx(cb, P.lbw) << (3 + P.lbw), y0 = block_by(cb, P.lbw) << (3 + P.lbh);
    const int lrow = 1 + P.lbw, nword = 1 << (4 + P.lbw + P.lbh); // words per row of the block (log2); words of the block
    const uint4 *src = reinterpret_cast<const uint4 *>(P.base_map);
    uint4 *dst = reinterpret_cast<uint4 *>(P.lmaps + (size_t)cand * npx);
    for (int i = t; i < npx / 16; i += 256) dst[i] = src[i];
    __syncthreads(); // the copy of the block's rows is in place before its bytes are replaced
    for (int w = t; w < nword; w += 256) {
        const int px = (y0 + (w >> lrow)) * P.W + x0 + ((w & ((1 << lrow) - 1)) << 2);
        if (y0 + (w >> lrow) >= P.H) continue; // (a block never leaves the image: bh divides h/8)
        uint32_t m = 0;
#pragma unroll 1
        for (int q = 0; q < 4; q++) m |= block_search(P, px + q, base) << (8 * q); // (one copy of the search: four would spill scalar registers)
        reinterpret_cast<uint32_t *>(P.lmaps + (size_t)cand * npx)[px >> 2] = m;
    }
}

// palette_map -> full colour indices (sub * sub_size + map, the tiles of the candidate's block under its new subpalette),
// row-major and C4.  grid (W*H/1024, candidates); a thread takes the four pixels of one word.
__global__ __launch_bounds__(256) void k_block_full(const uint8_t *__restrict__ lmaps, const uint8_t *__restrict__ tile_pal, const uint16_t *__restrict__ blocks, const uint8_t *__restrict__ subs,
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

// The window's block calls in order, as k_tile_commit (TileCall::tile holds the block): every call up to and including the
// first that accepts is logged; that one's block (its (1 << lbw) x (1 << lbh) table entries), map and error become the image's.
__global__ __launch_bounds__(1024) void k_block_commit(const double *__restrict__ errs, const TileCall *__restrict__ calls, int ncalls, const uint8_t *__restrict__ subs,
                                                      const uint8_t *__restrict__ lmaps, int npx, int lbw, int lbh, uint8_t *__restrict__ tile_pal, uint8_t *__restrict__ map,
                                                      double *__restrict__ inc_err, TileLog *__restrict__ log, TileWinRes *__restrict__ res) {
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
    const int cb = (int)calls[s_call].tile, ntb = 1 << (lbw + lbh);
    if ((int)threadIdx.x < ntb) { // the block's tiles, at most 64
        const int tx = (block_bx(cb, lbw) << lbw) + ((int)threadIdx.x & ((1 << lbw) - 1)), ty = (block_by(cb, lbw) << lbh) + ((int)threadIdx.x >> lbw);
        tile_pal[ty * 32 + tx] = subs[win];
    }
    if (threadIdx.x == 0) *inc_err = errs[win];
}

// per-block f32 sums in the reference's order with the block in place of the tile (lib.rs:91-116): the block's pixels x outer,
// y inner, one ordered chain per block
__global__ void k_block_sums(const uint8_t *__restrict__ orig, const float *__restrict__ labpx, int W, int H, int perceptual, int lbw, int lbh, float *__restrict__ sums /*[blocks][3]*/,
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

// The blocked move over the costs of k_tile_costs: cost(b, p) = the binary64 sum, over the block's tiles in raster order, of
// cost[tile][p], tiles without an opaque pixel left out; a block with an opaque pixel moves as a whole by k_tile_move's rule
// (strictly smallest cost, ties keep the current subpalette, then the lower index).  `moved` counts tiles.
__global__ void k_block_move(const double *__restrict__ cost, const int *__restrict__ any, int H, int sub_count, int lbw, int lbh, uint8_t *__restrict__ tile_pal,
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
