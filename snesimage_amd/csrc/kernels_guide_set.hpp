// snesimage_amd/csrc/kernels_guide_set.hpp — guided calls of a shared-palette set (shared_guide_host.inc; definition:
// include/snesimage_hip.h; DESIGN 5f').
//
// The proxy of kernels_guide.hpp carries over to a set without a new definition: the palette and the slot are shared and a
// pixel's floor depends on its own tile only, so the set's cost table is the integer sum of the members' tables — made here in
// one pass over one pixel list:
//   ks_guide_gather   the slot's population over ALL members as one list of (rgb8 of T_f, floor m), one block per global tile
//                     g = member * ntile + tile (as kernels_char_set.hpp numbers them), through a device table of the members'
//                     target and tile_palettes pointers;
//   k_guide_cost      kernels_guide.hpp's, unchanged, over that list (its integer sums make the list's order irrelevant);
//   ks_guide_select   k_guide_select's selection; the same launch writes the shortlist into EVERY member's candidate buffer
//                     through the member table (no F copies), and the costs into the workspace.
// All kernels are wave64; stores are plain vector stores; no scratch.
#pragma once
#include "kernels_guide.hpp"
#include "kernels_char_set.hpp"

namespace snes {

// What the generator touches of a member: it reads the target and tile_palettes, and writes the candidate list.
struct GuideMember { const uint8_t *target; const uint8_t *tile_pal; uint8_t *cand; };

// The population of a set.  grid = the G global tiles, block = the tile's 64 pixels (one wave).  k_guide_gather's body on the
// member's own planes otherwise: a tile of another subpalette leaves at once (sp < 0: the tied slot of a backdrop set, whose
// population is every tile of every member), the others take the next 64 places of the list with one atomic add per tile.
// colors: ONE member's palette as raw 5-bit triples — ks_commit and ks_commit_tied write every member's copy in the same launch,
// so any member's is the set's — read here so that a sweep's call sees the commit before it.
__global__ __launch_bounds__(64) void ks_guide_gather(const GuideMember *__restrict__ M, const uint8_t *__restrict__ colors, int ntile, int W, int sub_size, int sp, int si,
                                                     GuidePixel *__restrict__ list, unsigned int *__restrict__ count) {
    __shared__ uint32_t s_pal[256]; // (sub_count * sub_size <= 253)
    __shared__ unsigned int s_at;
    const int g = blockIdx.x, lane = threadIdx.x;
    const int f = g / ntile, t = g - f * ntile;
    const uint8_t *__restrict__ target = M[f].target;
    const int p = M[f].tile_pal[t];
    if (sp >= 0 && p != sp) return; // (uniform over the block)
    for (int j = lane; j < sub_size && j < 256; j += 64) { const uint8_t *c = colors + 3 * (p * sub_size + j); s_pal[j] = rgb5_to_rgb8(c[0], c[1], c[2]); }
    if (lane == 0) s_at = atomicAdd(count, 1u);
    __syncthreads();
    const int px = ((t >> 5) * 8 + (lane >> 3)) * W + (t & 31) * 8 + (lane & 7);
    const uint32_t o = reinterpret_cast<const uint32_t *>(target)[px];
    const uint32_t rgb = o & 0x00ffffffu;
    uint32_t m = kGuideNoFloor;
    for (int j = 0; j < sub_size; j++)
        if (j != si) { const uint32_t k = red_mean_key(rgb, s_pal[j]); m = k < m ? k : m; }
    GuidePixel q; q.rgb = rgb; q.m = (o >> 24) == 0 ? 0u : m;
    list[(size_t)s_at * 64 + lane] = q;
}

// The shortlist of a set.  k_guide_select's selection: one block of 1024 threads, thread i keeps the keys cost << 15 | u of the
// colours i, i + 1024, ... (32 of them) in registers; K rounds of a block-wide minimum; the owner of the winner drops it; the
// slot's current colour never enters.  A cost is below 2^47.2 (kSetTiles tiles x 64 pixels x the largest key, 299,505,150), so
// the packed key stays below 2^63.  Thread r < K writes candidate r into every member's list.
__global__ __launch_bounds__(1024) void ks_guide_select(const unsigned long long *__restrict__ cost, const uint8_t *__restrict__ colors, int slot, int K, const GuideMember *__restrict__ M, int F,
                                                       unsigned long long *__restrict__ cand_cost) {
    __shared__ unsigned long long s_red[16], s_out[kGuideShort];
    const int tid = threadIdx.x;
    const uint32_t cur = rgb5_as_u16(colors[3 * slot], colors[3 * slot + 1], colors[3 * slot + 2]);
    unsigned long long key[32];
#pragma unroll
    for (int i = 0; i < 32; i++) { const uint32_t u = (uint32_t)tid + 1024u * i; key[i] = u == cur ? kCharNone : ((cost[u] << 15) | u); }
    unsigned long long mine = kCharNone;
#pragma unroll
    for (int i = 0; i < 32; i++) mine = key[i] < mine ? key[i] : mine;
    for (int r = 0; r < K; r++) {
        const unsigned long long mn = block_min_u64<16>(mine, s_red);
        if (mine == mn) { // one owner: the keys differ
            s_out[r] = mn;
            mine = kCharNone;
#pragma unroll
            for (int i = 0; i < 32; i++) { if (key[i] == mn) key[i] = kCharNone; mine = key[i] < mine ? key[i] : mine; }
        }
    }
    __syncthreads();
    if (tid < K) {
        const unsigned long long k = s_out[tid];
        const uint32_t u = (uint32_t)(k & 0x7fffu);
        const uint8_t r5 = (uint8_t)(u & 31u), g5 = (uint8_t)((u >> 5) & 31u), b5 = (uint8_t)(u >> 10);
        for (int f = 0; f < F; f++) { uint8_t *cand = M[f].cand; cand[3 * tid] = r5; cand[3 * tid + 1] = g5; cand[3 * tid + 2] = b5; }
        cand_cost[tid] = k >> 15;
    }
}

} // namespace snes
