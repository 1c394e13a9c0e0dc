// snesimage_amd/csrc/kernels_guide.hpp — guided calls (guide_host.inc, shared_guide_host.inc; definition: include/snesimage_hip.h;
// DESIGN 5f, 5f').
//
// A guided call does not draw its candidates: it ranks ALL 32,768 BGR555 colours for the slot by an exact integer proxy — the
// k-means objective in the redmean key: what the pixels of the slot's subpalette would cost if the entry were that colour,
// every pixel keeping the best of its other entries as a floor — and hands the K cheapest to the scorer, where error() decides.
// The palette and the slot of a shared-palette set are shared and a pixel's floor depends on its own tile only, so the set's
// cost table is the integer sum of its members' tables: one pass over one pixel list makes it, and a single image is a set of
// one.  The kernels reach the images through a device table of members (GuideMember).
//   k_guide_gather   the slot's population over all members as a compact list of (rgb8 of T, floor m), 8 bytes a pixel, one
//                    block per global tile g = member * ntile + tile (as kernels_char_set.hpp numbers them);
//   k_guide_cost     cost(u) = sum over the list of min(m, key(T, rgb8(u))), one lane per colour, one block per 256 colours and
//                    slice of the list; the slices meet in 64-bit integer atomic adds (a wave's 64 adds are contiguous);
//   k_guide_select   the K lowest (cost, u) but the slot's current colour, in order: the candidates, written into EVERY
//                    member's candidate buffer by the same launch (no F copies), and their costs.
// Every sum is an integer sum: neither the order of the list nor the order of the adds shows in the result.
// All kernels are wave64; stores are plain vector stores; no scratch.
#pragma once
#include "kernels_char.hpp"

namespace snes {

constexpr int kGuideColors = 32768;      // every BGR555 colour, indexed u = r | g << 5 | b << 10 (rgb5_as_u16)
constexpr int kGuideSlice = 1024;        // pixels of the list per block of k_guide_cost: a 256 x 8 picture at one subpalette spans two
constexpr int kGuideShort = 64;          // longest shortlist
constexpr uint32_t kGuideNoFloor = 0xffffffffu; // a one-entry subpalette has no other entry: every key is below it

struct GuidePixel { uint32_t rgb, m; }; // packed 0x00BBGGRR of T, and the floor; a transparent pixel has m = 0 and adds 0 to every sum

// What the generator touches of a member: it reads the target and tile_palettes, and writes the candidate list.
struct GuideMember { const uint8_t *target; const uint8_t *tile_pal; uint8_t *cand; };

// The population.  grid = the global tiles of all members, block = the tile's 64 pixels (one wave).  A tile of another
// subpalette leaves at once (sp < 0: the tied slot of a backdrop context or set, whose population is every tile of every
// member); the others take the next 64 places of the list with one atomic add per tile.  colors: ONE member's palette as raw
// 5-bit triples — ks_commit and ks_commit_tied write every member's copy in the same launch, so any member's is the set's — read
// here so that a sweep's call sees the commit before it.
__global__ __launch_bounds__(64) void k_guide_gather(const GuideMember *__restrict__ M, const uint8_t *__restrict__ colors, int ntile, int W, int sub_size, int sp, int si,
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

// cost(u) for the 256 colours of blockIdx.x over slice blockIdx.y of the list.  The slice is staged in LDS and read by all
// lanes at one address (a broadcast).  A key is below 2^29: eight of them fit a 32-bit partial sum, which then joins the lane's
// 64-bit accumulator.  Blocks beyond the list's end leave at once (the host launches for the largest list: it does not know
// the count).
__global__ __launch_bounds__(256) void k_guide_cost(const GuidePixel *__restrict__ list, const unsigned int *__restrict__ count, unsigned long long *__restrict__ cost) {
    __shared__ uint2 s_px[kGuideSlice];
    const int n = (int)(*count) * 64;
    const int first = blockIdx.y * kGuideSlice;
    if (first >= n) return; // (uniform over the block)
    const int len = n - first < kGuideSlice ? n - first : kGuideSlice; // a multiple of 64
    for (int i = threadIdx.x; i < len; i += 256) s_px[i] = reinterpret_cast<const uint2 *>(list)[first + i];
    __syncthreads();
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    const uint32_t crgb = rgb5_to_rgb8(u & 31u, (u >> 5) & 31u, u >> 10);
    unsigned long long acc = 0ull;
    for (int i = 0; i < len; i += 8) {
        uint32_t part = 0u;
#pragma unroll
        for (int j = 0; j < 8; j++) { const uint2 q = s_px[i + j]; const uint32_t k = red_mean_key(q.x, crgb); part += k < q.y ? k : q.y; }
        acc += part;
    }
    atomicAdd(cost + u, acc);
}

// The shortlist.  One block of 1024 threads; thread i keeps the keys cost << 15 | u of the colours i, i + 1024, ... (32 of
// them) in registers — the keys differ, u being part of them, and order as (cost, u) does.  A cost is below 2^47.2 (kSetTiles
// tiles x 64 pixels x the largest key, 299,505,150), so the packed key stays below 2^63.  K rounds of a block-wide minimum; the
// owner of the winner drops it.  The slot's current colour never enters.  Thread r < K writes candidate r into every member's list.
__global__ __launch_bounds__(1024) void k_guide_select(const unsigned long long *__restrict__ cost, const uint8_t *__restrict__ colors, int slot, int K, const GuideMember *__restrict__ M, int F,
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
