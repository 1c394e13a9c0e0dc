// snesimage_amd/csrc/kernels_guide_window.hpp — the guided calls' generator for a slot window (guided_window_host.inc;
// definition: include/snesimage_hip.h, snesimage_guided_run_slots; DESIGN 5f''').
//
// A guided window is a scheduled window (kernels_batch.hpp) whose candidate lists are shortlists: kw_gen_candidates' place is
// taken by the three kernels of kernels_guide.hpp with the call of the window as one more grid dimension.  Every call has its own
// pixel list, count and 32,768-entry table in the workspace; call j's slot is WindowSlot::slot of the window's record j, in the
// context's own terms (sub_size is the internal one: a backdrop context's regular slots see B as one of the other entries).
//   kw_guide_gather   grid (tiles, calls) x 64:          k_guide_gather for the call's slot, into the call's list and count;
//   kw_guide_cost     grid (128, slices, calls) x 256:   k_guide_cost on the call's list into the call's table;
//   kw_guide_select   grid (calls) x 1024:               k_guide_select; candidate r of call j goes to cand + 3 * (j * K + r), and
//                                                        errors[j * K + r] is preset to +inf, as kw_gen_candidates presets it.
// Every sum is an integer sum: the tables, and so the shortlists, equal the single-call generator's whatever the order of the
// list and of the adds.  Like every kernel of a window they leave at once when an earlier window's commit has voided theirs.
// All kernels are wave64; stores are plain vector stores; no scratch.
#pragma once
#include "kernels_batch.hpp"
#include "kernels_guide.hpp"

namespace snes {

__global__ __launch_bounds__(64) void kw_guide_gather(const WindowSlot *__restrict__ S, const uint8_t *__restrict__ target, const uint8_t *__restrict__ tile_pal, const uint8_t *__restrict__ colors, int ntile, int W,
                                                     int sub_size, GuidePixel *__restrict__ lists, unsigned int *__restrict__ counts, const int *__restrict__ dead, int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ uint32_t s_pal[256]; // (sub_count * sub_size <= 253)
    __shared__ unsigned int s_at;
    const int t = blockIdx.x, call = blockIdx.y, lane = threadIdx.x;
    const int slot = S[call].slot, sp = slot / sub_size, si = slot - sp * sub_size;
    if (tile_pal[t] != sp) return; // (uniform over the block)
    for (int j = lane; j < sub_size && j < 256; j += 64) { const uint8_t *c = colors + 3 * (sp * sub_size + j); s_pal[j] = rgb5_to_rgb8(c[0], c[1], c[2]); }
    if (lane == 0) s_at = atomicAdd(counts + call, 1u);
    __syncthreads();
    const int px = ((t >> 5) * 8 + (lane >> 3)) * W + (t & 31) * 8 + (lane & 7);
    const uint32_t o = reinterpret_cast<const uint32_t *>(target)[px];
    const uint32_t rgb = o & 0x00ffffffu;
    uint32_t m = kGuideNoFloor;
    for (int j = 0; j < sub_size; j++)
        if (j != si) { const uint32_t k = red_mean_key(rgb, s_pal[j]); m = k < m ? k : m; }
    GuidePixel q; q.rgb = rgb; q.m = (o >> 24) == 0 ? 0u : m;
    lists[((size_t)call * ntile + s_at) * 64 + lane] = q; // (a call's list holds at most ntile tiles)
}

// blockIdx.z = call.  Blocks beyond the call's count leave at once (the host launches for the largest list, every tile).
__global__ __launch_bounds__(256) void kw_guide_cost(const GuidePixel *__restrict__ lists, const unsigned int *__restrict__ counts, int ntile, unsigned long long *__restrict__ costs,
                                                    const int *__restrict__ dead, int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ uint2 s_px[kGuideSlice];
    const int call = blockIdx.z;
    const int n = (int)counts[call] * 64;
    const int first = blockIdx.y * kGuideSlice;
    if (first >= n) return; // (uniform over the block)
    const int len = n - first < kGuideSlice ? n - first : kGuideSlice; // a multiple of 64
    const uint2 *__restrict__ list = reinterpret_cast<const uint2 *>(lists) + (size_t)call * ntile * 64;
    for (int i = threadIdx.x; i < len; i += 256) s_px[i] = list[first + i];
    __syncthreads();
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    const uint32_t crgb = rgb5_to_rgb8(u & 31u, (u >> 5) & 31u, u >> 10);
    unsigned long long acc = 0ull;
    for (int i = 0; i < len; i += 8) {
        uint32_t part = 0u; // a key is below 2^29: eight of them fit
#pragma unroll
        for (int j = 0; j < 8; j++) { const uint2 q = s_px[i + j]; const uint32_t k = red_mean_key(q.x, crgb); part += k < q.y ? k : q.y; }
        acc += part;
    }
    atomicAdd(costs + (size_t)call * kGuideColors + u, acc);
}

// blockIdx.x = call: k_guide_select's K rounds of a block-wide minimum over the call's table.
__global__ __launch_bounds__(1024) void kw_guide_select(const WindowSlot *__restrict__ S, const unsigned long long *__restrict__ costs, const uint8_t *__restrict__ colors, int K, uint8_t *__restrict__ cand,
                                                       double *__restrict__ errors, const int *__restrict__ dead, int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ unsigned long long s_red[16], s_out[kGuideShort];
    const int tid = threadIdx.x, call = blockIdx.x;
    const int slot = S[call].slot;
    const unsigned long long *__restrict__ cost = costs + (size_t)call * kGuideColors;
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
        const uint32_t u = (uint32_t)(s_out[tid] & 0x7fffu);
        uint8_t *c = cand + 3 * ((size_t)call * K + tid);
        c[0] = (uint8_t)(u & 31u); c[1] = (uint8_t)((u >> 5) & 31u); c[2] = (uint8_t)(u >> 10);
        errors[(size_t)call * K + tid] = __longlong_as_double(0x7ff0000000000000ll);
    }
}

} // namespace snes
