// snesimage_amd/csrc/kernels_guide_set_window.hpp — the guided calls' generator for a slot window of a shared-palette set
// (shared_guided_window_host.inc; definition: include/snesimage_hip.h, snesimage_shared_guided_run_slots; DESIGN 5f'''').
//
// All calls of a window see one palette, so the calls on one subpalette p share their pixels.  For a pixel x of p's population,
// over the entries j of the subpalette (the expanded one on a backdrop set):
//   a(x) = the lowest red_mean_key(T(x), rgb8(entry j));  j*(x) = the first j that reaches it;  b(x) = the lowest key over
//   j != j*(x), kGuideNoFloor with one entry.
// The floor of slot (p, i) is m_i(x) = b(x) where j*(x) == i, else a(x) (a tie of the two lowest keys gives a == b).  Hence
//   A_p(u)     = sum over p's population            of min(a, key(x, u))                         once per subpalette and window,
//   D_{p,i}(u) = sum over the pixels with j* == i   of min(b, key(x, u)) - min(a, key(x, u))     once per call (every term >= 0),
//   cost_{p,i}(u) = A_p(u) + D_{p,i}(u),
// in integers and exactly: the S calls of a subpalette cost about twice its population x 32,768 keys instead of S times.
// A window's distinct subpalettes are numbered in the order of their first call: plan[j] = the number of call j's subpalette,
// the index of its shared list, count and table (written by the host, which knows the calls).
//   ksgw_gather_shared  grid (global tiles) x 64:       (rgb8 of T, a) into the list of the tile's subpalette, if the window has
//                                                       a call on it: the layout kw_guide_cost reads, with "call" = plan number;
//   kw_guide_cost       (kernels_guide_window.hpp, unchanged) makes A of every shared list;
//   ksgw_gather_own     grid (global tiles, calls) x 64: the pixels of the tile whose nearest entry is the call's, compacted by
//                                                       ballot, as (rgb8, a, b); a tile's run is padded to 8 pixels with zero
//                                                       pixels (a = b = 0 adds 0, as a transparent pixel does);
//   ksgw_cost_diff      grid (128, slices, calls) x 256: D of the call's own list, slices taken in a grid-stride loop;
//   ksgw_select         grid (calls) x 1024:            k_guide_select over A[plan[j]] + D[j]; candidate r of call j goes to
//                                                       cand + 3 * (j * K + r) and errors[j * K + r] is preset to +inf, as
//                                                       kw_gen_candidates presets it in a set's window.
// Every sum is an integer sum met in 64-bit atomic adds: the tables, and so the shortlists, equal the single-call generator's bit
// for bit.  All kernels are wave64 and start with the window's `dead` check; stores are plain vector stores; no scratch.
#pragma once
#include "kernels_guide_window.hpp"

namespace snes {

constexpr int kGuideGranule = 8; // pixels: the unit of a call's own list (ksgw_cost_diff sums eight 32-bit terms at a time)

struct GuideOwnPixel { uint32_t rgb, a, b, pad; }; // packed 0x00BBGGRR of T, the lowest and the second-lowest key; 16 bytes: one LDS read

// The shared lists.  The block's tile goes to list plan[first call on its subpalette]; a tile whose subpalette no call of the
// window names leaves at once.
__global__ __launch_bounds__(64) void ksgw_gather_shared(const WindowSlot *__restrict__ S, const int *__restrict__ plan, int K, const GuideMember *__restrict__ M, const uint8_t *__restrict__ colors, int ntile,
                                                        int G, int W, int sub_size, GuidePixel *__restrict__ lists, unsigned int *__restrict__ counts, const int *__restrict__ dead, int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ uint32_t s_pal[256]; // (sub_count * sub_size <= 253)
    __shared__ unsigned int s_at;
    const int g = blockIdx.x, lane = threadIdx.x;
    const int f = g / ntile, t = g - f * ntile;
    const int p = M[f].tile_pal[t];
    int q = -1;
    for (int j = 0; j < K; j++)
        if (S[j].slot / sub_size == p) { q = plan[j]; break; } // (uniform over the block)
    if (q < 0) return;
    for (int j = lane; j < sub_size && j < 256; j += 64) { const uint8_t *c = colors + 3 * (p * sub_size + j); s_pal[j] = rgb5_to_rgb8(c[0], c[1], c[2]); }
    if (lane == 0) s_at = atomicAdd(counts + q, 1u);
    __syncthreads();
    const int px = ((t >> 5) * 8 + (lane >> 3)) * W + (t & 31) * 8 + (lane & 7);
    const uint32_t o = reinterpret_cast<const uint32_t *>(M[f].target)[px];
    const uint32_t rgb = o & 0x00ffffffu;
    uint32_t a = kGuideNoFloor;
    for (int j = 0; j < sub_size; j++) { const uint32_t k = red_mean_key(rgb, s_pal[j]); a = k < a ? k : a; }
    GuidePixel v; v.rgb = rgb; v.m = (o >> 24) == 0 ? 0u : a;
    lists[((size_t)q * G + s_at) * 64 + lane] = v; // (a list holds at most G tiles)
}

// A call's own list.  blockIdx.y = call.  counts[call] is in granules of 8 pixels; a tile adds at most 8 of them, so a call's
// list stays within G * 64 pixels.
__global__ __launch_bounds__(64) void ksgw_gather_own(const WindowSlot *__restrict__ S, const GuideMember *__restrict__ M, const uint8_t *__restrict__ colors, int ntile, int G, int W, int sub_size,
                                                     GuideOwnPixel *__restrict__ lists, unsigned int *__restrict__ counts, const int *__restrict__ dead, int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ uint32_t s_pal[256];
    __shared__ unsigned int s_at;
    const int g = blockIdx.x, call = blockIdx.y, lane = threadIdx.x;
    const int f = g / ntile, t = g - f * ntile;
    const int slot = S[call].slot, sp = slot / sub_size, si = slot - sp * sub_size;
    if (M[f].tile_pal[t] != sp) return; // (uniform over the block)
    for (int j = lane; j < sub_size && j < 256; j += 64) { const uint8_t *c = colors + 3 * (sp * sub_size + j); s_pal[j] = rgb5_to_rgb8(c[0], c[1], c[2]); }
    __syncthreads();
    const int px = ((t >> 5) * 8 + (lane >> 3)) * W + (t & 31) * 8 + (lane & 7);
    const uint32_t o = reinterpret_cast<const uint32_t *>(M[f].target)[px];
    const uint32_t rgb = o & 0x00ffffffu;
    uint32_t a = kGuideNoFloor, b = kGuideNoFloor;
    int js = -1;
    for (int j = 0; j < sub_size; j++) {
        const uint32_t k = red_mean_key(rgb, s_pal[j]);
        if (js < 0 || k < a) { b = a; a = k; js = j; } // strict <: the first entry that reaches the lowest key stays j*
        else if (k < b) b = k;
    }
    const bool own = (o >> 24) != 0 && js == si;
    const unsigned long long mask = __ballot(own);
    const int n = __popcll(mask);
    if (n == 0) return; // (uniform: the entry is nearest to no pixel of this tile)
    const int gran = (n + kGuideGranule - 1) / kGuideGranule;
    if (lane == 0) s_at = atomicAdd(counts + call, (unsigned int)gran);
    __syncthreads();
    GuideOwnPixel *__restrict__ run = lists + (size_t)call * G * 64 + (size_t)s_at * kGuideGranule;
    if (own) { GuideOwnPixel v; v.rgb = rgb; v.a = a; v.b = b; v.pad = 0u; run[__popcll(mask & ((1ull << lane) - 1ull))] = v; }
    if (lane < gran * kGuideGranule - n) { GuideOwnPixel z; z.rgb = 0u; z.a = 0u; z.b = 0u; z.pad = 0u; run[n + lane] = z; }
}

// D for the 256 colours of blockIdx.x over the slices blockIdx.y, blockIdx.y + gridDim.y, ... of call blockIdx.z's own list: the
// host does not know the counts, and the own lists of a subpalette's calls share its population between them, so a grid for the
// largest list would be idle blocks for the most part.  A term min(b, key) - min(a, key) is below 2^29: eight fit 32 bits.
__global__ __launch_bounds__(256) void ksgw_cost_diff(const GuideOwnPixel *__restrict__ lists, const unsigned int *__restrict__ counts, int G, unsigned long long *__restrict__ costs, const int *__restrict__ dead,
                                                     int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ uint4 s_px[kGuideSlice];
    const int call = blockIdx.z;
    const int n = (int)counts[call] * kGuideGranule;
    const uint4 *__restrict__ list = reinterpret_cast<const uint4 *>(lists) + (size_t)call * G * 64;
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    const uint32_t crgb = rgb5_to_rgb8(u & 31u, (u >> 5) & 31u, u >> 10);
    unsigned long long acc = 0ull;
    for (int first = blockIdx.y * kGuideSlice; first < n; first += gridDim.y * kGuideSlice) { // (uniform over the block)
        const int len = n - first < kGuideSlice ? n - first : kGuideSlice; // a multiple of 8
        __syncthreads(); // the slice before this one has been read
        for (int i = threadIdx.x; i < len; i += 256) s_px[i] = list[first + i];
        __syncthreads();
        for (int i = 0; i < len; i += kGuideGranule) {
            uint32_t part = 0u;
#pragma unroll
            for (int j = 0; j < kGuideGranule; j++) {
                const uint4 q = s_px[i + j];
                const uint32_t k = red_mean_key(q.x, crgb);
                part += (k < q.z ? k : q.z) - (k < q.y ? k : q.y);
            }
            acc += part;
        }
    }
    if (acc) atomicAdd(costs + (size_t)call * kGuideColors + u, acc);
}

// blockIdx.x = call: k_guide_select's K rounds of a block-wide minimum over A[plan[call]] + D[call].
__global__ __launch_bounds__(1024) void ksgw_select(const WindowSlot *__restrict__ S, const int *__restrict__ plan, const unsigned long long *__restrict__ shared_costs, const unsigned long long *__restrict__ own_costs,
                                                   const uint8_t *__restrict__ colors, int K, uint8_t *__restrict__ cand, double *__restrict__ errors, const int *__restrict__ dead, int dead_base) {
    if (*dead >= dead_base) return;
    __shared__ unsigned long long s_red[16], s_out[kGuideShort];
    const int tid = threadIdx.x, call = blockIdx.x;
    const int slot = S[call].slot;
    const unsigned long long *__restrict__ A = shared_costs + (size_t)plan[call] * kGuideColors;
    const unsigned long long *__restrict__ D = own_costs + (size_t)call * kGuideColors;
    const uint32_t cur = rgb5_as_u16(colors[3 * slot], colors[3 * slot + 1], colors[3 * slot + 2]);
    unsigned long long key[32];
#pragma unroll
    for (int i = 0; i < 32; i++) { const uint32_t u = (uint32_t)tid + 1024u * i; key[i] = u == cur ? kCharNone : (((A[u] + D[u]) << 15) | u); }
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
