// snesimage_amd/csrc/kernels_guide_lab.hpp — the CIELAB proxy of guided calls (guide_host.inc, shared_guide_host.inc;
// definition: include/snesimage_hip.h; DESIGN 5f'').
//
// The proxy of kernels_guide.hpp with the distance the pixels of a perceptual context choose their entry by:
// d(c, x) = ciede2000(Lab(rgb8(c)), Lab(T(x))) in f32, entry first, as prep_body calls it, made an exact integer by
// q(d) = min((uint32_t)(d * 65536.0f), 0xFFFFFF).  q is monotone, so min(q(m), q(d)) = q(min(m, d)): the floor travels as
// the f32 distance and one conversion per pixel and colour serves both.
//   k_guide_gather_lab    the slot's population over all members as a list of (Lab of T, floor m as f32), 16 bytes a pixel,
//                         one block per global tile;
//   k_guide_cost_lab      cost(u) = sum over the list of q(min(m, d(c_u, x))), one lane per colour, one block per 256
//                         colours and slice of the list; the slices meet in 64-bit integer atomic adds.
// k_guide_select takes the table as it is: a cost is below 2^43.
// Every sum is an integer sum: neither the order of the list, nor the order of the adds, nor the colour a lane holds shows in
// the result.  All kernels are wave64; stores are plain vector stores.
#pragma once
#include "kernels_guide.hpp"

namespace snes {

constexpr int kGuideLabPart = 64;           // q's per 32-bit partial sum: 64 * 0xFFFFFF < 2^30 (128 would still fit)
constexpr float kGuideLabQMax = 16777215.0f; // 0xFFFFFF, exact in f32

// Lab of T and the floor; a transparent pixel has m = 0 and adds q(0) = 0 to every sum, a one-entry subpalette has m = +inf
struct GuideLabPixel { float l, a, b, m; };

__device__ __forceinline__ Lab guide_lab_of(uint32_t rgb8, const float *__restrict__ lab_eotf) {
    return linear_to_lab(lab_eotf[rgb8 & 0xff], lab_eotf[(rgb8 >> 8) & 0xff], lab_eotf[(rgb8 >> 16) & 0xff]);
}
// d * 2^16 is exact in f32; clamping before the truncation equals clamping behind it (0xFFFFFF is a float)
__device__ __forceinline__ uint32_t guide_lab_q(float d) { return (uint32_t)fminf(d * 65536.0f, kGuideLabQMax); }

// The population.  grid = the global tiles g = member * ntile + tile, block = the tile's 64 pixels (one wave); k_guide_gather's
// discipline and body, in Lab.
__global__ __launch_bounds__(64) void k_guide_gather_lab(const GuideMember *__restrict__ M, const uint8_t *__restrict__ colors, const float *__restrict__ lab_eotf, int ntile, int W, int sub_size,
                                                        int sp, int si, GuideLabPixel *__restrict__ list, unsigned int *__restrict__ count) {
    __shared__ Lab s_pal[256]; // (sub_count * sub_size <= 253)
    __shared__ unsigned int s_at;
    const int g = blockIdx.x, lane = threadIdx.x;
    const int f = g / ntile, t = g - f * ntile;
    const uint8_t *__restrict__ target = M[f].target;
    const int p = M[f].tile_pal[t];
    if (sp >= 0 && p != sp) return; // (uniform over the block)
    for (int j = lane; j < sub_size && j < 256; j += 64) { const uint8_t *c = colors + 3 * (p * sub_size + j); s_pal[j] = guide_lab_of(rgb5_to_rgb8(c[0], c[1], c[2]), lab_eotf); }
    if (lane == 0) s_at = atomicAdd(count, 1u);
    __syncthreads();
    const int px = ((t >> 5) * 8 + (lane >> 3)) * W + (t & 31) * 8 + (lane & 7);
    const uint32_t o = reinterpret_cast<const uint32_t *>(target)[px];
    const Lab tl = guide_lab_of(o, lab_eotf);
    float m = __builtin_inff();
    for (int j = 0; j < sub_size; j++)
        if (j != si) { const float d = ciede2000(s_pal[j], tl); m = d < m ? d : m; }
    GuideLabPixel q; q.l = tl.l; q.a = tl.a; q.b = tl.b; q.m = (o >> 24) == 0 ? 0.0f : m;
    list[(size_t)s_at * 64 + lane] = q;
}

// cost(u) for 256 colours over slice blockIdx.y of the list.  The slice is staged in LDS and read by all lanes at one address
// (a broadcast).  The integer sums leave the mapping of colours to lanes free: a wave holds the 32 blues of two neighbouring
// reds at one green — blue moves lightness least, so the lanes of a wave agree most often on the two sure "no"s of color.hpp
// (ciede2000_cannot_beat, ciede2000_cannot_beat_ab) against the pixel's floor, and a wave whose lanes all say no passes the
// formula by: such a pixel adds q(m), which is what min(m, d) gives when d is above m.  Blocks beyond the list's end leave at once.
// Measured on an MI355X (the bench picture, perceptual, generator ms at 8 x 15 / 1 x 15; all four variants write equal tables):
// this kernel 6.0 / 30.5; u = blockIdx.x * 256 + threadIdx.x with both tests 6.6 / 37.9; the lightness test alone 6.7 / 35.7;
// no test at all 8.4 / 62.9 (75 VGPRs).  The tests pay off in spite of the divergence, and the mapping adds to it.
__global__ __launch_bounds__(256) void k_guide_cost_lab(const GuideLabPixel *__restrict__ list, const unsigned int *__restrict__ count, const float *__restrict__ lab_eotf,
                                                      unsigned long long *__restrict__ cost) {
    __shared__ float4 s_px[kGuideSlice];
    const int n = (int)(*count) * 64;
    const int first = blockIdx.y * kGuideSlice;
    if (first >= n) return; // (uniform over the block)
    const int len = n - first < kGuideSlice ? n - first : kGuideSlice; // a multiple of 64
    for (int i = threadIdx.x; i < len; i += 256) s_px[i] = reinterpret_cast<const float4 *>(list)[first + i];
    __syncthreads();
    const uint32_t g5 = blockIdx.x & 31u, r5 = (blockIdx.x >> 5) * 8u + (threadIdx.x >> 5), b5 = threadIdx.x & 31u;
    const uint32_t u = r5 | (g5 << 5) | (b5 << 10);
    const Lab cl = guide_lab_of(rgb5_to_rgb8(r5, g5, b5), lab_eotf);
    const float cch = sqrtf(cl.a * cl.a + cl.b * cl.b);
    unsigned long long acc = 0ull;
    for (int i = 0; i < len; i += kGuideLabPart) {
        uint32_t part = 0u;
        for (int j = 0; j < kGuideLabPart; j++) {
            const float4 q = s_px[i + j];
            const Lab t{q.x, q.y, q.z};
            float v = q.w;
            if (!ciede2000_cannot_beat(cl, t, q.w) && !ciede2000_cannot_beat_ab(cl, cch, t, q.w)) { const float d = ciede2000(cl, t); v = d < v ? d : v; }
            part += guide_lab_q(v);
        }
        acc += part;
    }
    atomicAdd(cost + u, acc);
}

} // namespace snes
