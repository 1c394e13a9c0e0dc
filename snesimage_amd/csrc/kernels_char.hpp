// snesimage_amd/csrc/kernels_char.hpp — the character budget (char_host.inc; definition: include/snesimage_hip.h).
//
// A tile's CHARACTER is the 64 values the JSON's `tiles` holds for it; two tiles share one if they are equal under one of the
// four flips the tilemap word provides.  A MERGE (t, b, f) gives tile t the indices of tile b under flip f, in t's own
// subpalette.  Which merges are worth scoring is decided by an integer proxy (the sum of the remap's distance key over the
// tile's 64 pixels, k_merge_proxy), which merge is taken by error() itself: the shortlisted candidates' maps (k_merge_maps) go
// through the map-reading scorer of the tile moves as they are, and k_merge_commit applies the winner.
// All kernels are wave64; a block's waves meet through LDS.
#pragma once
#include "kernels.hpp"

namespace snes {

constexpr int kCharShort = 64;                       // longest shortlist, and the slots of a block's partial list
constexpr unsigned long long kCharNone = ~0ull;      // "no candidate": above every packed key
struct MergeLog { double error; unsigned long long cost; uint16_t tile, donor; uint8_t flip, rank; uint16_t unique; }; // = snesimage_merge_result
struct CharInfo { uint32_t unique, nshort; };         // classes of the image as it stands; candidates in the shortlist

// cost << 22 | t << 12 | b << 2 | f: orders as the tuple (cost, t, b, f) does (t, b < 1024; cost < 2^37)
__device__ inline unsigned long long merge_key(unsigned long long cost, uint32_t t, uint32_t b, uint32_t f) { return (cost << 22) | ((unsigned long long)t << 12) | (b << 2) | f; }

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
// the minimum over a block of NW waves; every thread gets it.  s_red: NW slots.  Two barriers.
template <int NW> __device__ inline unsigned long long block_min_u64(unsigned long long v, unsigned long long *s_red) {
    v = wave_min_u64(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = s_red[0];
#pragma unroll
    for (int i = 1; i < NW; i++) m = s_red[i] < m ? s_red[i] : m;
    __syncthreads(); // s_red is free again
    return m;
}

// Characters and pinned flags.  grid = tiles of the image, block = the tile's 64 pixels (one wave).
// zero_at: the map value that reads 0 (the backdrop entry of a backdrop context), or -1.
__global__ __launch_bounds__(64) void k_char_build(const uint8_t *__restrict__ orig, const uint8_t *__restrict__ map, int W, int zero_at, uint8_t *__restrict__ chars, uint8_t *__restrict__ pinned) {
    const int t = blockIdx.x, p = threadIdx.x;
    const int px = ((t >> 5) * 8 + (p >> 3)) * W + (t & 31) * 8 + (p & 7);
    const bool clear = orig[4 * (size_t)px + 3] == 0;
    const int m = map[px];
    chars[t * 64 + p] = (clear || m == zero_at) ? (uint8_t)0 : (uint8_t)(m + 1);
    const unsigned long long any = __ballot(clear);
    if (p == 0) pinned[t] = any != 0ull ? 1 : 0;
}

// rep(t) and flip_of(t): the lowest (u, f), u <= t, with c_t == flip_f(c_u) — u = t, f = 0 always qualifies.  A character is
// eight rows of eight bytes: a horizontal flip reverses a row's bytes, a vertical one the rows.  grid = tiles, block 256:
// the threads share the tiles below t.
__global__ __launch_bounds__(256) void k_char_classes(const uint8_t *__restrict__ chars, uint16_t *__restrict__ rep, uint8_t *__restrict__ flip) {
    __shared__ unsigned long long s_red[4];
    const int t = blockIdx.x;
    const unsigned long long *C = reinterpret_cast<const unsigned long long *>(chars);
    unsigned long long mine[8];
#pragma unroll
    for (int y = 0; y < 8; y++) mine[y] = C[t * 8 + y];
    unsigned long long best = (unsigned long long)t << 2;
    for (int u = threadIdx.x; u < t; u += 256) {
        unsigned long long o[8];
#pragma unroll
        for (int y = 0; y < 8; y++) o[y] = C[u * 8 + y];
#pragma unroll
        for (int f = 3; f >= 0; f--) {
            bool eq = true;
#pragma unroll
            for (int y = 0; y < 8; y++) {
                unsigned long long r = o[(f & 2) ? 7 - y : y];
                if (f & 1) r = __builtin_bswap64(r);
                eq = eq && mine[y] == r;
            }
            const unsigned long long k = ((unsigned long long)u << 2) | (unsigned)f;
            if (eq && k < best) best = k;
        }
    }
    best = block_min_u64<4>(best, s_red);
    if (threadIdx.x == 0) { rep[t] = (uint16_t)(best >> 2); flip[t] = (uint8_t)(best & 3); }
}

// Class sizes (csize[t] = tiles in t's class) and U.  One block of 1024 threads, a thread per tile.
__global__ __launch_bounds__(1024) void k_char_count(const uint16_t *__restrict__ rep, int ntile, uint16_t *__restrict__ csize, CharInfo *__restrict__ info) {
    __shared__ unsigned int s_cnt[1024];
    const int t = threadIdx.x;
    s_cnt[t] = 0;
    __syncthreads();
    const int r = t < ntile ? (int)rep[t] : 0;
    if (t < ntile) atomicAdd(&s_cnt[r], 1u);
    const int u = __syncthreads_count(t < ntile && r == t);
    if (t < ntile) csize[t] = (uint16_t)s_cnt[r];
    if (t == 0) info->unique = (uint32_t)u;
}

// The proxy costs of one recipient's candidates and the K lowest packed keys among them.  grid = tiles, block 256.
// A recipient is unpinned and alone in its class; its donors are the unpinned class representatives other than itself.
// key[pixel][map value] (dynamic LDS, 64 * sub_size words) holds the remap's integer distance between the tile's ORIGINAL
// pixel and the entry of the tile's own subpalette, so a candidate costs 64 LDS reads addressed by the donor's character.
// Every thread keeps the keys of its four donors (16 candidates) in registers; K rounds of a block minimum pick the list.
// part[t][0 .. 63]: the list, ascending, kCharNone behind its end.
__global__ __launch_bounds__(256) void k_merge_proxy(const uint8_t *__restrict__ orig, int W, const uint8_t *__restrict__ chars, const uint8_t *__restrict__ pinned, const uint16_t *__restrict__ rep,
                                                    const uint16_t *__restrict__ csize, const uint8_t *__restrict__ tile_pal, const uint32_t *__restrict__ pal_rgb8, int S, int zero_at, int ntile,
                                                    int K, unsigned long long *__restrict__ part) {
    extern __shared__ uint32_t s_key[];
    __shared__ unsigned long long s_red[4], s_out[kCharShort]; // (with the largest table, 64 * 253 words, 65,312 bytes of the 64 KB a block may take)
    const int t = blockIdx.x, tid = threadIdx.x;
    unsigned long long *out = part + (size_t)t * kCharShort;
    if (pinned[t] || csize[t] != 1) { // (the same for the whole block)
        if (tid < kCharShort) out[tid] = kCharNone;
        return;
    }
    const int base = (int)tile_pal[t] * S;
    for (int e = tid; e < 64 * S; e += 256) {
        const int p = e / S, v = e - p * S;
        const int px = ((t >> 5) * 8 + (p >> 3)) * W + (t & 31) * 8 + (p & 7);
        s_key[e] = red_mean_key(pal_rgb8[base + v], reinterpret_cast<const uint32_t *>(orig)[px] & 0x00ffffffu);
    }
    __syncthreads();
    const int zero_v = zero_at >= 0 ? zero_at : 0; // (without a backdrop an unpinned tile holds no 0)
    unsigned long long keys[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int b = tid + 256 * i;
        const bool ok = b < ntile && b != t && rep[b < ntile ? b : 0] == b && !pinned[b < ntile ? b : 0];
        unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        if (ok) {
            const uint32_t *cw = reinterpret_cast<const uint32_t *>(chars) + b * 16;
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0; // a row's eight keys stay below 2^32 (8 * 299,505,150)
            for (int w = 0; w < 16; w++) {
                const uint32_t word = cw[w];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int ch = (int)((word >> (8 * k)) & 0xffu), q = 4 * w + k; // b's pixel q lands on t's pixel q ^ mask
                    int v = ch ? ch - 1 : zero_v;
                    v = v < S ? v : S - 1;
                    a0 += s_key[q * S + v]; a1 += s_key[(q ^ 7) * S + v]; a2 += s_key[(q ^ 56) * S + v]; a3 += s_key[(q ^ 63) * S + v];
                }
                if (w & 1) { c0 += a0; c1 += a1; c2 += a2; c3 += a3; a0 = a1 = a2 = a3 = 0; }
            }
        }
        keys[4 * i + 0] = ok ? merge_key(c0, t, b, 0) : kCharNone;
        keys[4 * i + 1] = ok ? merge_key(c1, t, b, 1) : kCharNone;
        keys[4 * i + 2] = ok ? merge_key(c2, t, b, 2) : kCharNone;
        keys[4 * i + 3] = ok ? merge_key(c3, t, b, 3) : kCharNone;
    }
    int cnt = 0;
    unsigned long long lo = 0; // the keys differ from one another (t, b, f): the next one is the least at or above lo
    for (int r = 0; r < K; r++) {
        unsigned long long m = kCharNone;
#pragma unroll
        for (int i = 0; i < 16; i++) if (keys[i] >= lo && keys[i] < m) m = keys[i];
        m = block_min_u64<4>(m, s_red);
        if (m == kCharNone) break;
        if (tid == 0) s_out[r] = m;
        lo = m + 1; cnt = r + 1;
    }
    __syncthreads();
    if (tid < kCharShort) out[tid] = tid < cnt ? s_out[tid] : kCharNone;
}

// The K lowest keys of the blocks' lists: a merge of ntile sorted lists, a thread per list.  One block of 1024 threads.
__global__ __launch_bounds__(1024) void k_merge_topk(const unsigned long long *__restrict__ part, int ntile, int K, unsigned long long *__restrict__ keys, CharInfo *__restrict__ info) {
    __shared__ unsigned long long s_red[16], s_out[kCharShort];
    const int tid = threadIdx.x;
    int pos = 0, cnt = 0;
    for (int r = 0; r < K; r++) {
        const unsigned long long mine = (tid < ntile && pos < kCharShort) ? part[(size_t)tid * kCharShort + pos] : kCharNone;
        const unsigned long long m = block_min_u64<16>(mine, s_red);
        if (m == kCharNone) break;
        if (mine == m) { pos++; s_out[r] = m; } // one owner: the keys differ
        cnt = r + 1;
    }
    __syncthreads();
    if (tid < kCharShort) keys[tid] = tid < cnt ? s_out[tid] : kCharNone;
    if (tid == 0) info->nshort = (uint32_t)cnt;
}

// A candidate's palette_map: the stored map with tile t's 64 pixels taken from tile b under flip f; and the candidate's
// (tile, subpalette) pair for k_move_full — the tile keeps its subpalette.  grid = candidates, block 256.
__global__ __launch_bounds__(256) void k_merge_maps(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ base_map, const uint8_t *__restrict__ tile_pal, int W, int npx,
                                                   uint8_t *__restrict__ lmaps, uint16_t *__restrict__ tiles, uint8_t *__restrict__ subs) {
    const int cand = blockIdx.x, tid = threadIdx.x;
    const uint32_t k = (uint32_t)(keys[cand] & 0x3fffffu);
    const int t = (int)(k >> 12), b = (int)((k >> 2) & 1023u), f = (int)(k & 3u);
    uint8_t mine = 0; int px = 0;
    const bool inside = t < (npx >> 6) && b < (npx >> 6); // (the host hands over tiles of the image only)
    if (tid < 64 && inside) {
        const int x = tid & 7, y = tid >> 3, sx = (f & 1) ? 7 - x : x, sy = (f & 2) ? 7 - y : y;
        px = ((t >> 5) * 8 + y) * W + (t & 31) * 8 + x;
        mine = base_map[((b >> 5) * 8 + sy) * W + (b & 31) * 8 + sx];
    }
    copy_map_sync<256>(lmaps + (size_t)cand * npx, base_map, npx); // the copy of the tile's rows is in place before its 64 bytes are replaced
    if (tid < 64 && inside) lmaps[(size_t)cand * npx + px] = mine;
    if (tid == 0) { tiles[cand] = (uint16_t)t; subs[cand] = tile_pal[t]; }
}

// The step's decision: the lowest (error, rank) of the n <= 64 scored candidates — a NaN never wins — becomes the image's:
// its tile is rewritten in the stored map, its error is the incumbent.  One block, one wave.  Without a winner (all NaN)
// nothing changes and the record says rank 255.
__global__ __launch_bounds__(64) void k_merge_commit(const double *__restrict__ errs, const unsigned long long *__restrict__ keys, int n, const uint8_t *__restrict__ lmaps, int npx, int W,
                                                    uint8_t *__restrict__ map, double *__restrict__ inc_err, MergeLog *__restrict__ log) {
    const int j = threadIdx.x;
    double e = j < n ? errs[j] : 0.0;
    int w = (j < n && e == e) ? j : -1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double e2 = __shfl_xor(e, o, 64);
        const int w2 = __shfl_xor(w, o, 64);
        if (w2 >= 0 && (w < 0 || e2 < e || (e2 == e && w2 < w))) { e = e2; w = w2; }
    }
    MergeLog r{};
    if (w < 0) {
        r.error = __longlong_as_double(0x7ff8000000000000ll); r.rank = 255;
        if (j == 0) *log = r;
        return;
    }
    const unsigned long long key = keys[w];
    const int t = (int)((key >> 12) & 1023u);
    const int px = ((t >> 5) * 8 + (j >> 3)) * W + (t & 31) * 8 + (j & 7);
    map[px] = lmaps[(size_t)w * npx + px];
    if (j == 0) {
        r.error = e; r.cost = key >> 22; r.tile = (uint16_t)t; r.donor = (uint16_t)((key >> 2) & 1023u); r.flip = (uint8_t)(key & 3u); r.rank = (uint8_t)w; r.unique = 0;
        *log = r; *inc_err = e;
    }
}

// ---- the refit: each shared character fitted to all the tiles that use it -----------------------------------------------------
//
// A class of the snapshot (rep[], flip[] as k_char_classes left them) is ELIGIBLE if it has at least two members and none is
// pinned.  Its FIT gives every position q of the representative's orientation the map value v that costs least over all
// members, each read through its own subpalette and flip: cost(q, v) = sum over members m of red_mean_key(original pixel
// q ^ mask(flip[m]) of tile m, entry tile_pal[m] * S + v), ties to the lowest v.  The candidate map (k_refit_maps) goes through
// the map-reading scorer as a merge does, and k_refit_commit applies the window's first call that beats the incumbent.

struct RefitFit { unsigned long long gain; uint16_t members; uint8_t eligible, differs; uint32_t pad; };      // per tile; all zero unless the tile represents an eligible class
struct RefitLog { double error; unsigned long long gain; uint16_t rep, members; uint8_t changed, scored, pad[2]; }; // = snesimage_refit_result
struct RefitWinRes { int32_t consumed, accepted; };  // calls that took effect; the one that accepted (-1: none)

__device__ inline int flip_mask(int f) { return ((f & 1) ? 7 : 0) | ((f & 2) ? 56 : 0); }
__device__ inline int tile_px(int t, int p, int W) { return ((t >> 5) * 8 + (p >> 3)) * W + (t & 31) * 8 + (p & 7); }

// The fit of the class tile t represents.  grid = tiles, block 256: thread (q = tid & 63, lane group = tid >> 6) takes the
// values v = lane group, + 4, ... of position q, sums each over the members in 64 bits (a key stays below 2^29, a class has at
// most 1,024 members: below 2^39) and keeps the lowest (cost << 8 | v); the four lane groups meet through LDS.
// The members' tile, flip and subpalette are listed in LDS (4 KB); their original pixels come from L2.
__global__ __launch_bounds__(256) void k_refit_fit(const uint8_t *__restrict__ orig, const uint8_t *__restrict__ map, int W, const uint8_t *__restrict__ pinned, const uint16_t *__restrict__ rep,
                                                  const uint8_t *__restrict__ flip, const uint16_t *__restrict__ csize, const uint8_t *__restrict__ tile_pal, const uint32_t *__restrict__ pal_rgb8,
                                                  int S, int ncol, int ntile, uint8_t *__restrict__ fits, RefitFit *__restrict__ fit) {
    __shared__ uint16_t s_tile[1024];
    __shared__ uint8_t s_mask[1024], s_sub[1024];
    __shared__ uint32_t s_pal[256];
    __shared__ unsigned long long s_best[4][64], s_cur[64];
    __shared__ int s_n, s_pin;
    const int t = blockIdx.x, tid = threadIdx.x;
    if ((int)rep[t] != t || csize[t] < 2) { // (the same for the whole block)
        if (tid == 0) { RefitFit z{}; fit[t] = z; }
        if (tid < 64) fits[t * 64 + tid] = 0;
        return;
    }
    if (tid == 0) { s_n = 0; s_pin = 0; }
    for (int e = tid; e < ncol && e < 256; e += 256) s_pal[e] = pal_rgb8[e];
    __syncthreads();
    for (int u = tid; u < ntile; u += 256) {
        if ((int)rep[u] != t) continue;
        const int i = atomicAdd(&s_n, 1); // (the order of the list does not matter: the sums are integers)
        if (i < 1024) { s_tile[i] = (uint16_t)u; s_mask[i] = (uint8_t)flip_mask(flip[u]); s_sub[i] = tile_pal[u]; }
        if (pinned[u]) s_pin = 1;
    }
    __syncthreads();
    const int n = s_n < 1024 ? s_n : 1024;
    if (s_pin) { // a pinned member: the class is never changed
        if (tid == 0) { RefitFit z{}; fit[t] = z; }
        if (tid < 64) fits[t * 64 + tid] = 0;
        return;
    }
    const int q = tid & 63, lg = tid >> 6;
    const int cur = map[tile_px(t, q, W)];
    const int cur_v = cur < S ? cur : S - 1; // (a stored map holds values below S)
    unsigned long long best = kCharNone;
    for (int v = lg; v < S; v += 4) {
        unsigned long long cost = 0;
        for (int i = 0; i < n; i++) {
            const int e = (int)s_sub[i] * S + v;
            const uint32_t px = reinterpret_cast<const uint32_t *>(orig)[tile_px((int)s_tile[i], q ^ (int)s_mask[i], W)] & 0x00ffffffu;
            cost += red_mean_key(s_pal[e < 256 ? e : 255], px);
        }
        const unsigned long long k = (cost << 8) | (unsigned)v;
        best = k < best ? k : best; // v ascends: the lowest v of equal costs stays
        if (v == cur_v) s_cur[q] = cost;
    }
    s_best[lg][q] = best;
    __syncthreads();
    if (tid < 64) { // one wave
        unsigned long long m = s_best[0][q];
#pragma unroll
        for (int i = 1; i < 4; i++) m = s_best[i][q] < m ? s_best[i][q] : m;
        const int fitted = (int)(m & 0xffu);
        unsigned long long g = s_cur[q] - (m >> 8);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) g += __shfl_xor(g, o, 64);
        const unsigned long long diff = __ballot(fitted != cur);
        fits[t * 64 + q] = (uint8_t)fitted;
        if (q == 0) { RefitFit r{}; r.gain = g; r.members = (uint16_t)n; r.eligible = 1; r.differs = diff != 0ull ? 1 : 0; fit[t] = r; }
    }
}

// A refit candidate's palette_map: the stored map with every member m of class reps[cand] rewritten to
// fitted[p ^ mask(flip[m])]; and the pair (rep, its own subpalette) for k_move_full, which so substitutes nothing.
// grid = candidates, block 256: a wave per member tile, a lane per pixel.
__global__ __launch_bounds__(256) void k_refit_maps(const uint16_t *__restrict__ reps, const uint8_t *__restrict__ base_map, const uint16_t *__restrict__ rep, const uint8_t *__restrict__ flip,
                                                   const uint8_t *__restrict__ fits, const uint8_t *__restrict__ tile_pal, int W, int npx, uint8_t *__restrict__ lmaps,
                                                   uint16_t *__restrict__ tiles, uint8_t *__restrict__ subs) {
    const int cand = blockIdx.x, tid = threadIdx.x, ntile = npx >> 6;
    int r = reps[cand];
    r = r < ntile ? r : 0; // (the host hands over representatives of the image only)
    copy_map_sync<256>(lmaps + (size_t)cand * npx, base_map, npx); // the copy is in place before the members' bytes are replaced
    const int p = tid & 63;
    for (int u = tid >> 6; u < ntile; u += 4) {
        if ((int)rep[u] != r) continue; // (the same for the whole wave)
        lmaps[(size_t)cand * npx + tile_px(u, p, W)] = fits[r * 64 + (p ^ flip_mask(flip[u]))];
    }
    if (tid == 0) { tiles[cand] = (uint16_t)r; subs[cand] = tile_pal[r]; }
}

// The window's refit calls in order (lib.rs:216-219 per call: taken iff its error is below the incumbent, strict): every call up
// to and including the first that accepts is logged; that one's map and error become the image's.  One block.
__global__ __launch_bounds__(1024) void k_refit_commit(const double *__restrict__ errs, const uint16_t *__restrict__ reps, int ncalls, const RefitFit *__restrict__ fit,
                                                      const uint8_t *__restrict__ lmaps, int npx, uint8_t *__restrict__ map, double *__restrict__ inc_err, RefitLog *__restrict__ log,
                                                      RefitWinRes *__restrict__ res) {
    __shared__ int s_win;
    if (threadIdx.x == 0) {
        const double inc = *inc_err;
        int win = -1, used = ncalls;
        for (int i = 0; i < ncalls && win < 0; i++) {
            const double e = errs[i];
            const RefitFit f = fit[reps[i]];
            const bool take = e < inc;
            RefitLog r{};
            r.error = take ? e : inc; r.gain = f.gain; r.rep = reps[i]; r.members = f.members; r.changed = take ? 1 : 0; r.scored = 1;
            log[i] = r;
            if (take) { win = i; used = i + 1; }
        }
        res->consumed = used; res->accepted = win;
        s_win = win;
    }
    __syncthreads(); // the records are written before the state changes hands
    const int win = s_win;
    if (win < 0) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(lmaps + (size_t)win * npx); // (outside the members' tiles it is the stored map itself)
    uint4 *dst = reinterpret_cast<uint4 *>(map);
    for (int i = threadIdx.x; i < npx / 16; i += 1024) dst[i] = src[i];
    if (threadIdx.x == 0) *inc_err = errs[win];
}

} // namespace snes
