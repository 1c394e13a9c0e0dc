// snesimage_amd/csrc/kernels_char_set.hpp — the character budget across the members of a shared-palette set
// (shared_char_host.inc; definition: include/snesimage_hip.h, "character budget of a set").
//
// The members' tiles are numbered as GLOBAL TILES g = member * ntile + tile, at most kSetTiles of them.  Characters and pinned
// flags of all members go into one G x 64 array (ks_char_build, through a device table of the members' pointers), on which
// k_char_classes (kernels_char.hpp) runs as it is; ks_char_count sizes the classes.  ks_merge_proxy lists each recipient's K
// cheapest candidates over the representatives of ALL members, ks_merge_topk merges the G lists into the shortlist and splits
// it by recipient member, ks_merge_maps writes a member's candidates into that member's tile workspace, and ks_merge_commit
// compares the members' error vectors by (d, rank), d = e - the recipient member's incumbent.
// All kernels are wave64, none takes scratch; a block's waves meet through LDS (at most 65,312 bytes: ks_merge_proxy).
#pragma once
#include "kernels_char.hpp"

namespace snes {

constexpr int kSetTiles = 8192; // most global tiles: 13 bits each for recipient and donor beside a cost below 2^35
// one member of the set as the kernels see it.  errs, lmaps: the member's tile workspace (null until a call scores)
struct SetMember { const uint8_t *orig; uint8_t *map; const uint8_t *tile_pal; double *inc_err; const double *errs; const uint8_t *lmaps; };
struct SetMergeLog { double error, member_error; unsigned long long cost; uint16_t member, tile, donor_member, donor, unique; uint8_t flip, rank; uint8_t pad[4]; }; // = snesimage_shared_merge_result

// cost << 28 | gt << 15 | gb << 2 | f: orders as the tuple (cost, gt, gb, f) does (gt, gb < 8192; cost <= 64 * 299,505,150 < 2^35)
__device__ inline unsigned long long set_merge_key(unsigned long long cost, uint32_t gt, uint32_t gb, uint32_t f) { return (cost << 28) | ((unsigned long long)gt << 15) | (gb << 2) | f; }
__device__ inline int set_key_recipient(unsigned long long k) { return (int)((k >> 15) & 8191u); }
__device__ inline int set_key_donor(unsigned long long k) { return (int)((k >> 2) & 8191u); }

// Characters and pinned flags of every member.  grid = global tiles, block = the tile's 64 pixels (one wave).
__global__ __launch_bounds__(64) void ks_char_build(const SetMember *__restrict__ tab, int ntile, int W, uint8_t *__restrict__ chars, uint8_t *__restrict__ pinned) {
    const int g = blockIdx.x, p = threadIdx.x, m = g / ntile, t = g - m * ntile;
    const uint8_t *orig = tab[m].orig, *map = tab[m].map;
    const int px = tile_px(t, p, W);
    const bool clear = orig[4 * (size_t)px + 3] == 0;
    chars[(size_t)g * 64 + p] = clear ? (uint8_t)0 : (uint8_t)(map[px] + 1);
    const unsigned long long any = __ballot(clear);
    if (p == 0) pinned[g] = any != 0ull ? 1 : 0;
}

// Class sizes (csize[g] = tiles in g's class) and U for G <= kSetTiles.  One block of 1024 threads, an LDS counter per tile
// (32 KB), up to eight tiles per thread.
__global__ __launch_bounds__(1024) void ks_char_count(const uint16_t *__restrict__ rep, int G, uint16_t *__restrict__ csize, CharInfo *__restrict__ info) {
    __shared__ unsigned int s_cnt[kSetTiles];
    __shared__ unsigned int s_u;
    const int tid = threadIdx.x;
    for (int g = tid; g < kSetTiles; g += 1024) s_cnt[g] = 0;
    if (tid == 0) s_u = 0;
    __syncthreads();
    unsigned int u = 0;
    for (int g = tid; g < G; g += 1024) {
        int r = (int)rep[g];
        r = r < kSetTiles ? r : 0; // (k_char_classes writes rep[g] <= g)
        atomicAdd(&s_cnt[r], 1u);
        u += r == g ? 1u : 0u;
    }
    if (u) atomicAdd(&s_u, u);
    __syncthreads();
    for (int g = tid; g < G; g += 1024) { const int r = (int)rep[g]; csize[g] = (uint16_t)s_cnt[r < kSetTiles ? r : 0]; }
    if (tid == 0) info->unique = s_u;
}

// a thread's four lowest keys, ascending; over: a key at or above the bound was left out
__device__ inline void keep4(unsigned long long k, unsigned long long &b0, unsigned long long &b1, unsigned long long &b2, unsigned long long &b3, bool &over) {
    if (k >= b3) { over = true; return; }
    if (b3 != kCharNone) over = true;
    b3 = k;
    if (b3 < b2) { const unsigned long long x = b2; b2 = b3; b3 = x; }
    if (b2 < b1) { const unsigned long long x = b1; b1 = b2; b2 = x; }
    if (b1 < b0) { const unsigned long long x = b0; b0 = b1; b1 = x; }
}

// The proxy costs of one global recipient's candidates and the K lowest packed keys among them.  grid = global tiles, block 256.
// A recipient is unpinned and alone in its set-wide class; its donors are the unpinned class representatives of the whole set
// other than itself.  key[pixel][map value] (dynamic LDS, 64 * S words) is the recipient member's, as in k_merge_proxy: the
// recipient's ORIGINAL pixels against its own subpalette of the shared palette.  Thread i takes the donors i, i + 256, ... of
// all G and keeps the four lowest of its keys at or above its bound in registers; K rounds of a block minimum pick the list,
// and a thread whose four are used up while it left keys out goes through its donors again from its last key on.
// part[g][0 .. 63]: the list, ascending, kCharNone behind its end.
__global__ __launch_bounds__(256) void ks_merge_proxy(const SetMember *__restrict__ tab, int ntile, int W, const uint8_t *__restrict__ chars, const uint8_t *__restrict__ pinned,
                                                     const uint16_t *__restrict__ rep, const uint16_t *__restrict__ csize, const uint32_t *__restrict__ pal_rgb8, int S, int G, int K,
                                                     unsigned long long *__restrict__ part) {
    extern __shared__ uint32_t s_key[];
    __shared__ unsigned long long s_red[4], s_out[kCharShort]; // (with the largest table, 64 * 253 words, 65,312 bytes of the 64 KB a block may take)
    const int g = blockIdx.x, tid = threadIdx.x;
    unsigned long long *out = part + (size_t)g * kCharShort;
    if (pinned[g] || csize[g] != 1) { // (the same for the whole block)
        if (tid < kCharShort) out[tid] = kCharNone;
        return;
    }
    const int m = g / ntile, t = g - m * ntile;
    const uint8_t *orig = tab[m].orig;
    const int base = (int)tab[m].tile_pal[t] * S;
    for (int e = tid; e < 64 * S; e += 256) {
        const int p = e / S, v = e - p * S;
        s_key[e] = red_mean_key(pal_rgb8[base + v], reinterpret_cast<const uint32_t *>(orig)[tile_px(t, p, W)] & 0x00ffffffu);
    }
    __syncthreads();
    unsigned long long b0 = kCharNone, b1 = kCharNone, b2 = kCharNone, b3 = kCharNone;
    bool over = false;
    auto fill = [&](unsigned long long lo) { // the four lowest of this thread's keys at or above lo
        b0 = b1 = b2 = b3 = kCharNone; over = false;
        for (int b = tid; b < G; b += 256) {
            if (b == g || (int)rep[b] != b || pinned[b]) continue;
            const uint32_t *cw = reinterpret_cast<const uint32_t *>(chars) + (size_t)b * 16;
            unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0; // a row's eight keys stay below 2^32 (8 * 299,505,150)
            for (int w = 0; w < 16; w++) {
                const uint32_t word = cw[w];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int ch = (int)((word >> (8 * k)) & 0xffu), q = 4 * w + k; // b's pixel q lands on g's pixel q ^ mask
                    int v = ch ? ch - 1 : 0;                                          // (an unpinned tile of a set holds no 0)
                    v = v < S ? v : S - 1;
                    a0 += s_key[q * S + v]; a1 += s_key[(q ^ 7) * S + v]; a2 += s_key[(q ^ 56) * S + v]; a3 += s_key[(q ^ 63) * S + v];
                }
                if (w & 1) { c0 += a0; c1 += a1; c2 += a2; c3 += a3; a0 = a1 = a2 = a3 = 0; }
            }
            const unsigned long long k0 = set_merge_key(c0, g, b, 0), k1 = set_merge_key(c1, g, b, 1), k2 = set_merge_key(c2, g, b, 2), k3 = set_merge_key(c3, g, b, 3);
            if (k0 >= lo) keep4(k0, b0, b1, b2, b3, over);
            if (k1 >= lo) keep4(k1, b0, b1, b2, b3, over);
            if (k2 >= lo) keep4(k2, b0, b1, b2, b3, over);
            if (k3 >= lo) keep4(k3, b0, b1, b2, b3, over);
        }
    };
    fill(0ull);
    int cnt = 0;
    unsigned long long lo = 0; // this thread's keys differ from one another and leave in ascending order: the rest lie at or above lo
    for (int r = 0; r < K; r++) {
        if (b0 == kCharNone && over) fill(lo);
        const unsigned long long mn = block_min_u64<4>(b0, s_red);
        if (mn == kCharNone) break;
        if (b0 == mn) { lo = mn + 1; b0 = b1; b1 = b2; b2 = b3; b3 = kCharNone; } // one owner: the keys differ
        if (tid == 0) s_out[r] = mn;
        cnt = r + 1;
    }
    __syncthreads();
    if (tid < kCharShort) out[tid] = tid < cnt ? s_out[tid] : kCharNone;
}

// The K lowest keys of the G sorted lists, and their stable split by recipient member.  One block of 1024 threads; thread i
// owns the lists i, i + 1024, ... (eight at most) and keeps their heads in registers.
// skeys[0 .. 63]: the shortlist in rank order (kCharNone behind its end); spos[r]: rank r's place among its member's
// candidates; mkeys[m * 64 + j]: member m's candidates in rank order; mcount[m]: how many; info->nshort.
__global__ __launch_bounds__(1024) void ks_merge_topk(const unsigned long long *__restrict__ part, int G, int ntile, int F, int K, unsigned long long *__restrict__ skeys, uint8_t *__restrict__ spos,
                                                     unsigned long long *__restrict__ mkeys, uint32_t *__restrict__ mcount, CharInfo *__restrict__ info) {
    __shared__ unsigned long long s_red[16], s_out[kCharShort];
    const int tid = threadIdx.x;
    unsigned long long head[8];
    int pos[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { const int l = tid + 1024 * i; pos[i] = 0; head[i] = l < G ? part[(size_t)l * kCharShort] : kCharNone; }
    int cnt = 0;
    for (int r = 0; r < K; r++) {
        unsigned long long mine = kCharNone;
#pragma unroll
        for (int i = 0; i < 8; i++) mine = head[i] < mine ? head[i] : mine;
        const unsigned long long mn = block_min_u64<16>(mine, s_red);
        if (mn == kCharNone) break;
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (head[i] == mn) { // one owner: the keys differ
                pos[i]++;
                head[i] = pos[i] < kCharShort ? part[(size_t)(tid + 1024 * i) * kCharShort + pos[i]] : kCharNone;
                s_out[r] = mn;
            }
        cnt = r + 1;
    }
    __syncthreads();
    if (tid < kCharShort) {
        const unsigned long long key = tid < cnt ? s_out[tid] : kCharNone;
        skeys[tid] = key;
        if (tid < cnt) {
            const int m = set_key_recipient(key) / ntile;
            int before = 0;
            for (int j = 0; j < tid; j++) before += set_key_recipient(s_out[j]) / ntile == m ? 1 : 0;
            spos[tid] = (uint8_t)before;
            if (m < F) mkeys[(size_t)m * kCharShort + before] = key;
        } else spos[tid] = 0;
    }
    for (int m = tid; m < F; m += 1024) {
        uint32_t n = 0;
        for (int j = 0; j < cnt; j++) n += set_key_recipient(s_out[j]) / ntile == m ? 1u : 0u;
        mcount[m] = n;
    }
    if (tid == 0) info->nshort = (uint32_t)cnt;
}

// The palette_maps of one member's candidates, into that member's tile workspace: the member's stored map with the tile's 64
// bytes taken from the donor's tile of the DONOR's member's stored map under flip f; and the (tile, subpalette) pair as
// k_merge_maps writes it — the tile keeps its subpalette.  grid = the member's candidates, block 256.
__global__ __launch_bounds__(256) void ks_merge_maps(const unsigned long long *__restrict__ keys, const SetMember *__restrict__ tab, int member, int ntile, int F, int W, int npx,
                                                    uint8_t *__restrict__ lmaps, uint16_t *__restrict__ tiles, uint8_t *__restrict__ subs) {
    const int cand = blockIdx.x, tid = threadIdx.x;
    const unsigned long long key = keys[cand];
    const int gt = set_key_recipient(key), gb = set_key_donor(key), f = (int)(key & 3u);
    const int t = gt - member * ntile, mb = gb / ntile, b = gb - mb * ntile;
    const bool inside = t >= 0 && t < ntile && mb < F; // (the host and ks_merge_topk hand over this member's recipients only)
    const uint8_t *base_map = tab[member].map;
    uint8_t mine = 0; int px = 0;
    if (tid < 64 && inside) {
        const int x = tid & 7, y = tid >> 3, sx = (f & 1) ? 7 - x : x, sy = (f & 2) ? 7 - y : y;
        px = tile_px(t, tid, W);
        mine = tab[mb].map[((b >> 5) * 8 + sy) * W + (b & 31) * 8 + sx];
    }
    copy_map_sync<256>(lmaps + (size_t)cand * npx, base_map, npx); // the copy of the tile's rows is in place before its 64 bytes are replaced
    if (tid < 64 && inside) lmaps[(size_t)cand * npx + px] = mine;
    if (tid == 0) { tiles[cand] = (uint16_t)(inside ? t : 0); subs[cand] = tab[member].tile_pal[inside ? t : 0]; }
}

// The step's decision over the members' error vectors: candidate of rank r was scored as number spos[r] of its recipient's
// member; d = e - that member's incumbent (one binary64 subtraction); the lowest (d, rank) wins, a NaN never.  The winner's 64
// bytes go into its member's stored map, its error becomes that member's incumbent, and the record carries E = the members'
// incumbents summed in member order.  One block, one wave.  Without a winner nothing changes and the record says rank 255.
__global__ __launch_bounds__(64) void ks_merge_commit(const unsigned long long *__restrict__ skeys, const uint8_t *__restrict__ spos, int n, const SetMember *__restrict__ tab, int ntile, int F,
                                                     int npx, int W, SetMergeLog *__restrict__ log) {
    const int j = threadIdx.x;
    double d = 0.0;
    int w = -1;
    if (j < n) {
        const int m = set_key_recipient(skeys[j]) / ntile;
        if (m < F) {
            const double e = tab[m].errs[spos[j]];
            d = e - *tab[m].inc_err;
            w = d == d ? j : -1;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double d2 = __shfl_xor(d, o, 64);
        const int w2 = __shfl_xor(w, o, 64);
        if (w2 >= 0 && (w < 0 || d2 < d || (d2 == d && w2 < w))) { d = d2; w = w2; }
    }
    SetMergeLog r{};
    if (w < 0) {
        r.error = __longlong_as_double(0x7ff8000000000000ll); r.member_error = r.error; r.rank = 255;
        if (j == 0) *log = r;
        return;
    }
    const unsigned long long key = skeys[w];
    const int gt = set_key_recipient(key), gb = set_key_donor(key), m = gt / ntile, t = gt - m * ntile, k = (int)spos[w];
    const double e = tab[m].errs[k];
    const int px = tile_px(t, j, W);
    tab[m].map[px] = tab[m].lmaps[(size_t)k * npx + px];
    if (j == 0) {
        double E = 0.0;
        for (int i = 0; i < F; i++) { const double v = i == m ? e : *tab[i].inc_err; E = i == 0 ? v : E + v; } // member order, as snesimage_shared_error sums
        r.error = E; r.member_error = e; r.cost = key >> 28; r.member = (uint16_t)m; r.tile = (uint16_t)t; r.donor_member = (uint16_t)(gb / ntile); r.donor = (uint16_t)(gb % ntile);
        r.unique = 0; r.flip = (uint8_t)(key & 3u); r.rank = (uint8_t)w;
        *log = r; *tab[m].inc_err = e;
    }
}

// ---- the refit across the members of a set: each shared character fitted to all the tiles of all members that use it ---------
//
// The snapshot is the set-wide classes as k_char_classes left them (rep[], flip[] over the G global tiles).  ks_refit_fit fits
// every eligible class at once; the host, which reads the fits anyway to log the skipped calls, builds the small tables of a
// window (which call is scored as which candidate of which member) and uploads them; ks_refit_maps writes one member's
// candidates into that member's tile workspace; ks_refit_commit decides on E = the members' errors summed in member order.

constexpr int kSetRefitMembers = 256; // most members of a set with G <= kSetTiles (an image has at least 32 tiles)
struct SetRefitFit { unsigned long long gain; uint16_t members, touched; uint8_t eligible, differs; uint16_t pad; }; // per global tile; all zero unless it represents an eligible class
struct SetRefitLog { double error; unsigned long long gain; uint16_t rep, members, touched; uint8_t changed, scored; }; // = snesimage_shared_refit_result
struct SetRefitCall { uint16_t rep, first, count, pad; };  // a window's call: class rep, scored as slots[first .. first + count), ascending member
struct SetRefitSlot { uint16_t member, slot; };              // touched member, and the candidate's number in that member's workspace

// The fit of the class global tile g represents.  grid = global tiles, block 256; thread (q = tid & 63, lane group = tid >> 6)
// as in k_refit_fit.  A class may hold every tile of the set, so a tile of the class is ONE word of the LDS list (32 KB):
// tile | member << 10 | mask << 18 | subpalette << 24 (tile < 1024, member < 256, mask < 64).  The sums are 64-bit integers
// (8,192 keys below 2^29: below 2^42), so the order of the list does not matter.  Static LDS: 38,440 bytes; no scratch.
__global__ __launch_bounds__(256) void ks_refit_fit(const SetMember *__restrict__ tab, int ntile, int W, const uint8_t *__restrict__ pinned, const uint16_t *__restrict__ rep,
                                                   const uint8_t *__restrict__ flip, const uint16_t *__restrict__ csize, const uint32_t *__restrict__ pal_rgb8, int S, int ncol, int G, int F,
                                                   uint8_t *__restrict__ fits, SetRefitFit *__restrict__ fit) {
    __shared__ uint32_t s_list[kSetTiles];
    __shared__ const uint8_t *s_orig[kSetRefitMembers];
    __shared__ uint32_t s_pal[256], s_touch[kSetRefitMembers / 32];
    __shared__ unsigned long long s_best[4][64], s_cur[64];
    __shared__ int s_n, s_pin;
    const int g = blockIdx.x, tid = threadIdx.x;
    if ((int)rep[g] != g || csize[g] < 2) { // (the same for the whole block)
        if (tid == 0) { SetRefitFit z{}; fit[g] = z; }
        if (tid < 64) fits[(size_t)g * 64 + tid] = 0;
        return;
    }
    if (tid == 0) { s_n = 0; s_pin = 0; }
    if (tid < kSetRefitMembers / 32) s_touch[tid] = 0;
    for (int e = tid; e < ncol && e < 256; e += 256) s_pal[e] = pal_rgb8[e];
    for (int m = tid; m < F && m < kSetRefitMembers; m += 256) s_orig[m] = tab[m].orig;
    __syncthreads();
    for (int u = tid; u < G; u += 256) {
        if ((int)rep[u] != g) continue;
        const int m = u / ntile, t = u - m * ntile;
        const int i = atomicAdd(&s_n, 1); // (the order of the list does not matter: the sums are integers)
        if (i < kSetTiles && m < kSetRefitMembers)
            s_list[i] = (uint32_t)t | ((uint32_t)m << 10) | ((uint32_t)flip_mask(flip[u]) << 18) | ((uint32_t)tab[m].tile_pal[t] << 24);
        if (m < kSetRefitMembers) atomicOr(&s_touch[m >> 5], 1u << (m & 31));
        if (pinned[u]) s_pin = 1;
    }
    __syncthreads();
    const int n = s_n < kSetTiles ? s_n : kSetTiles;
    if (s_pin) { // a pinned tile, in whichever member: the class is never changed
        if (tid == 0) { SetRefitFit z{}; fit[g] = z; }
        if (tid < 64) fits[(size_t)g * 64 + tid] = 0;
        return;
    }
    const int q = tid & 63, lg = tid >> 6;
    const int mg = g / ntile;
    const int cur = tab[mg].map[tile_px(g - mg * ntile, q, W)];
    const int cur_v = cur < S ? cur : S - 1; // (a stored map holds values below S)
    unsigned long long best = kCharNone;
    for (int v = lg; v < S; v += 4) {
        unsigned long long cost = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t w = s_list[i];
            const int e = (int)(w >> 24) * S + v;
            const uint32_t px = reinterpret_cast<const uint32_t *>(s_orig[(w >> 10) & 255u])[tile_px((int)(w & 1023u), q ^ (int)((w >> 18) & 63u), W)] & 0x00ffffffu;
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
        unsigned long long gn = s_cur[q] - (m >> 8);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) gn += __shfl_xor(gn, o, 64);
        const unsigned long long diff = __ballot(fitted != cur);
        fits[(size_t)g * 64 + q] = (uint8_t)fitted;
        if (q == 0) {
            int touched = 0;
#pragma unroll
            for (int i = 0; i < kSetRefitMembers / 32; i++) touched += __popc(s_touch[i]);
            SetRefitFit r{}; r.gain = gn; r.members = (uint16_t)n; r.touched = (uint16_t)touched; r.eligible = 1; r.differs = diff != 0ull ? 1 : 0;
            fit[g] = r;
        }
    }
}

// One member's refit candidates, into that member's tile workspace: the member's stored map with every tile of class
// reps[cand] THAT LIES IN THIS MEMBER rewritten to fitted[p ^ mask(flip)]; and the pair (tile 0, its own subpalette) for
// k_move_full, which so substitutes nothing.  grid = the member's candidates, block 256: a wave per tile, a lane per pixel.
__global__ __launch_bounds__(256) void ks_refit_maps(const uint16_t *__restrict__ reps, const SetMember *__restrict__ tab, int member, int ntile, int G, int W, int npx,
                                                    const uint16_t *__restrict__ rep, const uint8_t *__restrict__ flip, const uint8_t *__restrict__ fits, uint8_t *__restrict__ lmaps,
                                                    uint16_t *__restrict__ tiles, uint8_t *__restrict__ subs) {
    const int cand = blockIdx.x, tid = threadIdx.x;
    int r = reps[cand];
    r = r < G ? r : 0; // (the host hands over representatives of the set only)
    copy_map_sync<256>(lmaps + (size_t)cand * npx, tab[member].map, npx); // the copy is in place before the class's bytes are replaced
    const int p = tid & 63, g0 = member * ntile;
    for (int u = tid >> 6; u < ntile; u += 4) {
        if ((int)rep[g0 + u] != r) continue; // (the same for the whole wave)
        lmaps[(size_t)cand * npx + tile_px(u, p, W)] = fits[(size_t)r * 64 + (p ^ flip_mask(flip[g0 + u]))];
    }
    if (tid == 0) { tiles[cand] = 0; subs[cand] = tab[member].tile_pal[0]; }
}

// The window's refit calls in order.  E = the members' incumbents, E' = the same with a touched member's incumbent replaced by
// the error of its candidate, both summed in member order with plain + (as ks_commit and snesimage_shared_error sum); a call
// is taken iff E' < E, strict (lib.rs:216-219 on the joint error; a NaN never wins).  Every call up to and including the first
// that accepts is logged; then that one's maps and errors become the touched members'.  One block.
__global__ __launch_bounds__(1024) void ks_refit_commit(const SetRefitCall *__restrict__ calls, const SetRefitSlot *__restrict__ slots, int ncalls, const SetRefitFit *__restrict__ fit,
                                                       const SetMember *__restrict__ tab, int F, int npx, SetRefitLog *__restrict__ log, RefitWinRes *__restrict__ res) {
    __shared__ int s_win;
    if (threadIdx.x == 0) {
        double E = 0.0;
        for (int i = 0; i < F; i++) { const double v = *tab[i].inc_err; E = i == 0 ? v : E + v; }
        int win = -1, used = ncalls;
        for (int c = 0; c < ncalls && win < 0; c++) {
            const SetRefitCall call = calls[c];
            double E1 = 0.0;
            int k = 0;
            for (int i = 0; i < F; i++) {
                double v;
                if (k < (int)call.count && (int)slots[call.first + k].member == i) { v = tab[i].errs[slots[call.first + k].slot]; k++; }
                else v = *tab[i].inc_err;
                E1 = i == 0 ? v : E1 + v;
            }
            const SetRefitFit f = fit[call.rep];
            const bool take = E1 < E;
            SetRefitLog r{};
            r.error = take ? E1 : E; r.gain = f.gain; r.rep = call.rep; r.members = f.members; r.touched = f.touched; r.changed = take ? 1 : 0; r.scored = 1;
            log[c] = r;
            if (take) { win = c; used = c + 1; }
        }
        res->consumed = used; res->accepted = win;
        s_win = win;
    }
    __syncthreads(); // the records are written before the state changes hands
    const int win = s_win;
    if (win < 0) return;
    const SetRefitCall call = calls[win];
    for (int k = 0; k < (int)call.count; k++) {
        const SetRefitSlot sl = slots[call.first + k];
        const uint4 *src = reinterpret_cast<const uint4 *>(tab[sl.member].lmaps + (size_t)sl.slot * npx); // (outside the class's tiles it is the stored map itself)
        uint4 *dst = reinterpret_cast<uint4 *>(tab[sl.member].map);
        for (int i = threadIdx.x; i < npx / 16; i += 1024) dst[i] = src[i];
        if (threadIdx.x == 0) *tab[sl.member].inc_err = tab[sl.member].errs[sl.slot];
    }
}

} // namespace snes
