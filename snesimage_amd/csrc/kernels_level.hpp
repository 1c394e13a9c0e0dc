// snesimage_amd/csrc/kernels_level.hpp — per-tile ordered-dither levels chosen by the objective (level_host.inc; DESIGN 5d').
//
// A BANK is L <= 8 ordered-dither tables of one side n; every tile names one of them (level[tile]).  The target image is
// T.c = clamp(orig.c + bank[level[tile(x, y)]][y % n][x % n], 0, 255), the pattern's phase in image coordinates.  A level
// candidate is a (tile, level) pair: the image as it stands with that one tile's 64 pixels re-chosen against the candidate's
// T, palette and tile_palettes untouched.  Its palette_map goes through the map-reading scorer exactly as a tile move's does
// (kernels_tile.hpp: k_tile_full, fed the tile's own subpalette, substitutes nothing); no scoring kernel is instantiated anew.
#pragma once
#include "kernels.hpp"
#include "kernels_opt.hpp"
#include "kernels_tile.hpp"

namespace snes {

struct OrderedBank { int8_t d[8 * 256]; }; // table l at d[256 * l], n * n offsets row-major, zeros behind them

__device__ __forceinline__ uint32_t level_target_px(uint32_t o, int d) {
    const int r = min(max((int)(o & 0xff) + d, 0), 255), g = min(max((int)((o >> 8) & 0xff) + d, 0), 255), b = min(max((int)((o >> 16) & 0xff) + d, 0), 255);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | (o & 0xff000000u);
}

// k_build_target with a table per tile: four pixels (one uint4) per lane — a quad never straddles a tile — the bank by value,
// staged in LDS.  Same clamp, same Lab outputs through the same functions.
__global__ __launch_bounds__(256) void k_build_target_levels(const uint8_t *__restrict__ orig, OrderedBank bank, int n, const uint8_t *__restrict__ level, const float *__restrict__ lab_eotf,
                                                             int W, int H, uint8_t *__restrict__ target, float *__restrict__ labpx, float *__restrict__ labpxT) {
    __shared__ int8_t s_bank[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += 256) s_bank[i] = bank.d[i];
    __syncthreads();
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= W * H / 4) return;
    const int px0 = 4 * q, x0 = px0 % W, y = px0 / W;
    const int lv = level[(x0 >> 3) + (y >> 3) * (W >> 3)] & 7;
    const uint4 o4 = reinterpret_cast<const uint4 *>(orig)[q];
    const uint32_t in[4] = {o4.x, o4.y, o4.z, o4.w};
    uint32_t out[4];
    for (int i = 0; i < 4; i++) out[i] = level_target_px(in[i], (int)s_bank[256 * lv + (y & (n - 1)) * n + ((x0 + i) & (n - 1))]);
    reinterpret_cast<uint4 *>(target)[q] = make_uint4(out[0], out[1], out[2], out[3]);
    if (!labpx) return;
    for (int i = 0; i < 4; i++) {
        const uint32_t o = out[i];
        Lab l = linear_to_lab(lab_eotf[o & 0xff], lab_eotf[(o >> 8) & 0xff], lab_eotf[(o >> 16) & 0xff]);
        const size_t px = (size_t)px0 + i, pt = (size_t)(x0 + i) * H + y;
        labpx[3 * px] = l.l; labpx[3 * px + 1] = l.a; labpx[3 * px + 2] = l.b;
        labpxT[3 * pt] = l.l; labpxT[3 * pt + 1] = l.a; labpxT[3 * pt + 2] = l.b;
    }
}

struct LevelRemapParams {
    const uint8_t *orig, *base_map, *tile_pal; const uint32_t *pal_rgb8; const float *pal_lab, *lab_eotf;
    const uint16_t *ltiles; const uint8_t *llevels; // the candidates' pairs
    uint16_t *tiles; uint8_t *subs;                 // what k_tile_full reads: the tile and its own subpalette
    uint8_t *lmaps;                                 // [cand][W*H]: the candidate's palette_map
    int W, H, sub_size, perceptual, n;
};
// Block = candidate: the base map copied, then the tile's 64 pixels re-chosen against clamp(orig + bank[l][..]) in the tile's own
// subpalette — the search of prep_body (exact integer redmean key, or CIEDE2000 on Lab computed in place as k_build_target
// computes it; strict <: lowest index).  A backdrop context hands in its expanded palette, as k_tile_remap sees it.
__global__ __launch_bounds__(256) void k_level_remap(LevelRemapParams P, OrderedBank bank) {
    const int cand = blockIdx.x, t = threadIdx.x;
    const int ct = P.ltiles[cand], lv = P.llevels[cand] & 7;
    const int sub = P.tile_pal[ct], base = sub * P.sub_size;
    const int npx = P.W * P.H;
    uint8_t mine = 0; int px = 0;
    if (t < 64) {
        const int x = (ct & 31) * 8 + (t & 7), y = (ct >> 5) * 8 + (t >> 3);
        px = y * P.W + x;
        const uint32_t o = level_target_px(reinterpret_cast<const uint32_t *>(P.orig)[px], (int)bank.d[256 * lv + (y & (P.n - 1)) * P.n + (x & (P.n - 1))]);
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
                const Lab tl = linear_to_lab(P.lab_eotf[o & 0xff], P.lab_eotf[(o >> 8) & 0xff], P.lab_eotf[(o >> 16) & 0xff]);
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
    if (t == 0) { P.tiles[cand] = (uint16_t)ct; P.subs[cand] = (uint8_t)sub; }
    const uint4 *src = reinterpret_cast<const uint4 *>(P.base_map);
    uint4 *dst = reinterpret_cast<uint4 *>(P.lmaps + (size_t)cand * npx);
    for (int i = t; i < npx / 16; i += 256) dst[i] = src[i];
    __syncthreads(); // the copy of the tile's rows is in place before its 64 bytes are replaced
    if (t < 64) P.lmaps[(size_t)cand * npx + px] = mine;
}

struct LevelCommitParams {
    const double *errs; const TileCall *calls; int ncalls; const uint8_t *llevels, *lmaps; int npx;
    uint8_t *level, *map; double *inc_err; TileLog *log; TileWinRes *res;
    const uint8_t *orig; const float *lab_eotf; int n, W, H;
    uint8_t *target; float *labpx, *labpxT; // labpx == nullptr: no Lab planes (not perceptual)
};
// The window's level calls in order (lib.rs:216-219 per call: best := incumbent, ascending level, strict <): every call up to
// and including the first that accepts is logged; that one's map, level and error become the image's, and its tile's 64 pixels
// of T (with Lab(T) in both layouts) are rewritten, so that T on the device is always T(level).  One block.
__global__ __launch_bounds__(1024) void k_level_commit(LevelCommitParams P, OrderedBank bank) {
    __shared__ int s_win, s_call;
    if (threadIdx.x == 0) {
        const double inc = *P.inc_err;
        int win = -1, used = P.ncalls, acc = -1;
        for (int i = 0; i < P.ncalls && win < 0; i++) {
            const TileCall c = P.calls[i];
            double best = inc; int bj = -1;
            for (uint32_t j = c.first; j < c.first + c.count; j++) { const double e = P.errs[j]; if (e < best) { best = e; bj = (int)j; } }
            TileLog r; r.error = best; r.sub = bj >= 0 ? (int32_t)P.llevels[bj] : (int32_t)c.cur; r.changed = bj >= 0 ? 1 : 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
            P.log[i] = r;
            if (bj >= 0) { win = bj; acc = i; used = i + 1; }
        }
        P.res->consumed = used; P.res->accepted = acc;
        s_win = win; s_call = acc;
    }
    __syncthreads(); // the records are written before the state changes hands
    const int win = s_win;
    if (win < 0) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(P.lmaps + (size_t)win * P.npx);
    uint4 *dst = reinterpret_cast<uint4 *>(P.map);
    for (int i = threadIdx.x; i < P.npx / 16; i += 1024) dst[i] = src[i];
    const int ct = (int)P.calls[s_call].tile, lv = P.llevels[win] & 7;
    if (threadIdx.x == 0) { P.level[ct] = (uint8_t)lv; *P.inc_err = P.errs[win]; }
    if (threadIdx.x < 64) {
        const int t = threadIdx.x, x = (ct & 31) * 8 + (t & 7), y = (ct >> 5) * 8 + (t >> 3), px = y * P.W + x;
        const uint32_t o = level_target_px(reinterpret_cast<const uint32_t *>(P.orig)[px], (int)bank.d[256 * lv + (y & (P.n - 1)) * P.n + (x & (P.n - 1))]);
        reinterpret_cast<uint32_t *>(P.target)[px] = o;
        if (P.labpx) {
            Lab l = linear_to_lab(P.lab_eotf[o & 0xff], P.lab_eotf[(o >> 8) & 0xff], P.lab_eotf[(o >> 16) & 0xff]);
            const size_t pt = (size_t)x * P.H + y;
            P.labpx[3 * (size_t)px] = l.l; P.labpx[3 * (size_t)px + 1] = l.a; P.labpx[3 * (size_t)px + 2] = l.b;
            P.labpxT[3 * pt] = l.l; P.labpxT[3 * pt + 1] = l.a; P.labpxT[3 * pt + 2] = l.b;
        }
    }
}

// ---- tied levels of a shared-palette set (shared_level_host.inc; DESIGN 5d'') ----------------------------------------------
// One candidate list for all members: candidate j is "every member's tile ltiles[j] on level llevels[j]", scored by each member
// as candidate j of its own tile workspace (k_level_remap as it is).
constexpr int kSetLevelCands = 512; // most candidates of a window: kTileGroup of tile_host.inc
struct SetLevelMember {
    const uint8_t *orig; const float *lab_eotf; const double *errs; const uint8_t *lmaps; // errs, lmaps: the member's tile workspace
    uint8_t *level, *map, *target; float *labpx, *labpxT; double *inc_err;                // labpx == nullptr: no Lab planes
};
struct SetLevelCommitParams {
    const SetLevelMember *tab; int F; const TileCall *calls; int ncalls, ncand; const uint8_t *llevels; int npx, n, W, H;
    TileLog *log; TileWinRes *res;
};
// The window's tied level calls in order.  E and every candidate's E_l are the members' errors summed in member order — first,
// then plain + (as ks_commit, ks_refit_commit and snesimage_shared_error sum: no tree, no reordering); per call best := E,
// ascending level, strict < (lib.rs:216-219 on the joint error; a NaN never wins).  Every call up to and including the first that
// accepts is logged; that one's maps, level and errors become EVERY member's, and tile t of every member's T (with Lab(T) in
// both layouts, through the functions k_level_commit uses) is rewritten.  One block.
__global__ __launch_bounds__(1024) void ks_level_commit(SetLevelCommitParams P, OrderedBank bank) {
    __shared__ double s_E[kSetLevelCands];
    __shared__ int s_win, s_call;
    for (int j = threadIdx.x; j < P.ncand && j < kSetLevelCands; j += 1024) {
        double e = 0.0;
        for (int i = 0; i < P.F; i++) { const double v = P.tab[i].errs[j]; e = i == 0 ? v : e + v; }
        s_E[j] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double inc = 0.0;
        for (int i = 0; i < P.F; i++) { const double v = *P.tab[i].inc_err; inc = i == 0 ? v : inc + v; }
        int win = -1, used = P.ncalls, acc = -1;
        for (int i = 0; i < P.ncalls && win < 0; i++) {
            const TileCall c = P.calls[i];
            double best = inc; int bj = -1;
            for (uint32_t j = c.first; j < c.first + c.count && j < (uint32_t)kSetLevelCands; j++) { const double e = s_E[j]; if (e < best) { best = e; bj = (int)j; } }
            TileLog r; r.error = best; r.sub = bj >= 0 ? (int32_t)P.llevels[bj] : (int32_t)c.cur; r.changed = bj >= 0 ? 1 : 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
            P.log[i] = r;
            if (bj >= 0) { win = bj; acc = i; used = i + 1; }
        }
        P.res->consumed = used; P.res->accepted = acc;
        s_win = win; s_call = acc;
    }
    __syncthreads(); // the records are written before the state changes hands
    const int win = s_win;
    if (win < 0) return;
    const int ct = (int)P.calls[s_call].tile, lv = P.llevels[win] & 7;
    for (int m = 0; m < P.F; m++) {
        const SetLevelMember M = P.tab[m];
        const uint4 *src = reinterpret_cast<const uint4 *>(M.lmaps + (size_t)win * P.npx);
        uint4 *dst = reinterpret_cast<uint4 *>(M.map);
        for (int i = threadIdx.x; i < P.npx / 16; i += 1024) dst[i] = src[i];
        if (threadIdx.x == 0) { M.level[ct] = (uint8_t)lv; *M.inc_err = M.errs[win]; }
        if (threadIdx.x < 64) {
            const int t = threadIdx.x, x = (ct & 31) * 8 + (t & 7), y = (ct >> 5) * 8 + (t >> 3), px = y * P.W + x;
            const uint32_t o = level_target_px(reinterpret_cast<const uint32_t *>(M.orig)[px], (int)bank.d[256 * lv + (y & (P.n - 1)) * P.n + (x & (P.n - 1))]);
            reinterpret_cast<uint32_t *>(M.target)[px] = o;
            if (M.labpx) {
                Lab l = linear_to_lab(M.lab_eotf[o & 0xff], M.lab_eotf[(o >> 8) & 0xff], M.lab_eotf[(o >> 16) & 0xff]);
                const size_t pt = (size_t)x * P.H + y;
                M.labpx[3 * (size_t)px] = l.l; M.labpx[3 * (size_t)px + 1] = l.a; M.labpx[3 * (size_t)px + 2] = l.b;
                M.labpxT[3 * pt] = l.l; M.labpxT[3 * pt + 1] = l.a; M.labpxT[3 * pt + 2] = l.b;
            }
        }
    }
}

} // namespace snes
