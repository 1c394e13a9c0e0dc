// snesimage_amd/csrc/kernels_level.hpp — per-tile ordered-dither levels chosen by the objective (level_host.inc; DESIGN 5d').
//
// A BANK is L <= 8 ordered-dither tables of one side n; every tile names one of them (level[tile]).  The target image is
// T.c = clamp(orig.c + bank[level[tile(x, y)]][y % n][x % n], 0, 255), the pattern's phase in image coordinates.  A level
// candidate is a (tile, level) pair: the image as it stands with that one tile's 64 pixels re-chosen against the candidate's
// T, palette and tile_palettes untouched.  Its palette_map goes through the map-reading scorer exactly as a tile move's does
// (kernels_tile.hpp: k_move_full, fed the tile's own subpalette, substitutes nothing); no scoring kernel is instantiated anew.
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

// pixel p of tile ct: its position, and its value in T under level lv — clamp(orig + bank[lv][y % n][x % n])
struct LevelPx { int x, y, px; uint32_t o; };
__device__ __forceinline__ LevelPx level_px(const uint8_t *__restrict__ orig, const OrderedBank &bank, int lv, int n, int ct, int p, int W) {
    LevelPx r;
    r.x = (ct & 31) * 8 + (p & 7); r.y = (ct >> 5) * 8 + (p >> 3); r.px = r.y * W + r.x;
    r.o = level_target_px(reinterpret_cast<const uint32_t *>(orig)[r.px], (int)bank.d[256 * lv + (r.y & (n - 1)) * n + (r.x & (n - 1))]);
    return r;
}

struct LevelRemapParams {
    const uint8_t *orig, *base_map, *tile_pal; const uint32_t *pal_rgb8; const float *pal_lab, *lab_eotf;
    const uint16_t *ltiles; const uint8_t *llevels; // the candidates' pairs
    uint16_t *tiles; uint8_t *subs;                 // what k_move_full reads: the tile and its own subpalette
    uint8_t *lmaps;                                 // [cand][W*H]: the candidate's palette_map
    int W, H, sub_size, perceptual, n;
};
// Block = candidate: the base map copied, then the tile's 64 pixels re-chosen against clamp(orig + bank[l][..]) in the tile's own
// subpalette — nearest_entry, on Lab computed in place as k_build_target computes it.  A backdrop context hands in its expanded
// palette, as k_move_remap sees it.
__global__ __launch_bounds__(256) void k_level_remap(LevelRemapParams P, OrderedBank bank) {
    const int cand = blockIdx.x, t = threadIdx.x;
    const int ct = P.ltiles[cand], lv = P.llevels[cand] & 7;
    const int sub = P.tile_pal[ct], base = sub * P.sub_size;
    const int npx = P.W * P.H;
    uint8_t mine = 0; int px = 0;
    if (t < 64) {
        const LevelPx q = level_px(P.orig, bank, lv, P.n, ct, t, P.W);
        px = q.px;
        mine = (uint8_t)nearest_entry(q.o, [&]() { return linear_to_lab(P.lab_eotf[q.o & 0xff], P.lab_eotf[(q.o >> 8) & 0xff], P.lab_eotf[(q.o >> 16) & 0xff]); },
                                      P.perceptual, P.pal_rgb8, P.pal_lab, base, P.sub_size);
    }
    if (t == 0) { P.tiles[cand] = (uint16_t)ct; P.subs[cand] = (uint8_t)sub; }
    copy_map_sync<256>(P.lmaps + (size_t)cand * npx, P.base_map, npx);
    if (t < 64) P.lmaps[(size_t)cand * npx + px] = mine;
}

// Tile ct's 64 pixels of T under level lv, with Lab(T) in both layouts where the planes exist (labpx != nullptr): what a commit
// rewrites so that T on the device is always T(level).  Threads 0..63 of the block.
__device__ __forceinline__ void level_rewrite_tile(const uint8_t *__restrict__ orig, const OrderedBank &bank, int lv, int n, int ct, int W, int H, const float *__restrict__ lab_eotf,
                                                   uint8_t *__restrict__ target, float *__restrict__ labpx, float *__restrict__ labpxT) {
    if (threadIdx.x >= 64) return;
    const LevelPx q = level_px(orig, bank, lv, n, ct, (int)threadIdx.x, W);
    reinterpret_cast<uint32_t *>(target)[q.px] = q.o;
    if (!labpx) return;
    const Lab l = linear_to_lab(lab_eotf[q.o & 0xff], lab_eotf[(q.o >> 8) & 0xff], lab_eotf[(q.o >> 16) & 0xff]);
    const size_t px = (size_t)q.px, pt = (size_t)q.x * H + q.y;
    labpx[3 * px] = l.l; labpx[3 * px + 1] = l.a; labpx[3 * px + 2] = l.b;
    labpxT[3 * pt] = l.l; labpxT[3 * pt + 1] = l.a; labpxT[3 * pt + 2] = l.b;
}

struct LevelCommitParams {
    const double *errs; const TileCall *calls; int ncalls; const uint8_t *llevels, *lmaps; int npx;
    uint8_t *level, *map; double *inc_err; TileLog *log; TileWinRes *res;
    const uint8_t *orig; const float *lab_eotf; int n, W, H;
    uint8_t *target; float *labpx, *labpxT; // labpx == nullptr: no Lab planes (not perceptual)
};
// The window's level calls in order (window_decide, ascending level): the accepting call's map, level and error become the
// image's, and its tile's 64 pixels of T are rewritten (level_rewrite_tile).  One block.
__global__ __launch_bounds__(1024) void k_level_commit(LevelCommitParams P, OrderedBank bank) {
    const TileWin w = window_decide([&]() { return *P.inc_err; }, [&](uint32_t j) { return P.errs[j]; }, P.calls, P.ncalls, P.llevels, P.log, P.res);
    if (w.cand < 0) return;
    copy_map<1024>(P.map, P.lmaps + (size_t)w.cand * P.npx, P.npx);
    const int ct = (int)P.calls[w.call].tile, lv = P.llevels[w.cand] & 7;
    if (threadIdx.x == 0) { P.level[ct] = (uint8_t)lv; *P.inc_err = P.errs[w.cand]; }
    level_rewrite_tile(P.orig, bank, lv, P.n, ct, P.W, P.H, P.lab_eotf, P.target, P.labpx, P.labpxT);
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
// then plain + (as ks_commit, ks_refit_commit and snesimage_shared_error sum: no tree, no reordering); window_decide takes them
// as the joint error (a candidate beyond the kSetLevelCands sums held in LDS never wins).  The accepting call's maps, level and
// errors become EVERY member's, and tile t of every member's T is rewritten (level_rewrite_tile).  One block.
__global__ __launch_bounds__(1024) void ks_level_commit(SetLevelCommitParams P, OrderedBank bank) {
    __shared__ double s_E[kSetLevelCands];
    for (int j = threadIdx.x; j < P.ncand && j < kSetLevelCands; j += 1024) {
        double e = 0.0;
        for (int i = 0; i < P.F; i++) { const double v = P.tab[i].errs[j]; e = i == 0 ? v : e + v; }
        s_E[j] = e;
    }
    __syncthreads();
    const TileWin w = window_decide(
        [&]() { double inc = 0.0; for (int i = 0; i < P.F; i++) { const double v = *P.tab[i].inc_err; inc = i == 0 ? v : inc + v; } return inc; },
        [&](uint32_t j) { return j < (uint32_t)kSetLevelCands ? s_E[j] : (double)INFINITY; }, P.calls, P.ncalls, P.llevels, P.log, P.res);
    if (w.cand < 0) return;
    const int ct = (int)P.calls[w.call].tile, lv = P.llevels[w.cand] & 7;
    for (int m = 0; m < P.F; m++) {
        const SetLevelMember M = P.tab[m];
        copy_map<1024>(M.map, M.lmaps + (size_t)w.cand * P.npx, P.npx);
        if (threadIdx.x == 0) { M.level[ct] = (uint8_t)lv; *M.inc_err = M.errs[w.cand]; }
        level_rewrite_tile(M.orig, bank, lv, P.n, ct, P.W, P.H, M.lab_eotf, M.target, M.labpx, M.labpxT);
    }
}

} // namespace snes
