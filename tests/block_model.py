"""The model of palette blocks (include/snesimage_hip.h: "Palette blocks") over the unchanged CPU oracle: the blocked k-means
initialiser, the blocked reassignment and the block call / block sweep, written from the contract.  Block b = by * (32/bw) + bx
covers tiles tx in [bx*bw, (bx+1)*bw), ty in [by*bh, (by+1)*bh).  Everything here runs on the CPU."""
import math

import numpy as np

from tile_model import MIN_GAP, REL_ERR, check_gap, model_candidate  # noqa: F401  (re-exported: one statement of the premises)


def n_blocks(h, bw, bh):
    return (32 // bw) * ((h // 8) // bh)


def block_tiles(b, bw, bh):
    """Tile indices (t = ty * 32 + tx) of block b in raster order: ty outer, tx inner."""
    nbx = 32 // bw
    bx, by = b % nbx, b // nbx
    return [ty * 32 + tx for ty in range(by * bh, (by + 1) * bh) for tx in range(bx * bw, (bx + 1) * bw)]


def mixed_blocks(tp, h, bw, bh):
    """The blocks of the image over which the tile table is not constant."""
    return [b for b in range(n_blocks(h, bw, bh)) if len({int(tp[t]) for t in block_tiles(b, bw, bh)}) > 1]


def is_tied(tp, h, bw, bh):
    return not mixed_blocks(tp, h, bw, bh)


# ---- the initialiser: lib.rs:79-189 with the block in place of the tile --------------------------------------------------

def summed_values(O, img, perceptual):
    """float32 (h, w, 3): what the initialiser sums per opaque pixel — the 8-bit channels, or the pixel's Lab."""
    if not perceptual:
        return img[..., :3].astype(np.float32)
    rgb = img[..., :3].reshape(-1, 3)
    uniq, inv = np.unique(rgb, axis=0, return_inverse=True)
    lab = np.array([O.srgb8_to_lab(c) for c in uniq], np.float32)
    return lab[inv.reshape(-1)].reshape(img.shape[0], img.shape[1], 3)


def block_sums(O, img, bw, bh, perceptual):
    """float32 sums [nby, nbx, 3] and counts [nby, nbx]: per block one ordered chain over its opaque pixels, x outer, y inner."""
    h = img.shape[0]
    pw, ph = bw * 8, bh * 8
    vals, opaque = summed_values(O, img, perceptual), img[..., 3] > 0
    sums = np.zeros((h // ph, 256 // pw, 3), np.float32)
    counts = np.zeros((h // ph, 256 // pw), np.int64)
    for x in range(pw):
        for y in range(ph):
            m = opaque[y::ph, x::pw]
            sums = np.where(m[..., None], sums + vals[y::ph, x::pw], sums).astype(np.float32)  # float32 + float32, rounded once
            counts += m
    return sums, counts


def centre_to_color(O, centre, perceptual, nes):
    """lib.rs:140-171: Lab centre -> sRGB8 / 8, or round(centre / 8) as u8 (saturating, NaN -> 0); --nes: the nearest table colour."""
    if perceptual:
        raw = (O.lab_to_srgb8(centre) // 8).astype(np.uint8)
    else:
        raw = np.array([0 if not (v == v) or v <= 0.0 else min(255, int(math.floor(v / 8.0 + 0.5))) for v in centre], np.uint8)
    return O.new_nes_only(raw, perceptual) if nes else raw


def model_initialize_tiles(O, o, img, bw, bh, perceptual=False, nes=False):
    """The blocked initialiser on oracle `o` (sub_count > 1).  Raises RuntimeError where cogset's 2 <= k < n fails."""
    h, k = img.shape[0], o.sub_count
    sums, counts = block_sums(O, img, bw, bh, perceptual)
    nbx, nby = 32 // bw, (h // 8) // bh
    points, which = [], []
    for bx in range(nbx):  # bx outer, by inner: the order of the k-means points, and so the starting centres
        for by in range(nby):
            s = sums[by, bx]
            if (s[0] + s[1]) + s[2] > np.float32(0.0):
                points.append([float(s[i]) / float(counts[by, bx]) for i in range(3)])
                which.append(by * nbx + bx)
    centres, assign, _ = O.kmeans(np.array(points, np.float64).reshape(-1, 3), k)
    tp = o.tile_palettes
    for b, a in zip(which, assign):
        tp[block_tiles(b, bw, bh)] = a  # a block left out keeps what it had
    pal = np.zeros((k, o.sub_size, 3), np.uint8)
    for i in range(k):
        pal[i, :] = centre_to_color(O, centres[i], perceptual, nes)
    o.tile_palettes = tp
    o.palette = pal.reshape(-1, 3)
    o.optimize()


# ---- the reassignment ----------------------------------------------------------------------------------------------------

def tile_costs(O, o, img, perceptual=False):
    """cost[tile][p] as snesimage_reassign_tiles defines it (binary64, the tile's opaque pixels in raster order), and any[tile]."""
    h, C, S = img.shape[0], o.sub_count, o.sub_size
    pal = o.palette.reshape(C, S, 3)
    dist = O.distance_cielab if perceptual else O.distance_red_mean
    cache = {}

    def pixel(rgb):
        key = (int(rgb[0]), int(rgb[1]), int(rgb[2]))
        if key not in cache:
            target = np.array(key, np.float64)
            out = []
            for p in range(C):
                j = O.closest_color_index(pal[p], target, perceptual)
                out.append(dist(O.snes_as_rgba(pal[p, j])[:3], np.array(key, np.uint8)))
            cache[key] = out
        return cache[key]

    ntile = 32 * (h // 8)
    cost, has = [[0.0] * C for _ in range(ntile)], [False] * ntile
    for t in range(ntile):
        tx, ty = t % 32, t // 32
        for y in range(ty * 8, ty * 8 + 8):
            for x in range(tx * 8, tx * 8 + 8):
                if img[y, x, 3] == 0:
                    continue
                has[t] = True
                d = pixel(img[y, x])
                for p in range(C):
                    cost[t][p] = cost[t][p] + d[p]
    return cost, has


def model_reassign(O, o, img, bw, bh, perceptual=False):
    """The blocked reassignment on oracle `o` -> tiles moved (a multiple of bw * bh)."""
    h, C = img.shape[0], o.sub_count
    cost, has = tile_costs(O, o, img, perceptual)
    tp = o.tile_palettes
    moved = 0
    for b in range(n_blocks(h, bw, bh)):
        tiles = block_tiles(b, bw, bh)
        live = [t for t in tiles if has[t]]  # tiles without an opaque pixel contribute nothing
        if not live:
            continue
        bc = []
        for p in range(C):
            c = 0.0
            for t in live:  # raster order
                c = c + cost[t][p]
            bc.append(c)
        cur = int(tp[tiles[0]])
        best = cur
        for p in range(C):
            if bc[p] < bc[best]:
                best = p
        if best != cur:
            tp[tiles] = best
            moved += len(tiles)
    if moved:
        o.tile_palettes = tp
        o.optimize()
    return moved


# ---- block moves decided by the objective ------------------------------------------------------------------------------------

def model_block_candidate(o, b, sub, bw, bh):
    """error() and palette_map of the oracle's state with every tile of block b drawn from `sub`; the oracle is left as it was."""
    return model_candidate(o, block_tiles(b, bw, bh), sub)


def model_block_call(o, b, sub_count, inc, bw, bh):
    """One block call on the oracle -> (incumbent error after, the block's subpalette after, changed)."""
    tiles = block_tiles(b, bw, bh)
    cur = int(o.tile_palettes[tiles[0]])
    best, best_k, best_map = inc, -1, None
    for k in range(sub_count):
        if k == cur:
            continue
        e, m = model_candidate(o, tiles, k)
        check_gap(e, inc)
        if e < best:
            best, best_k, best_map = e, k, m
    if best_k >= 0:
        tp = o.tile_palettes.copy()
        tp[tiles] = best_k
        o.tile_palettes = tp
        o.palette_map = best_map
    return best, (best_k if best_k >= 0 else cur), int(best_k >= 0)


def model_block_sweep(o, first_block, n, sub_count, bw, bh, inc=None):
    """-> list of (error, sub, changed), one per block."""
    inc = o.error() if inc is None else inc
    log = []
    for b in range(first_block, first_block + n):
        inc, sub, ch = model_block_call(o, b, sub_count, inc, bw, bh)
        log.append((inc, sub, ch))
    return log
