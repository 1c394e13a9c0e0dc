"""The inputs of tests/test_many_tiles.py: pictures of 288, 544 and 1,024 tiles (and sets of 672 and 1,152 global tiles), the
smallest that take the tile-indexed kernels of the character budget, the refit and the native export past their strides of
256, their waves of 64 tiles and their blocks of 1,024 ("Tile counts").  The case table, the pictures, the
planted maps and what the models say about them; tests/test_many_tiles_model.py shows on the CPU that every input reaches the
path it is there for.  Everything here runs on the CPU, is computed once per process and left unchanged."""
import numpy as np

import backdrop_model as B
import character_model as M
import refit_model as R
import set_character_model as SM
import set_refit_model as SR

MIN_GAP = M.MIN_GAP

# id -> (h, sub_count, sub_size, backdrop).  The width is 256: h / 8 * 32 tiles.
CASES = {
    "T288": (72, 2, 3, False),     # shortlist and trajectory above 256 tiles: a second donor per thread of k_merge_proxy
    "T544": (136, 4, 7, False),    # above 512 tiles: a third donor, the cross-wave prefix of k_export_pos
    "T544b": (136, 4, 7, True),    # ... with a backdrop (map value 7 reads 0)
    "T1024": (256, 2, 3, False),   # the cap, on a planted map: every thread of the one-block kernels owns a tile
    "R544": (136, 2, 3, False),    # planted classes whose members lie on both sides of 256 and of 512
    "R1024": (256, 1, 7, False),   # one class of 1,024 members
    "R1024p": (256, 1, 7, True),   # ... one of them pinned: not eligible
    "E544": (136, 2, 3, False),    # the export from the k-means start, 2bpp
    "E544w": (136, 8, 15, False),  # ... 4bpp
    "E1024": (256, 2, 3, False),   # ... at the cap
}
SEED = 0

# A near copy planted into the picture: tile dst takes tile src's pixels with the two pixels (y, x) and (y, x + 1) swapped.
# src is a recipient the proxy ranks first in the unplanted picture, dst lies in the last row of tiles; the swapped pixels read
# different map values, so the two are different characters and each other's cheapest donors (chosen on the CPU).
NEAR_COPY = {"T288": (214, 270, 2, 2), "T544": (339, 530, 0, 5), "T544b": (339, 530, 0, 0)}


def ntile(case):
    return 32 * (CASES[case][0] // 8)


def tile_px(img, t):
    return img[(t // 32) * 8:(t // 32) * 8 + 8, (t % 32) * 8:(t % 32) * 8 + 8]


def image(case):
    h = CASES[case][0]
    img = B.image(h, SEED).copy()
    if case in NEAR_COPY:
        src, dst, y, x = NEAR_COPY[case]
        p = tile_px(img, dst)
        p[:] = tile_px(img, src)
        a = p[y, x].copy()
        p[y, x] = p[y, x + 1]
        p[y, x + 1] = a
    if case == "R1024p":
        img[h - 8, 248, 3] = 0  # pixel 0 of tile 1,023 is transparent: the tile is pinned
    return img


_kmeans = {}


def kmeans_state(O, case):
    """The k-means start of the case's picture -> dict(img, tp, pal, pmap), the expanded context's for a backdrop."""
    if case not in _kmeans:
        h, C, S, backdrop = CASES[case]
        img = image(case)
        if backdrop:
            o = B.Model(O, img, C, S, {}).o
        else:
            o = O.OracleImage(img, C, S)
            o.initialize_tiles()
            o.recalculate_palettes()
        _kmeans[case] = dict(img=img, tp=o.tile_palettes, pal=o.palette, pmap=o.palette_map)
        o.close()
    return _kmeans[case]


# ---- planted maps ------------------------------------------------------------------------------------------------------------
SINGLETONS = (0, 255, 256, 511, 512, 767, 768, 1020, 1021, 1022, 1023)  # T1024: both sides of every stride of 256, and the last wave's end
COMMON = 1                                                               # every other tile of T1024 and R1024 takes this tile's values
N_CLASSES = 6                                                            # R544


def planted_classes(O):
    """R544: six classes of 3 to 5 tiles that the k-means start leaves alone in their classes: the representative below 256,
    members in 256..511 and in 512..543, under flips (i + k) % 4."""
    km = kmeans_state(O, "R544")
    rep, flip, U, size = M.classes(M.characters(km["pmap"], km["img"]))
    singles = np.flatnonzero(size == 1)
    lo, mid, hi = singles[singles < 256], singles[(singles >= 256) & (singles < 512)], singles[singles >= 512]
    out = []
    for i in range(N_CLASSES):
        mem = [int(lo[10 + 25 * i]), int(mid[5 + 35 * i]), int(hi[2 * i + 1])]
        if i % 2:
            mem.insert(1, int(lo[140 + i]))
        if i % 3 == 0:
            mem.insert(len(mem) - 1, int(mid[20 + 35 * i]))
        out.append(mem)
    return out


def planted_map(O, case):
    """The map the case starts from, or None for the k-means start's own."""
    km = kmeans_state(O, case)
    h = CASES[case][0]
    vals = M.tiles_of(km["pmap"]).copy()
    if case == "T1024":  # every singleton takes the k-means values of the singleton before it (the first: the last one's), which
        # suit that tile's pixels and no other's: each is the cheapest recipient of one donor and the cheapest donor of one recipient
        new = np.repeat(vals[COMMON][None], 1024, 0)
        for j, s in enumerate(SINGLETONS):
            new[s] = vals[SINGLETONS[j - 1]]
        return M.untile(new, h)
    if case == "R544":
        for i, mem in enumerate(planted_classes(O)):
            for k, m in enumerate(mem[1:], 1):
                vals[m] = M.flip_char(vals[mem[0]], (i + k) % 4)
        return M.untile(vals, h)
    if case == "R1024":
        return M.untile(np.repeat(vals[COMMON][None], 1024, 0), h)
    if case == "R1024p":  # with the backdrop value (7 reads 0) at pixel 0, where tile 1,023 is transparent: all 1,024 read one character
        v = vals[COMMON].copy()
        v[0] = CASES[case][2]
        return M.untile(np.repeat(v[None], 1024, 0), h)
    return None


def oracle_at(O, case):
    """A fresh oracle in the case's starting state, and its Budget."""
    h, C, S, backdrop = CASES[case]
    km = kmeans_state(O, case)
    o = O.OracleImage(km["img"], C, S + 1 if backdrop else S)
    o.tile_palettes, o.palette, o.palette_map = km["tp"], km["pal"], km["pmap"]
    pm = planted_map(O, case)
    if pm is not None:
        o.palette_map = pm
    return o, M.Budget(O, o, km["img"], S if backdrop else None)


# ---- what the models say -------------------------------------------------------------------------------------------------------
_cache = {}


def _cached(fn):
    def wrapper(O, *key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(O, *key)
        return _cache[k]
    wrapper.__name__ = fn.__name__
    return wrapper


@_cached
def classes(O, case):
    """-> dict(chars, rep, flip, U, size, pinned) of the starting state."""
    o, bud = oracle_at(O, case)
    pm, chars, rep, flip, U, size = bud.state()
    o.close()
    return dict(chars=chars, rep=rep, flip=flip, U=U, size=size, pinned=bud.pinned)


@_cached
def shortlist(O, case):
    """-> dict(top: the model's candidates()[:64], ncand)."""
    o, bud = oracle_at(O, case)
    cand = bud.candidates()
    o.close()
    return dict(top=cand[:64], ncand=len(cand))


@_cached
def trajectory(O, case, merges, K):
    """`merges` guarded reduction steps with a shortlist of K -> dict(recs, U0, U, pmap, err)."""
    o, bud = oracle_at(O, case)
    U0 = bud.state()[4]
    recs, U = bud.reduce(U0 - merges, K)
    r = dict(recs=recs, U0=U0, U=U, pmap=o.palette_map, err=o.error(), rgba=o.as_rgba())
    o.close()
    return r


SCORED_PAIRS = {"T544": ((530, 7, 1), (540, 20, 2), (7, 530, 3), (20, 540, 0)), "T544b": ((530, 7, 1), (7, 530, 3))}  # (t, b, f): t >= 512 > 32 > b, and the reverse


@_cached
def scored_pairs(O, case):
    o, bud = oracle_at(O, case)
    assert not bud.pinned.any()
    r = dict(inc=o.error(), scored=[bud.score(*c) for c in SCORED_PAIRS[case]])
    o.close()
    return r


@_cached
def refit(O, case):
    """The refit on the starting state -> dict(snap, scored: (error, map) per class, inc, sweep: (records, accepted, U), pmap, err
    behind one sweep)."""
    o, bud = oracle_at(O, case)
    rf = R.Refit(bud)
    snap = rf.snapshot()
    r = dict(snap=snap, inc=o.error(), scored=[rf.score(c) for c in snap])
    r["sweep"] = rf.sweep()
    r.update(pmap=o.palette_map, err=o.error(), rgba=o.as_rgba())
    o.close()
    return r


# ---- sets --------------------------------------------------------------------------------------------------------------------
SET_GEOMETRY = (1, 7)
PAST_1024_SEED = 9  # the explicit palette of tests/test_set_characters.py::make_set under which two of the five pool tiles of
                    # frames_past_1024() read the same characters: a class of more than 256 tiles


def symmetric(px):
    """A tile's pixels made their own image under every flip: the top-left quadrant mirrored."""
    q = np.minimum(np.arange(8), 7 - np.arange(8))
    return px[q[:, None], q[None, :]]


REFILL_SINGULAR = (10, 20, 266, 276, 522, 532)  # global tiles: {10, 266, 522} and {20, 276, 532} are congruent mod 256


def refill_frames():
    """Three frames of 56 rows (G = 672), planted as frames_past_1024(): most tiles pixel copies of five.  The six singular tiles
    are one symmetric tile with one pixel inverted, each in another orbit of the flips: different characters, and a donor costs
    a recipient the same under all four flips.  So a recipient's cheapest keys are the 8 and the 12 of the two residues mod 256,
    each residue one thread of ks_merge_proxy, which keeps four."""
    h, F, nt = 56, 3, 224
    base = B.image(h, 20)
    pool = [tile_px(base, t).copy() for t in (0, 37, 150, 200, 223)]
    odd = symmetric(tile_px(base, 100)).copy()
    imgs = []
    for i in range(F):
        img = np.zeros_like(base)
        for t in range(nt):
            tile_px(img, t)[:] = pool[(t + i) % 5]
        imgs.append(img)
    for u, g in enumerate(REFILL_SINGULAR):
        p = tile_px(imgs[g // nt], g % nt)
        p[:] = odd
        y, x = u // 4, u % 4  # one orbit each
        p[y, x, :3] = 255 - odd[y, x, :3]
    return imgs, nt


_set_inputs = {}


def set_inputs(O, name):
    """-> (imgs, ntile, tile_palettes per member, palette): "refill" in the oracle's k-means start of the member stack,
    "past1024" (whose stack is higher than the oracle takes) on the explicit palette."""
    if name not in _set_inputs:
        if name == "refill":
            imgs, nt = refill_frames()
            tps, pal = SM.stack_start(O, imgs, *SET_GEOMETRY)
        else:
            import test_set_characters as TS
            imgs, nt = TS.frames_past_1024()
            tps, pal = [np.zeros(1024, np.uint8) for _ in imgs], TS.explicit_palette(*SET_GEOMETRY, PAST_1024_SEED)
        _set_inputs[name] = (imgs, nt, tps, pal)
    return _set_inputs[name]


def set_oracles(O, name):
    imgs, nt, tps, pal = set_inputs(O, name)
    oms = SM.oracle_members(O, imgs, tps, pal, *SET_GEOMETRY)
    return oms, SM.SetBudget(O, oms, imgs)


def close_all(oms):
    for o in oms:
        o.close()


@_cached
def set_shortlist(O, name):
    oms, sb = set_oracles(O, name)
    cand = sb.candidates()
    chars, rep, flip, U, size = sb.state()
    close_all(oms)
    return dict(top=cand[:64], ncand=len(cand), U=U, rep=rep, flip=flip, chars=chars, size=size)


SET_PAIRS = ((1038, 3, 1), (3, 1038, 2))  # (gt, gb, f) of past1024: member 2's tile 270 (a singular one) with member 0's tile 3, both ways


@_cached
def set_step(O, name, K):
    """The scored pairs, one reduction step, and the refit behind it -> dict(incs, scored, rec, pmaps, snap, refits, sweep,
    pmaps_refit)."""
    oms, sb = set_oracles(O, name)
    r = dict(incs=[o.error() for o in oms], scored=[sb.score(*c) for c in SET_PAIRS])
    r["rec"] = sb.step(K)
    r["pmaps"] = [o.palette_map for o in oms]
    rf = SR.SetRefit(sb)
    r["snap"] = rf.snapshot()
    r["incs_reduced"] = [o.error() for o in oms]
    r["refits"] = [rf.score(c) for c in r["snap"]]
    state = sb.state()
    r.update(chars=state[0], rep=state[1], flip=state[2], U=state[3])
    r["sweep"] = rf.sweep()
    r["pmaps_refit"] = [o.palette_map for o in oms]
    close_all(oms)
    return r
