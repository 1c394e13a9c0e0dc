"""The model of the character budget (include/snesimage_hip.h: "character", "merge candidate", "reduction step") in numpy
over the unchanged CPU oracle: the oracle provides the palette_map setter, error() and red_mean_key; everything else is
counting.  A backdrop context is modelled as backdrop_model.Model does it: the oracle's expanded context (C, S + 1), whose
map value S is the backdrop (zero_at = S)."""
import json

import numpy as np

REL_ERR = 1e-11
MIN_GAP = 1e-9  # premise of every decision compared: two errors are equal exactly or differ by more than this (relative)


# ---- characters and classes --------------------------------------------------------------------------------------------

def tiles_of(plane):
    """(h, 256) -> (ntile, 64): tile t = ty * 32 + tx, row-major inside the tile."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def untile(tiles, h):
    return tiles.reshape(h // 8, 32, 8, 8).transpose(0, 2, 1, 3).reshape(h, 256)


def flip_char(c, f):
    """flip_f(c)[y][x] = c[y ^ (f & 2 ? 7 : 0)][x ^ (f & 1 ? 7 : 0)] on (..., 64)."""
    c = np.asarray(c)
    g = c.reshape(c.shape[:-1] + (8, 8))
    if f & 2:
        g = g[..., ::-1, :]
    if f & 1:
        g = g[..., :, ::-1]
    return g.reshape(c.shape)


def characters(pmap, img, zero_at=None):
    """What as_json writes into `tiles`: 0 where the source alpha is 0 or the map value is the backdrop, else map + 1."""
    m = tiles_of(np.asarray(pmap, np.uint8)).astype(np.int64)
    a = tiles_of(np.ascontiguousarray(img[..., 3]))
    c = m + 1
    if zero_at is not None:
        c[m == zero_at] = 0
    c[a == 0] = 0
    return c.astype(np.uint8)


def pinned_tiles(img):
    return (tiles_of(np.ascontiguousarray(img[..., 3])) == 0).any(axis=1)


def classes(chars):
    """-> (rep, flip_of, U, size): rep(t) the lowest tile of t's class, flip_of(t) the lowest f with c_t == flip_f(c_rep(t)),
    size[t] the tiles in t's class."""
    n = len(chars)
    rep, flip = np.zeros(n, np.int64), np.zeros(n, np.int64)
    seen = {}
    for t in range(n):
        r = seen.get(chars[t].tobytes())
        if r is None:
            r = t
            for f in range(4):
                seen.setdefault(flip_char(chars[t], f).tobytes(), t)
        rep[t] = r
        flip[t] = next(f for f in range(4) if np.array_equal(chars[t], flip_char(chars[r], f)))
    size = np.bincount(rep, minlength=n)[rep]
    return rep, flip, int((rep == np.arange(n)).sum()), size


def pack_key(cost, t, b, f):
    return (int(cost) << 22) | (int(t) << 12) | (int(b) << 2) | int(f)


# ---- the proxy -----------------------------------------------------------------------------------------------------------

def red_mean_keys(px, ent):
    """The integer key of lib.rs:1080-1088 (512 * distance^2) between (..., 3) arrays of 8-bit colours; checked against the
    oracle's red_mean_key by the tests."""
    a, b = np.asarray(px, np.int64), np.asarray(ent, np.int64)
    rs = a[..., 0] + b[..., 0]
    d = a - b
    return (1024 + rs) * d[..., 0] ** 2 + 2048 * d[..., 1] ** 2 + (1534 - rs) * d[..., 2] ** 2


def palette_rgb8(O, o):
    return np.array([O.snes_as_rgba(c)[:3] for c in o.palette], np.int64)


class Budget:
    """The character budget on an oracle image `o` (a plain context, or the expanded context of a backdrop one with
    zero_at = S).  The oracle's palette and tile palettes are never changed; its map is the state."""

    def __init__(self, O, o, img, zero_at=None):
        self.O, self.o, self.img, self.zero_at = O, o, img, zero_at
        self.h = img.shape[0]
        self.ntile = 32 * (self.h // 8)
        self.S = o.sub_size
        self.pinned = pinned_tiles(img)
        self.orig = tiles_of_rgb(img)
        self.pal8 = palette_rgb8(O, o).reshape(o.sub_count, self.S, 3)
        self.tp = o.tile_palettes[:self.ntile].astype(np.int64)
        self._tab = {}

    def table(self, t):
        """key[pixel][map value] of tile t: its original pixels against its own subpalette."""
        if t not in self._tab:
            self._tab[t] = red_mean_keys(self.orig[t][:, None, :], self.pal8[self.tp[t]][None, :, :])
        return self._tab[t]

    def state(self):
        pm = self.o.palette_map
        chars = characters(pm, self.img, self.zero_at)
        return (pm, chars) + classes(chars)

    def candidates(self):
        """Every (cost, t, b, f) of the definition, sorted."""
        pm, chars, rep, flip, U, size = self.state()
        vals = tiles_of(pm).astype(np.int64)
        idx = np.arange(self.ntile)
        donors = idx[(rep == idx) & ~self.pinned]
        out = []
        px = np.arange(64)
        for t in idx[~self.pinned & (size == 1)]:
            tab, ds = self.table(t), donors[donors != t]
            for f in range(4):
                cost = tab[px[None, :], flip_char(vals[ds], f)].sum(axis=1)
                out.extend((int(c), int(t), int(b), f) for c, b in zip(cost, ds))
        out.sort()
        return out

    def shortlist(self, K):
        return self.candidates()[:K]

    def merged_map(self, t, b, f, pm=None):
        vals = tiles_of(self.o.palette_map if pm is None else pm).copy()
        vals[t] = flip_char(vals[b], f)
        return untile(vals, self.h)

    def score(self, t, b, f):
        """error() and map of the candidate; the oracle is left as it was."""
        pm = self.o.palette_map
        m = self.merged_map(t, b, f, pm)
        self.o.palette_map = m
        e = self.o.error()
        self.o.palette_map = pm
        return e, m

    def step(self, K, guard=True):
        """One reduction step -> record dict, or None without an eligible pair."""
        short = self.shortlist(K)
        if not short:
            return None
        inc = self.o.error()
        scored = [self.score(t, b, f) for _, t, b, f in short]
        best = None
        for rank, (e, _) in enumerate(scored):
            if e != e:
                continue
            if best is not None and guard:
                check_gap(e, scored[best][0])
            if best is None or e < scored[best][0]:
                best = rank
        cost, t, b, f = short[best]
        self.o.palette_map = scored[best][1]
        U = classes(characters(scored[best][1], self.img, self.zero_at))[2]
        return dict(error=scored[best][0], cost=cost, tile=t, donor=b, flip=f, rank=best, unique=U, before=inc)

    def reduce(self, max_unique, K, guard=True):
        recs = []
        U = self.state()[4]
        while U > max_unique:
            r = self.step(K, guard)
            if r is None:
                break
            assert r["unique"] == U - 1, "a merge takes exactly one class away"
            U = r["unique"]
            recs.append(r)
        return recs, U


def tiles_of_rgb(img):
    return np.stack([tiles_of(np.ascontiguousarray(img[..., c])) for c in range(3)], axis=-1).astype(np.int64)


def check_gap(e, ref):
    gap = abs(e - ref) / ref
    assert gap == 0.0 or gap > MIN_GAP, "the input breaks the premise: error %r against %r (gap %.3e)" % (e, ref, gap)


def assert_trajectory_decides(recs):
    """The condition on the inputs of a trajectory test: the objective overrules the proxy at least once, and a budget costs."""
    assert any(r["rank"] > 0 for r in recs), "the proxy's first choice always wins: nothing shows that the shortlist was scored"
    assert any(r["error"] > r["before"] for r in recs), "no step raises the error"


# ---- JSON ----------------------------------------------------------------------------------------------------------------

def tilemap_json(chars, tile_palettes):
    rep, flip, U, _ = classes(chars)
    reps = [t for t in range(len(chars)) if rep[t] == t]
    pos = {t: i for i, t in enumerate(reps)}
    d = {"characters": [[int(v) for v in chars[t]] for t in reps], "character": [pos[int(r)] for r in rep],
         "hflip": [int(f) & 1 for f in flip], "vflip": [int(f) >> 1 for f in flip], "palette": [int(v) for v in tile_palettes[:len(chars)]]}
    return json.dumps(d, separators=(",", ":"), sort_keys=True)


def unflip_tilemap(tm):
    """The `tiles` array a tilemap JSON stands for."""
    ch = np.array(tm["characters"], np.uint8)
    return [flip_char(ch[c], h + 2 * v).tolist() for c, h, v in zip(tm["character"], tm["hflip"], tm["vflip"])]


def count_unique(tiles):
    return classes(np.array(tiles, np.uint8).reshape(-1, 64))[2]
