"""The model of an ordered-dither context (include/snesimage_hip.h: snesimage_set_ordered_dither) over the unchanged CPU oracle.

Two oracles of the same geometry, flags, tile_palettes and palette: `oT` built from the target image T = clamp(orig +
d[y % n][x % n]) makes every nearest-colour choice (optimize, reassign_tiles), `oO` built from the original measures every
error on the map oT chose.  The initialisers run on a plain oracle over the original.  Everything here runs on the CPU."""
import numpy as np

REL_ERR = 1e-11
MIN_GAP = 1e-9  # premise of every decision compared: two errors are equal exactly or differ by more than this (relative)


def image(h, seed=0, variant=0):
    from snesimage_amd.synth import synth_image
    return synth_image(0x5EED0D00 + 16 * h + seed, 256, h, variant)


def with_hole(img):
    """`img` with alpha cleared in rows [4, 20) x columns [100, 150): whole tiles and parts of tiles.  synth_image's variant 1
    clears rows from 96 on, which no picture of these heights has."""
    out = img.copy()
    out[4:20, 100:150, 3] = 0
    assert (out[..., 3] == 0).any() and (out[..., 3] == 255).any()
    return out


def bayer(n, amplitude):
    """snesimage_bayer_offsets in Python integers (include/snesimage_hip.h): M_1 = [0], M_2n = [[4M, 4M+2], [4M+3, 4M+1]];
    d = sign(num) * ((2|num| + den) // (2 den)), num = A (2M + 1 - n^2), den = 2 n^2."""
    m = np.zeros((1, 1), np.int64)
    while m.shape[0] < n:
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    num = amplitude * (2 * m + 1 - n * n)
    den = 2 * n * n
    return (np.sign(num) * ((2 * np.abs(num) + den) // (2 * den))).astype(np.int8)


def target_image(img, table):
    """T: the offsets tiled over the picture and added to r, g, b with a clamp; alpha kept.  table None: the original."""
    if table is None:
        return img.copy()
    t = np.asarray(table, np.int64)
    n = t.shape[0]
    h, w = img.shape[:2]
    d = np.tile(t, (h // n + 1, w // n + 1))[:h, :w]
    out = img.copy()
    out[..., :3] = np.clip(img[..., :3].astype(np.int64) + d[..., None], 0, 255).astype(np.uint8)
    return out


def check_gap(e, ref):
    gap = abs(e - ref) / ref
    assert gap == 0.0 or gap > MIN_GAP, "the input breaks the premise: error %r against %r (gap %.3e)" % (e, ref, gap)


class Model:
    """count x size is the geometry the oracles run at: for a backdrop context the expanded one (size + 1, column `size` = B)."""

    def __init__(self, O, img, count, size, flags, table):
        self.O, self.C, self.S, self.flags, self.img = O, count, size, dict(flags), img
        self.T = target_image(img, table)
        self.oT = O.OracleImage(self.T, count, size, **flags)
        self.oO = O.OracleImage(img, count, size, **flags)
        self.min_gap = float("inf")  # smallest non-zero gap any compared pair showed

    def close(self):
        self.oT.close()
        self.oO.close()

    # -- state ---------------------------------------------------------------------------------------------------------
    def set_state(self, tile_palettes, palette):
        self.oT.tile_palettes = tile_palettes
        self.oT.palette = palette
        self.optimize()

    def kmeans_start(self, count=None, size=None):
        """The reference's initialisers on the original (a plain oracle), then optimize() against T.  Returns (tile_palettes,
        palette) of the plain oracle and its map.  count, size: the initialisers' geometry where it is not the model's
        (a backdrop context: the regular entries)."""
        o0 = self.O.OracleImage(self.img, count or self.C, size or self.S, **self.flags)
        o0.initialize_tiles()
        o0.recalculate_palettes()
        tp, pal, pm = o0.tile_palettes, o0.palette, o0.palette_map
        o0.close()
        if count is None and size is None:
            self.set_state(tp, pal)
        return tp, pal, pm

    def _sync(self):
        self.oO.tile_palettes = self.oT.tile_palettes
        self.oO.palette = self.oT.palette
        self.oO.palette_map = self.oT.palette_map

    def optimize(self):
        self.oT.optimize()

    @property
    def palette(self):
        return self.oT.palette

    @property
    def tile_palettes(self):
        return self.oT.tile_palettes

    @property
    def palette_map(self):
        return self.oT.palette_map

    def error(self):
        self._sync()
        return self.oO.error()

    def as_json(self):
        self._sync()
        return self.oO.as_json()

    def reassign_tiles(self):
        return self.oT.reassign_tiles()

    # -- candidates ----------------------------------------------------------------------------------------------------
    def candidates(self, entries, cand, want_maps=False):
        """error() (and map) of the state with every palette entry of `entries` (linear indices) set to the candidate, for
        every candidate; the model is left as it was."""
        pal, pm = self.oT.palette, self.oT.palette_map
        errs, maps = [], []
        for c in np.asarray(cand, np.uint8).reshape(-1, 3):
            p2 = pal.copy()
            p2[list(entries)] = c
            self.oT.palette = p2
            self.oT.optimize()
            errs.append(self.error())
            if want_maps:
                maps.append(self.oT.palette_map)
        self.oT.palette = pal
        self.oT.palette_map = pm
        return (np.array(errs), np.array(maps)) if want_maps else np.array(errs)

    def call(self, method, entries, channel, seed, step_id, n_random=0, guard=True):
        """One optimizer call (lib.rs:191-328 with the acceptance of lib.rs:216-219: strict <, ascending k) on the slot made
        of `entries` -> (error after, the slot's colour after, changed)."""
        before = self.oT.palette[entries[0]].copy()
        if method == 0:
            cand = self.O.random_candidates(seed, step_id, n_random or 64)
        else:
            assert method == 1, "the model covers the random and the channel method"
            cand = np.repeat(before[None, :], 32, 0)
            cand[:, channel] = np.arange(32)
        inc = self.error()
        errs = self.candidates(entries, cand)
        best, best_k = inc, -1
        for k, e in enumerate(errs):
            if guard:
                check_gap(e, best)
            gap = abs(e - best) / best
            if gap > 0.0:
                self.min_gap = min(self.min_gap, gap)
            if e < best:
                best, best_k = e, k
        if best_k >= 0:
            pal = self.oT.palette
            pal[list(entries)] = cand[best_k]
            self.oT.palette = pal
        self.oT.optimize()  # lib.rs:237
        after = self.oT.palette[entries[0]].copy()
        return best, after, int(not np.array_equal(after, before))

    def tile_oracle(self):
        """What tests/tile_model.py drives: an object whose optimize() chooses against T and whose error() compares with the
        original."""
        return _TileView(self)


class _TileView:
    def __init__(self, m):
        self.m = m

    tile_palettes = property(lambda self: self.m.oT.tile_palettes, lambda self, v: setattr(self.m.oT, "tile_palettes", v))
    palette_map = property(lambda self: self.m.oT.palette_map, lambda self, v: setattr(self.m.oT, "palette_map", v))

    def optimize(self):
        self.m.oT.optimize()

    def error(self):
        return self.m.error()


def trajectory(O, img, count, size, flags, table, n_calls, seed, state=(0, 0, 0, 0), guard=True):
    """The model's run of n_calls scheduled calls from the k-means start -> (model, records, final state); records[j] holds
    everything observable after call j.  step_id of call j is j."""
    m = Model(O, img, count, size, flags, table)
    m.kmeans_start()
    sched_all = O.schedule(count, size, 6 * count * size * 3 + n_calls + 8, bool(flags.get("nes")))
    start = next(k for k, r in enumerate(sched_all) if r[1:] == tuple(state))
    recs = []
    for j in range(n_calls):
        method, p, i, ch, _ = sched_all[start + j]
        e, rgb, changed = m.call(method, [p * size + i], ch, seed, j, 0, guard)
        recs.append(dict(method=method, p=p, i=i, ch=ch, error=e, rgb5=rgb, changed=changed, palette=m.palette, pmap=m.palette_map))
    return m, recs, sched_all[start + n_calls][1:]
