"""The model of per-tile ordered-dither levels (include/snesimage_hip.h: "level call", "level sweep") over the unchanged CPU
oracle, beside tests/ordered_model.py.

A bank of L tables gives L target images T_l = clamp(orig + bank[l][y % n][x % n]).  One oracle per level, built from T_l and
holding the common tile_palettes and palette, runs optimize() once per level and palette; a pixel's choice depends on T at
that pixel alone, so the map of any assignment of levels to tiles is composed tile-wise from those L maps, and a level
candidate is the current map with one tile's block taken from another level's.  error() goes through an oracle over the
original.  Everything here runs on the CPU."""
import numpy as np

import ordered_model as OM

REL_ERR = OM.REL_ERR
MIN_GAP = OM.MIN_GAP
image, with_hole, bayer = OM.image, OM.with_hole, OM.bayer


def ladder(n, amplitude, L):
    """The CLI's bank: level 0 = zeros, level j = Bayer n at amplitude A*j/(L-1) in integer division."""
    assert 2 <= L <= 8 and amplitude >= L - 1
    return np.stack([np.zeros((n, n), np.int8)] + [bayer(n, amplitude * j // (L - 1)) for j in range(1, L)])


def tile_mask(h, levels):
    """(h, 256) array of every pixel's level."""
    lv = np.asarray(levels, np.uint8)[:32 * (h // 8)].reshape(h // 8, 32)
    return np.repeat(np.repeat(lv, 8, 0), 8, 1)


def target_image(img, bank, levels):
    """T: per pixel the offset of its tile's table, phase in image coordinates; alpha kept."""
    bank = np.asarray(bank)
    h = img.shape[0]
    mask = tile_mask(h, levels)
    out = img.copy()
    for l in range(bank.shape[0]):
        t = OM.target_image(img, bank[l])
        out[mask == l] = t[mask == l]
    return out


class Model:
    """count x size is the geometry the oracles run at: for a backdrop context the expanded one (size + 1, column `size` = B)."""

    def __init__(self, O, img, count, size, flags, bank, start_level=0):
        self.O, self.C, self.S, self.flags, self.img = O, count, size, dict(flags), img
        self.bank = np.asarray(bank, np.int8)
        self.L, self.h = self.bank.shape[0], img.shape[0]
        self.ntile = 32 * (self.h // 8)
        self.levels = np.zeros(1024, np.uint8)
        self.levels[:self.ntile] = start_level  # (the rows of tiles below the image stay 0)
        self.oL = [O.OracleImage(OM.target_image(img, self.bank[l]), count, size, **flags) for l in range(self.L)]
        self.oO = O.OracleImage(img, count, size, **flags)
        self.maps = None      # per level: optimize() of the current palette against T_l
        self.palette_map = None
        self.min_gap = float("inf")

    def close(self):
        for o in self.oL + [self.oO]:
            o.close()

    # -- state ---------------------------------------------------------------------------------------------------------
    @property
    def T(self):
        return target_image(self.img, self.bank, self.levels)

    @property
    def tile_palettes(self):
        return self.oL[0].tile_palettes

    @property
    def palette(self):
        return self.oL[0].palette

    def compose(self, levels):
        mask = tile_mask(self.h, levels)
        out = np.zeros((self.h, 256), np.uint8)
        for l in range(self.L):
            out[mask == l] = self.maps[l][mask == l]
        return out

    def set_state(self, tile_palettes, palette):
        """optimize() once per level for this palette; the map of the current levels."""
        self.maps = []
        for o in self.oL:
            o.tile_palettes = tile_palettes
            o.palette = palette
            o.optimize()
            self.maps.append(o.palette_map)
        self.oO.tile_palettes = tile_palettes
        self.oO.palette = palette
        self.palette_map = self.compose(self.levels)

    def set_levels(self, levels):
        lv = np.zeros(1024, np.uint8)
        lv[:self.ntile] = np.asarray(levels, np.uint8)[:self.ntile]
        assert lv.max() < self.L
        self.levels = lv
        if self.maps is not None:
            self.palette_map = self.compose(self.levels)

    def kmeans_start(self, count=None, size=None):
        """The reference's initialisers on the original (a plain oracle) -> (tile_palettes, palette); the model takes them as
        its state where the geometry is its own."""
        o0 = self.O.OracleImage(self.img, count or self.C, size or self.S, **self.flags)
        o0.initialize_tiles()
        o0.recalculate_palettes()
        tp, pal = o0.tile_palettes, o0.palette
        o0.close()
        if count is None and size is None:
            self.set_state(tp, pal)
        return tp, pal

    def error_of(self, pmap):
        self.oO.palette_map = pmap
        return self.oO.error()

    def error(self):
        return self.error_of(self.palette_map)

    # -- candidates ----------------------------------------------------------------------------------------------------
    def candidate_map(self, tile, level):
        y, x = 8 * (tile // 32), 8 * (tile % 32)
        m = self.palette_map.copy()
        m[y:y + 8, x:x + 8] = self.maps[level][y:y + 8, x:x + 8]
        return m

    def candidate(self, tile, level):
        """(error, map) of the state with `tile` on `level`; the model is left as it was."""
        m = self.candidate_map(tile, level)
        return self.error_of(m), m

    def level_call(self, tile, inc, guard=True):
        """One level call -> (incumbent error after, the tile's level after, changed)."""
        cur = int(self.levels[tile])
        best, best_l, best_map = inc, -1, None
        for l in range(self.L):
            if l == cur:
                continue
            e, m = self.candidate(tile, l)
            if guard:
                OM.check_gap(e, best)
            gap = abs(e - best) / best
            if gap > 0.0:
                self.min_gap = min(self.min_gap, gap)
            if e < best:
                best, best_l, best_map = e, l, m
        if best_l >= 0:
            self.levels[tile] = best_l
            self.palette_map = best_map
        return best, (best_l if best_l >= 0 else cur), int(best_l >= 0)

    def level_sweep(self, first_tile=0, n_tiles=None, inc=None, guard=True):
        """-> list of (error, level, changed), one per tile."""
        n_tiles = self.ntile - first_tile if n_tiles is None else n_tiles
        inc = self.error() if inc is None else inc
        log = []
        for t in range(first_tile, first_tile + n_tiles):
            inc, lv, ch = self.level_call(t, inc, guard)
            log.append((inc, lv, ch))
        return log

    def slot_model(self):
        """An ordered_model.Model whose target image is T(level), in this model's state: what the optimizer's calls run on."""
        m = OM.Model(self.O, self.img, self.C, self.S, self.flags, None)
        m.oT.close()
        m.T = self.T
        m.oT = self.O.OracleImage(m.T, self.C, self.S, **self.flags)
        m.set_state(self.tile_palettes, self.palette)
        return m


def assert_log_matches(log, want):
    assert len(log) == len(want)
    for j, (r, (e, lv, ch)) in enumerate(zip(log, want)):
        assert int(r["sub"]) == lv and int(r["changed"]) == ch, (j, r, (e, lv, ch))
        assert abs(float(r["error"]) - e) <= REL_ERR * abs(e), (j, float(r["error"]), e)


# The inputs of the GPU tests (tests/test_tile_dither.py), chosen on the CPU (tests/test_level_model.py asserts on every one that
# the model's sweep holds the gap premise at every comparison, accepts and rejects at least one call, and moves at least one
# tile away from the start level): name -> (h, hole, count, size, flags, backdrop, n, amplitude, L, image seed)
CASES = {
    "row-2x3-L2": (8, False, 2, 3, {}, False, 4, 64, 2, 0),                                         # one tile row
    "wrap16-4x7-L4": (24, False, 4, 7, {}, False, 16, 64, 4, 0),                                    # the 16 x 16 pattern wraps inside the last tile row
    "hole-2x3-L4-perceptual": (24, True, 2, 3, dict(perceptual=True), False, 8, 48, 4, 0),          # whole and partly transparent tiles
    "backdrop-2x3-L2": (24, False, 2, 3, {}, True, 4, 64, 2, 0),
}


def case_setup(O, name):
    return setup(O, CASES[name])


def setup(O, spec):
    """-> (img, bank, start_level, model at the k-means start, backdrop B or None) of a tuple laid out as CASES' values.  For
    a backdrop case the model runs at the expanded geometry with column `size` = B (the mean of the opaque pixels)."""
    h, hole, count, size, flags, backdrop, n, amp, L, seed = spec
    img = image(h, seed)
    if hole:
        img = with_hole(img)
    bank = ladder(n, amp, L)
    if not backdrop:
        m = Model(O, img, count, size, flags, bank, L - 1)
        m.kmeans_start()
        return img, bank, L - 1, m, None
    import backdrop_model as BM
    B = BM.mean_backdrop(img)
    m = Model(O, img, count, size + 1, flags, bank, L - 1)
    tp, regular = m.kmeans_start(count, size)
    pal = np.zeros((count, size + 1, 3), np.uint8)
    pal[:, :size] = regular.reshape(count, size, 3)
    pal[:, size] = B
    m.set_state(tp, pal.reshape(-1, 3))
    return img, bank, L - 1, m, B


# candidate seed of the flow's optimizer calls, chosen on the CPU so that calls on both sides of the sweep change the palette
FLOW_SEED = {"row-2x3-L2": 1, "wrap16-4x7-L4": 4, "hole-2x3-L4-perceptual": 2, "backdrop-2x3-L2": 1}


def channel_start(O, name):
    """Index of the schedule's first channel call: slot (0, 0), channel 0.  The three calls from there share one slot, so
    whatever the library keeps per slot (the pack, the contested list, the slot contexts' packs) serves all three unless
    something invalidates it."""
    _, _, count, size = CASES[name][:4]
    sched = O.schedule(count, size, 4 * count * size + 1)
    return next(k for k, c in enumerate(sched) if c[0] == 1)


def scheduled_calls(O, m, name, first, n, n_random=64):
    """Calls first .. first + n - 1 of the reference's schedule (regular slots) on T(level) in the model's state; the model
    takes the palette they leave -> [(error, rgb5, changed)]."""
    _, _, count, size = CASES[name][:4]
    sm = m.slot_model()
    out = []
    for j, (method, p, i, ch, _) in list(enumerate(O.schedule(count, size, first + n)))[first:]:
        out.append(sm.call(method, [p * m.S + i], ch, FLOW_SEED[name], j, n_random))
    pal = sm.palette
    sm.close()
    m.set_state(m.tile_palettes, pal)
    return out


def flow(O, name):
    """What a run does, with nothing set or read in between: two random calls and the first channel call of slot (0, 0), a
    level sweep straight behind them, then the slot's other two channel calls and three calls of the next slot.  Every
    comparison holds the gap premise (asserted on the way)."""
    img, bank, start, m, B = case_setup(O, name)
    k0 = channel_start(O, name)
    r = dict(k0=k0, pre=scheduled_calls(O, m, name, 0, 2) + scheduled_calls(O, m, name, k0, 1))
    r["sweep"] = m.level_sweep()
    r.update(levels=m.levels.copy(), T=m.T, min_gap=m.min_gap)
    r["post"] = scheduled_calls(O, m, name, k0 + 1, 5)
    r.update(palette=m.palette, palette_map=m.palette_map)
    m.close()
    return r
