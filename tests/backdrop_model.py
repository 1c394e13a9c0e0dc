"""The model of a backdrop context (include/snesimage_hip.h: SNES_BACKDROP) over the unchanged CPU oracle.

A backdrop context (C, S, flags | BACKDROP) is the oracle's EXPANDED context (C, S + 1, flags) whose entries (p, S) hold the
backdrop colour B and change together.  Regular calls are `oracle.step` on that context; a tied candidate is: column S :=
candidate, optimize(), error().  Everything here runs on the CPU."""
import json

import numpy as np

REL_ERR = 1e-11
MIN_GAP = 1e-9  # premise of every decision compared: two errors are equal exactly or differ by more than this (relative)

FLAG_SETS = {
    "rgb": dict(),
    "perceptual": dict(perceptual=True),
    "dither": dict(dither=True),
    "dither_perceptual": dict(dither=True, perceptual=True),
}


def image(h, seed=0, variant=0):
    from snesimage_amd.synth import synth_image
    return synth_image(0x5EED0B00 + 16 * h + seed, 256, h, variant)


def mean_backdrop(img, O=None, nes=False, perceptual=False):
    """B as snesimage_create sets it: per channel (sum over opaque pixels + n/2) / n in integers, then >> 3."""
    opaque = img[..., 3] != 0
    n = int(opaque.sum())
    if n == 0:
        return np.zeros(3, np.uint8)
    b = np.array([((int(img[..., c][opaque].astype(np.int64).sum()) + n // 2) // n) >> 3 for c in range(3)], np.uint8)
    return O.new_nes_only(b, perceptual) if nes else b


def check_gap(e, ref):
    gap = abs(e - ref) / ref
    assert gap == 0.0 or gap > MIN_GAP, "the input breaks the premise: error %r against %r (gap %.3e)" % (e, ref, gap)


def linear_to_slot(L, C, S):
    """Index map of the backdrop schedule: L < C*S is (L / S, L % S), L == C*S the backdrop slot (C, 0)."""
    return (L // S, L % S) if L < C * S else (C, 0)


def model_schedule(O, C, S, n_calls, nes=False):
    """snesimage_schedule_next_backdrop as the oracle's scheduler on geometry (1, C*S + 1)."""
    return [(m,) + linear_to_slot(i, C, S) + (ch, st) for (m, _, i, ch, st) in O.schedule(1, C * S + 1, n_calls, nes)]


class Model:
    def __init__(self, O, img, C, S, flags, init="kmeans"):
        self.O, self.C, self.S, self.flags, self.img = O, C, S, dict(flags), img
        self.o = O.OracleImage(img, C, S + 1, **flags)
        self.B = mean_backdrop(img, O, bool(flags.get("nes")), bool(flags.get("perceptual")))
        if init == "kmeans":  # the reference's initialisers on the regular entries, at (C, S)
            o0 = O.OracleImage(img, C, S, **flags)
            o0.initialize_tiles()
            o0.recalculate_palettes()
            self.o.tile_palettes = o0.tile_palettes
            self.set_state(o0.palette, self.B)
            self.regular0, self.tiles0 = o0.palette, o0.tile_palettes
            o0.close()
        else:
            self.set_state(np.zeros((C * S, 3), np.uint8), self.B)

    # -- state: the regular entries (C*S, 3) and B <-> the expanded palette ---------------------------------------
    def expanded(self, regular, B):
        pal = np.zeros((self.C, self.S + 1, 3), np.uint8)
        pal[:, :self.S] = np.asarray(regular, np.uint8).reshape(self.C, self.S, 3)
        pal[:, self.S] = B
        return pal.reshape(-1, 3)

    def set_state(self, regular, B):
        self.B = np.array(B, np.uint8)
        self.o.palette = self.expanded(regular, B)
        self.o.optimize()

    @property
    def regular(self):
        return self.o.palette.reshape(self.C, self.S + 1, 3)[:, :self.S].reshape(-1, 3).copy()

    @property
    def palette_map(self):
        return self.o.palette_map

    def error(self):
        return self.o.error()

    # -- the tied slot -----------------------------------------------------------------------------------------------
    def tied_candidates(self, cand, want_maps=False):
        """errors (and maps) of the candidates for B; the model is left as it was."""
        pal, pm = self.o.palette, self.o.palette_map
        errs, maps = [], []
        for c in np.asarray(cand, np.uint8).reshape(-1, 3):
            self.o.palette = self.expanded(self.regular_of(pal), c)
            self.o.optimize()
            errs.append(self.o.error())
            if want_maps:
                maps.append(self.o.palette_map)
        self.o.palette = pal
        self.o.palette_map = pm
        return (np.array(errs), np.array(maps)) if want_maps else np.array(errs)

    def regular_of(self, pal):
        return pal.reshape(self.C, self.S + 1, 3)[:, :self.S].reshape(-1, 3)

    def tied_step(self, method, channel, seed, step_id, n_random=0, guard=True):
        """One optimizer call on the backdrop slot -> (error after, B after, changed)."""
        O = self.O
        if method == 0:
            cand = O.random_candidates(seed, step_id, n_random or 64)
        elif method == 1:
            cand = np.repeat(self.B[None, :], 32, 0)
            cand[:, channel] = np.arange(32)
        else:
            cand = np.array([O.nes_color(i) for i in range(56)], np.uint8)
        inc = self.o.error()
        errs = self.tied_candidates(cand)
        best, best_k = (inc, -1) if method != 2 else (float("inf"), 0)
        for k, e in enumerate(errs):
            if guard and np.isfinite(best):
                check_gap(e, best)
            if e < best:
                best, best_k = e, k
        changed = 0
        if best_k >= 0:
            changed = int(not np.array_equal(cand[best_k], self.B))
            self.set_state(self.regular, cand[best_k])
        else:
            self.o.optimize()  # lib.rs:237
        return (best if best_k >= 0 else inc), self.B.copy(), changed

    def call(self, method, p, i, ch, seed, step_id, n_random=0, guard=True):
        """One scheduled call, regular or backdrop -> (error after, the slot's colour after, changed)."""
        if p == self.C:
            return self.tied_step(method, ch, seed, step_id, n_random, guard)
        before = self.o.palette[p * (self.S + 1) + i].copy()
        if guard and method != 2:
            inc = self.o.error()
            cand = self.O.random_candidates(seed, step_id, n_random or 64) if method == 0 else None
            if cand is None:
                cand = np.repeat(before[None, :], 32, 0)
                cand[:, ch] = np.arange(32)
            best = inc
            for e in self.o.score_candidates(p, i, cand):
                check_gap(e, best)
                best = min(best, e)
        e, rgb = self.o.step(method, p, i, ch, seed, step_id, n_random if method == 0 else 0)
        return e, rgb, int(not np.array_equal(rgb, before))

    # -- JSON --------------------------------------------------------------------------------------------------------
    def as_json(self):
        return model_json(self.O, self.regular, self.B, self.o.tile_palettes, self.o.palette_map, self.img, self.C, self.S)

    def as_rgba(self):
        return self.o.as_rgba()


def model_json(O, regular, B, tile_palettes, pmap, img, C, S):
    """lib.rs:579-625 with the backdrop rules: slot 0 of every palette row holds B as a BGR555 word; `tiles` holds 0 for a
    transparent or a backdrop pixel, else map + 1.  Keys sorted, no spaces (serde_json)."""
    h, w = pmap.shape
    regular = np.asarray(regular, np.uint8).reshape(C, S, 3)
    b16 = O.snes_as_u16(B) if O is not None else int(B[0]) | (int(B[1]) << 5) | (int(B[2]) << 10)
    pal = []
    for p in range(C):
        for i in range(16):
            if i == 0:
                pal.append(b16)
            elif i <= S:
                c = regular[p, i - 1]
                pal.append(O.snes_as_u16(c) if O is not None else int(c[0]) | (int(c[1]) << 5) | (int(c[2]) << 10))
            else:
                pal.append(0)
    tiles = []
    for ty in range(h // 8):
        for tx in range(w // 8):
            t = []
            for y in range(8):
                for x in range(8):
                    yy, xx = ty * 8 + y, tx * 8 + x
                    m = int(pmap[yy, xx])
                    t.append(0 if (img[yy, xx, 3] == 0 or m == S) else m + 1)
            tiles.append(t)
    d = {"palette": pal, "tile_palettes": [int(v) for v in tile_palettes[:(w // 8) * (h // 8)]], "tiles": tiles}
    return json.dumps(d, separators=(",", ":"), sort_keys=True)


def trajectory(O, img, C, S, flags, n_calls, seed, state=(0, 0, 0, 0), n_random=0, guard=True, B0=None):
    """The model's run of n_calls scheduled calls -> (model, records, final state); records[j] = dict of everything
    observable after call j.  step_id of call j is j."""
    nes = bool(flags.get("nes"))
    m = Model(O, img, C, S, flags)
    if B0 is not None:  # start from another backdrop colour than the mean
        m.set_state(m.regular, B0)
    # scheduler state in linear terms
    sched_all = model_schedule(O, C, S, 6 * (C * S + 1) * 3 + n_calls + 8, nes)
    start = next(k for k, r in enumerate(sched_all) if r[1:] == tuple(state))
    recs = []
    for j in range(n_calls):
        method, p, i, ch, st = sched_all[start + j]
        e, rgb, changed = m.call(method, p, i, ch, seed, j, n_random, guard)
        recs.append(dict(method=method, p=p, i=i, ch=ch, error=e, rgb5=np.array(rgb), changed=changed, regular=m.regular, B=m.B.copy(),
                         pmap=m.palette_map))
    return m, recs, sched_all[start + n_calls][1:]
