"""The model of per-tile ordered-dither levels on a shared-palette set (include/snesimage_hip.h: "tied level call",
snesimage_shared_level_sweep), beside tests/level_model.py: one level_model.Model per frame, all holding one palette.

A TIED call on tile position t gives every frame's tile t the same level: for every level l other than the common one, E_l is
the frames' candidate errors summed in member order (first, then +), and lib.rs:216-219 decides on E — best := E, a strict
E_l < best is taken, by every frame at once, whatever it does to a single frame's error.  The per-frame sweep is
Model.level_sweep frame after frame.  Everything here runs on the CPU."""
import numpy as np

import level_model as LM
import ordered_model as OM

REL_ERR = LM.REL_ERR
MIN_GAP = LM.MIN_GAP


def total(errors):
    """The set's error: the members' errors summed in member order with plain +, as snesimage_shared_error sums."""
    e = None
    for v in errors:
        e = float(v) if e is None else e + float(v)
    return e


class SetModel:
    def __init__(self, O, imgs, count, size, flags, bank, start_level=0):
        self.O, self.C, self.S, self.flags = O, count, size, dict(flags)
        self.frames = [LM.Model(O, img, count, size, flags, bank, start_level) for img in imgs]
        self.F, self.L, self.ntile = len(self.frames), self.frames[0].L, self.frames[0].ntile
        self.min_gap = float("inf")
        # what tells a tied decision from per-frame decisions, counted over every tied call made
        self.stats = dict(accepted=0, rejected=0, accepted_member_worse=0, rejected_member_alone=0)

    def close(self):
        for m in self.frames:
            m.close()

    def start(self):
        """Every frame's own initialize_tiles(); frame 0's recalculate_palettes() palette for all frames."""
        pal, tps = None, []
        for i, m in enumerate(self.frames):
            o = self.O.OracleImage(m.img, self.C, self.S, **self.flags)
            o.initialize_tiles()
            tps.append(o.tile_palettes)
            if i == 0:
                o.recalculate_palettes()
                pal = o.palette
            o.close()
        for m, tp in zip(self.frames, tps):
            m.set_state(tp, pal)
        return tps, pal

    def set_palette(self, pal):
        for m in self.frames:
            m.set_state(m.tile_palettes, pal)

    def errors(self):
        return [m.error() for m in self.frames]

    def error(self):
        return total(self.errors())

    def candidate(self, tile, level):
        """(E, member errors, maps) of the set with every frame's `tile` on `level`; a frame already on it keeps its map."""
        es, maps = [], []
        for m in self.frames:
            e, mp = m.candidate(tile, level)
            es.append(e)
            maps.append(mp)
        return total(es), es, maps

    def tied_call(self, tile, incs, guard=True):
        """One tied call -> (E after, the common level after, changed); incs (the frames' incumbents) is updated in place."""
        cur = int(self.frames[0].levels[tile])
        assert all(int(m.levels[tile]) == cur for m in self.frames), "the frames differ in level on tile %d" % tile
        E = total(incs)
        best, best_l, best_es, best_maps = E, -1, None, None
        alone = False
        for l in range(self.L):
            if l == cur:
                continue
            El, es, maps = self.candidate(tile, l)
            if guard:
                OM.check_gap(El, best)
            gap = abs(El - best) / best
            if gap > 0.0:
                self.min_gap = min(self.min_gap, gap)
            alone = alone or any(e < inc for e, inc in zip(es, incs))
            if El < best:
                best, best_l, best_es, best_maps = El, l, es, maps
        if best_l < 0:
            self.stats["rejected"] += 1
            self.stats["rejected_member_alone"] += int(alone)
            return best, cur, 0
        self.stats["accepted"] += 1
        self.stats["accepted_member_worse"] += int(any(e > inc for e, inc in zip(best_es, incs)))
        for i, m in enumerate(self.frames):
            m.levels[tile] = best_l
            m.palette_map = best_maps[i]
            incs[i] = best_es[i]
        return best, best_l, 1

    def tied_sweep(self, first_tile=0, n_tiles=None, guard=True):
        """-> list of (E, level, changed), one per tile position."""
        n_tiles = self.ntile - first_tile if n_tiles is None else n_tiles
        incs = self.errors()
        return [self.tied_call(t, incs, guard) for t in range(first_tile, first_tile + n_tiles)]

    def frame_sweep(self, first_tile=0, n_tiles=None, guard=True):
        """Model.level_sweep on every frame, frame after frame -> [F] lists of (error, level, changed)."""
        out = []
        for m in self.frames:
            out.append(m.level_sweep(first_tile, n_tiles, guard=guard))
            self.min_gap = min(self.min_gap, m.min_gap)
        return out

    @property
    def levels(self):
        return np.stack([m.levels for m in self.frames])


# The inputs of the GPU tests (tests/test_set_tile_dither.py): name -> (F, h, hole, count, size, flags, n, amplitude, L, seed);
# frame i is level_model.image(h, seed + i).  tests/test_set_level_model.py asserts on each what makes it a test of a tied decision.
CASES = {
    "set2-row-2x3-L2": (2, 8, False, 2, 3, {}, 4, 64, 2, 0),
    "set3-wrap16-4x7-L4": (3, 24, False, 4, 7, {}, 16, 64, 4, 0),
    "set2-hole-2x3-L4-perceptual": (2, 24, True, 2, 3, dict(perceptual=True), 8, 48, 4, 0),
}


def case_images(name):
    F, h, hole = CASES[name][:3]
    seed = CASES[name][9]
    imgs = [LM.image(h, seed + i) for i in range(F)]
    return [LM.with_hole(im) for im in imgs] if hole else imgs


def case_setup(O, name):
    """-> (images, bank, start level, the set's model in its start state, the frames' tile palettes, the palette)"""
    F, h, hole, count, size, flags, n, amp, L, seed = CASES[name]
    imgs = case_images(name)
    bank = LM.ladder(n, amp, L)
    m = SetModel(O, imgs, count, size, flags, bank, L - 1)
    tps, pal = m.start()
    return imgs, bank, L - 1, m, tps, pal


def assert_log_matches(log, want):
    LM.assert_log_matches(log, want)


def set_call(O, sms, method, entries, channel, seed, step_id, n_random, gaps):
    """One optimizer call of the set (lib.rs:191-328 on E: strict <, ascending k) over the frames' slot models `sms`
    (level_model.Model.slot_model: each frame's T(level)) -> (E after, the slot's colour after, changed)."""
    before = sms[0].oT.palette[entries[0]].copy()
    if method == 0:
        cand = O.random_candidates(seed, step_id, n_random or 64)
    else:
        assert method == 1, "the model covers the random and the channel method"
        cand = np.repeat(before[None, :], 32, 0)
        cand[:, channel] = np.arange(32)
    best, best_k = total([s.error() for s in sms]), -1
    errs = [s.candidates(entries, cand) for s in sms]
    for k in range(len(cand)):
        E = total([e[k] for e in errs])
        OM.check_gap(E, best)
        gap = abs(E - best) / best
        if gap > 0.0:
            gaps.append(gap)
        if E < best:
            best, best_k = E, k
    for s in sms:
        if best_k >= 0:
            pal = s.oT.palette
            pal[list(entries)] = cand[best_k]
            s.oT.palette = pal
        s.oT.optimize()  # lib.rs:237
    after = sms[0].oT.palette[entries[0]].copy()
    return best, after, int(not np.array_equal(after, before))


# candidate seed of the flow's optimizer calls, chosen on the CPU so that some of the calls behind the sweep change the palette
FLOW_SEED = {"set2-row-2x3-L2": 3, "set2-hole-2x3-L4-perceptual": 1}
FLOW_CALLS, FLOW_RANDOM = 6, 8


def flow(O, name):
    """A tied sweep from the start state, then FLOW_CALLS scheduled calls of the set on the T(level) it left."""
    F, h, hole, count, size = CASES[name][:5]
    imgs, bank, start, m, tps, pal = case_setup(O, name)
    r = dict(sweep=m.tied_sweep(), levels=m.levels, T=[f.T for f in m.frames], maps1=[f.palette_map for f in m.frames])
    sms, gaps, calls = [f.slot_model() for f in m.frames], [], []
    for j, (method, p, i, ch, _) in enumerate(O.schedule(count, size, FLOW_CALLS)):
        calls.append(set_call(O, sms, method, [p * size + i], ch, FLOW_SEED[name], j, FLOW_RANDOM, gaps))
    r.update(calls=calls, palette=sms[0].palette, maps2=[s.palette_map for s in sms], E2=total([s.error() for s in sms]), min_gap=min(gaps + [m.min_gap]))
    for s in sms:
        s.close()
    m.close()
    return r
