"""The model of the guided calls of a shared-palette set (include/snesimage_hip.h: "guided calls of a set"; DESIGN 5f') in numpy
integers over the unchanged CPU oracle, beside tests/guided_model.py and tests/set_backdrop_model.py.

The cost table of a set is the sum over the members of guided_model.costs(T_f, tile_palettes_f, internal palette, C, S or S + 1,
...); the shortlist is guided_model.shortlist; errors are the members' score_candidates summed in member order, as
set_backdrop_model.SetModel sums them; acceptance is strict < against the summed incumbents.  A plain set starts from the stacked
oracle's initialize_tiles + recalculate_palettes; a backdrop set is built on set_backdrop_model.SetModel.  CPU only."""
import numpy as np

import guided_model as GM
import ordered_model as OM
import set_backdrop_model as SB

REL_ERR = GM.REL_ERR
MIN_GAP = GM.MIN_GAP


def set_costs(Ts, tiles, internal, C, Si, p, i):
    """cost(u) of the set: the members' tables added, in integers.  p == -1: the tied slot."""
    total = np.zeros(GM.NCOL, np.uint64)
    for T, tp in zip(Ts, tiles):
        total += GM.costs(T, tp, internal, C, Si, p, i)
    return total


class PlainSet:
    """F oracle contexts at (C, S) holding one palette; joint errors summed in member order."""

    def __init__(self, O, imgs, C, S, flags, init=True):
        self.O, self.C, self.S, self.flags, self.imgs = O, C, S, dict(flags), imgs
        self.per = 32 * (imgs[0].shape[0] // 8)
        self.o = [O.OracleImage(img, C, S, **self.flags) for img in imgs]
        if init:
            st = O.OracleImage(np.concatenate(imgs, axis=0), C, S, **self.flags)
            st.initialize_tiles()
            st.recalculate_palettes()
            for f, o in enumerate(self.o):
                t = np.zeros(1024, np.uint8)
                t[:self.per] = st.tile_palettes[f * self.per:(f + 1) * self.per]
                o.tile_palettes = t
            self.set_palette(st.palette)
            st.close()

    def close(self):
        for o in self.o:
            o.close()

    def set_palette(self, pal):
        for o in self.o:
            o.palette = pal
            o.optimize()

    def set_tiles(self, tiles):
        for o, t in zip(self.o, tiles):
            o.tile_palettes = t
            o.optimize()

    def error(self):
        E = 0.0
        for o in self.o:
            E = E + o.error()
        return E

    def score(self, p, i, cand):
        E = None
        for o in self.o:
            e = o.score_candidates(p, i, cand)
            E = e if E is None else E + e
        return E


class SetModel:
    """A set (C, S) of the frames `imgs` in the model's state.  backdrop: None — a plain set; else B (three 5-bit values)."""

    def __init__(self, O, imgs, C, S, flags=None, backdrop=None):
        self.O, self.C, self.S, self.flags, self.imgs = O, C, S, dict(flags or {}), imgs
        self.backdrop = backdrop is not None
        self.Si = S + 1 if self.backdrop else S
        if self.backdrop:
            self.sb = SB.SetModel(O, imgs, C, S, self.flags)
            self.sb.set_state(self.sb.regular, backdrop)
            self.oracles = [m.o for m in self.sb.m]
        else:
            self.ps = PlainSet(O, imgs, C, S, self.flags)
            self.oracles = self.ps.o
        self.min_gap = float("inf")

    def close(self):
        (self.sb if self.backdrop else self.ps).close()

    # -- state ------------------------------------------------------------------------------------------------------------
    @property
    def internal(self):
        return self.oracles[0].palette

    @property
    def palette(self):
        return self.internal.reshape(self.C, self.Si, 3)[:, :self.S].reshape(-1, 3).copy()

    @property
    def B(self):
        return self.internal[self.S].copy() if self.backdrop else None

    @property
    def tiles(self):
        return [o.tile_palettes for o in self.oracles]

    @property
    def pmaps(self):
        return [o.palette_map for o in self.oracles]

    def error(self):
        return self.sb.error() if self.backdrop else self.ps.error()

    def set_internal(self, pal):
        for o in self.oracles:
            o.palette = pal
            o.optimize()

    def set_tiles(self, tiles):
        for o, t in zip(self.oracles, tiles):
            o.tile_palettes = t
            o.optimize()

    def entries(self, p, i):
        tied = self.backdrop and p == self.C
        return ([q * self.Si + self.S for q in range(self.C)] if tied else [p * self.Si + i]), tied

    def slots(self):
        return [(p, i) for p in range(self.C) for i in range(self.S)] + ([(self.C, 0)] if self.backdrop else [])

    # -- the definition -----------------------------------------------------------------------------------------------------
    def costs(self, p, i, Ts=None):
        _, tied = self.entries(p, i)
        return set_costs(self.imgs if Ts is None else Ts, self.tiles, self.internal, self.C, self.Si, -1 if tied else p, self.S if tied else i)

    def candidates(self, p, i, K=0):
        ent, _ = self.entries(p, i)
        return GM.shortlist(self.costs(p, i), self.internal[ent[0]], K)

    def score(self, p, i, cand):
        if self.backdrop:
            return self.sb.score_candidates(p, i, cand)
        return self.ps.score(p, i, cand)

    def call(self, p, i, K=0, guard=True):
        """One guided call of the set -> dict of everything observable afterwards."""
        ent, tied = self.entries(p, i)
        cand, cost = self.candidates(p, i, K)
        inc = self.error()
        errs = self.score(p, i, cand)
        best, best_k = inc, -1
        for k, e in enumerate(errs):
            if guard:
                OM.check_gap(e, best)
            gap = abs(e - best) / best
            if gap > 0.0:
                self.min_gap = min(self.min_gap, gap)
            if e < best:
                best, best_k = e, k
        if best_k >= 0:
            pal = self.internal
            pal[ent] = cand[best_k]
            self.set_internal(pal)
        else:
            for o in self.oracles:
                o.optimize()  # lib.rs:237
        return dict(p=p, i=i, tied=tied, cand=cand, costs=cost, errs=np.array(errs), error=best, best_k=best_k, rgb5=self.internal[ent[0]].copy(), changed=int(best_k >= 0),
                    palette=self.palette, B=self.B, pmaps=self.pmaps)

    def sweep(self, K=0, n=None, guard=True):
        """Guided calls in the schedule's slot order: one sweep, or n calls (behind the last slot comes the first again)."""
        sl = self.slots()
        return [self.call(*sl[j % len(sl)], K, guard) for j in range(len(sl) if n is None else n)]


# The trajectories the GPU tests follow (tests/test_set_guided.py): frames set_backdrop_model.frames(F, H) (seed 0x5EED5B00,
# variant 0), the stacked k-means start, calls in slot order, wrapping.  tests/test_set_guided_model.py asserts on every one that
# the gap premise holds at every comparison and that calls accept and reject.
# name -> (F, H, C, S, flags, B0 (None: a plain set), K, calls)
CASES = {
    "plain-f2-2x3": (2, 16, 2, 3, {}, None, 16, 8),
    "plain-f3-2x3": (3, 16, 2, 3, {}, None, 16, 8),
    "plain-f2-4x7": (2, 16, 4, 7, {}, None, 8, 12),
    "perceptual-f2-2x3": (2, 16, 2, 3, dict(perceptual=True), None, 16, 8),
    "dither-f2-2x3": (2, 16, 2, 3, dict(dither=True), None, 16, 8),
    "backdrop-f2-2x3": (2, 16, 2, 3, {}, (31, 31, 31), 16, 7),  # one whole sweep, the tied slot last; from the stack mean the tied call rejects
}


def case_model(O, name):
    F, H, C, S, flags, B0, K, n = CASES[name]
    return SetModel(O, SB.frames(F, H), C, S, flags, B0)


_trajectories = {}


def trajectory(O, name):
    """The model's guided calls on a case, computed once and left unchanged."""
    if name not in _trajectories:
        F, H, C, S, flags, B0, K, n = CASES[name]
        m = case_model(O, name)
        r = dict(imgs=m.imgs, C=C, S=S, flags=flags, backdrop=m.backdrop, K=K, tiles=m.tiles, pal0=m.palette, B0=m.B, maps0=m.pmaps, err0=m.error())
        r["recs"] = m.sweep(K, n)
        r["min_gap"] = m.min_gap
        m.close()
        _trajectories[name] = r
    return _trajectories[name]
