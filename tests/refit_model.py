"""The model of the refit of shared characters (include/snesimage_hip.h: "snapshot", "fit", "refit call", "refit sweep") in
numpy over the unchanged CPU oracle, beside character_model.py: the oracle provides the palette_map setter and error();
everything else is integer arithmetic on the model's own red_mean_keys.  A backdrop context is the oracle's expanded context
(C, S + 1), as in character_model.Budget."""
import numpy as np

import character_model as M

Q = np.arange(64)


def mask(f):
    return (7 if f & 1 else 0) | (56 if f & 2 else 0)


def fit_class(orig, pal8, tp, members, flips, cur):
    """The fit of one class.  orig (ntile, 64, 3): the original pixels per tile; pal8 (sub_count, S, 3): 8-bit entries;
    tp: tile -> subpalette; members, flips: the class; cur (64): the representative's map values.
    -> (fitted[64], gain, cost[64, S])."""
    S = pal8.shape[1]
    cost = np.zeros((64, S), np.int64)
    for m, f in zip(members, flips):
        px = np.asarray(orig[m], np.int64)[Q ^ mask(int(f))]  # member m's pixel q ^ mask shows position q
        cost += M.red_mean_keys(px[:, None, :], np.asarray(pal8[tp[m]], np.int64)[None, :, :])
    fitted = cost.argmin(axis=1)  # the first minimum: the lowest v
    gain = int((cost[Q, np.asarray(cur, np.int64)] - cost[Q, fitted]).sum())
    return fitted, gain, cost


def spread(fitted, f):
    """The 64 map values member with flip f takes: map(m; p) = fitted[p ^ mask(f)]."""
    return np.asarray(fitted)[Q ^ mask(int(f))]


class Refit:
    """Refit sweeps on a character_model.Budget: the oracle's map is the state, its palette and tile palettes never change."""

    def __init__(self, bud):
        self.b = bud

    def snapshot(self, orig=None):
        """The eligible classes of the oracle's map, ascending rep, with their fits.  orig: other pixels to fit against than
        the original's (what a fit against a dither target would read)."""
        b = self.b
        pm, chars, rep, flip, U, size = b.state()
        vals = M.tiles_of(pm).astype(np.int64)
        orig = b.orig if orig is None else orig
        out = []
        for r in range(b.ntile):
            if rep[r] != r or size[r] < 2:
                continue
            mem = np.flatnonzero(rep == r)
            if b.pinned[mem].any():
                continue
            fitted, gain, _ = fit_class(orig, b.pal8, b.tp, mem, flip[mem], vals[r])
            out.append(dict(rep=r, members=mem, flips=flip[mem].copy(), fitted=fitted, cur=vals[r].copy(), gain=gain))
        return out

    def candidate_map(self, cls, pm=None):
        vals = M.tiles_of(self.b.o.palette_map if pm is None else pm).copy()
        for m, f in zip(cls["members"], cls["flips"]):
            vals[m] = spread(cls["fitted"], f)
        return M.untile(vals, self.b.h)

    def score(self, cls):
        """error() and map of the class's refit candidate; the oracle is left as it was."""
        o = self.b.o
        pm = o.palette_map
        m = self.candidate_map(cls, pm)
        o.palette_map = m
        e = o.error()
        o.palette_map = pm
        return e, m

    def sweep(self, guard=True):
        """One refit sweep -> (records, accepted, U afterwards)."""
        o = self.b.o
        classes = self.snapshot()
        inc = o.error()
        recs, accepted = [], 0
        for cls in classes:
            rec = dict(rep=cls["rep"], members=len(cls["members"]), gain=cls["gain"], changed=0, scored=0, before=inc)
            if not np.array_equal(cls["fitted"], cls["cur"]):
                rec["scored"] = 1
                pm = o.palette_map
                o.palette_map = self.candidate_map(cls, pm)
                e = o.error()
                if guard:
                    M.check_gap(e, inc)
                if e < inc:
                    inc, rec["changed"] = e, 1
                    accepted += 1
                else:
                    o.palette_map = pm
            rec["error"] = inc
            recs.append(rec)
        U = M.classes(M.characters(o.palette_map, self.b.img, self.b.zero_at))[2]
        return recs, accepted, U
