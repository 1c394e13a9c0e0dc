"""The model of the refit of shared characters across the members of a shared-palette set (include/snesimage_hip.h: "refit
across the members of a set") in numpy over one unchanged CPU oracle image per member: the oracles provide the palette_map
setter and error(); the fit is refit_model.fit_class over the global tiles; classes and members are those of
set_character_model.SetBudget.  Global tile g = member * ntile + tile."""
import numpy as np

import character_model as M
import refit_model as R
import set_character_model as SM
from character_model import MIN_GAP, REL_ERR  # noqa: F401


def joint(errs):
    """The members' errors summed in member order, left to right, as snesimage_shared_error sums."""
    E = 0.0
    for i, e in enumerate(errs):
        E = e if i == 0 else E + e
    return E


def check_gap(E1, E):
    """The premise of every decision compared: E' and E are equal exactly or differ by more than MIN_GAP relative (a GPU error
    is within REL_ERR of the oracle's: a factor of a hundred)."""
    gap = abs(E1 - E) / E
    assert gap == 0.0 or gap > MIN_GAP, "the input breaks the premise: E' %r against E %r (gap %.3e)" % (E1, E, gap)
    return gap


class SetRefit:
    """Refit sweeps on a SetBudget: the oracles' maps are the state, their palette and tile palettes never change."""

    def __init__(self, sb):
        self.sb = sb
        self.orig = np.concatenate([b.orig for b in sb.buds])  # (G, 64, 3)
        self.tp = np.concatenate([b.tp for b in sb.buds])      # global tile -> subpalette (the palette is shared)
        self.pal8 = sb.buds[0].pal8

    def snapshot(self):
        """The eligible classes of the oracles' maps, ascending global rep, with their fits and touched members."""
        sb = self.sb
        chars, rep, flip, U, size = sb.state()
        vals = sb.values()
        out = []
        for r in range(sb.G):
            if rep[r] != r or size[r] < 2:
                continue
            tiles = np.flatnonzero(rep == r)
            if sb.pinned[tiles].any():
                continue
            fitted, gain, _ = R.fit_class(self.orig, self.pal8, self.tp, tiles, flip[tiles], vals[r])
            out.append(dict(rep=r, tiles=tiles, flips=flip[tiles].copy(), fitted=fitted, cur=vals[r].copy(), gain=gain,
                            touched=sorted({int(g) // sb.ntile for g in tiles})))
        return out

    def candidate_maps(self, cls):
        """member -> candidate map, for the touched members."""
        sb = self.sb
        out = {}
        for m in cls["touched"]:
            vals = M.tiles_of(sb.oms[m].palette_map).copy()
            for g, f in zip(cls["tiles"], cls["flips"]):
                if int(g) // sb.ntile == m:
                    vals[int(g) % sb.ntile] = R.spread(cls["fitted"], f)
            out[m] = M.untile(vals, sb.h)
        return out

    def score(self, cls, incs=None):
        """(E', e per member, map per member) of the class's candidate — an untouched member keeps its incumbent and its stored
        map; the oracles are left as they were."""
        sb = self.sb
        incs = [o.error() for o in sb.oms] if incs is None else incs
        es, maps = list(incs), [o.palette_map for o in sb.oms]
        for m, cand in self.candidate_maps(cls).items():
            o = sb.oms[m]
            pm = o.palette_map
            o.palette_map = cand
            es[m] = o.error()
            o.palette_map = pm
            maps[m] = cand
        return joint(es), es, maps

    def sweep(self, guard=True):
        """One refit sweep -> (records, accepted, U afterwards)."""
        sb = self.sb
        incs = [o.error() for o in sb.oms]
        E = joint(incs)
        recs, accepted = [], 0
        for cls in self.snapshot():
            rec = dict(rep=cls["rep"], members=len(cls["tiles"]), touched=len(cls["touched"]), gain=cls["gain"], changed=0, scored=0, before=E,
                       member_rose=False, gap=None)
            if not np.array_equal(cls["fitted"], cls["cur"]):
                rec["scored"] = 1
                E1, es, maps = self.score(cls, incs)
                if guard:
                    rec["gap"] = check_gap(E1, E)
                if E1 < E:
                    rec["member_rose"] = any(es[m] > incs[m] for m in cls["touched"])
                    for m in cls["touched"]:
                        sb.oms[m].palette_map = maps[m]
                    incs, E, rec["changed"] = es, E1, 1
                    accepted += 1
            rec["error"] = E
            recs.append(rec)
        return recs, accepted, M.classes(sb.chars())[2]


# ---- the states of the trajectory tests (tests/test_set_refit.py; their premises: tests/test_set_refit_model.py) ----------------
# (input of set_character_model.TRAJECTORIES, merges of the joint reduction that come first)
STATES = {"dither_6": ("dither_1x15", 6), "dither_26": ("dither_1x15", 26), "rgb_32": ("rgb_2x3", 32)}
_CACHE = {}  # state -> (tile_palettes, palette, the members' maps after the reduction): computed once, never changed


def reduced_state(O, state):
    """Fresh oracle members in the state behind the model's own (guarded) joint reduction -> (imgs, count, size, flags, K, merges,
    oms, SetBudget)."""
    name, merges = STATES[state]
    imgs, count, size, flags, K, _ = SM.trajectory_inputs(name)
    if state not in _CACHE:
        tps, pal = SM.stack_start(O, imgs, count, size, **flags)
        oms = SM.oracle_members(O, imgs, tps, pal, count, size, **flags)
        sb = SM.SetBudget(O, oms, imgs)
        U0 = sb.state()[3]
        recs, U = sb.reduce(U0 - merges, K)
        assert len(recs) == merges and U == U0 - merges
        _CACHE[state] = (tps, pal, [o.palette_map.copy() for o in oms])
        for o in oms:
            o.close()
    tps, pal, maps = _CACHE[state]
    oms = SM.oracle_members(O, imgs, tps, pal, count, size, **flags)
    for o, m in zip(oms, maps):
        o.palette_map = m
    return imgs, count, size, flags, K, merges, oms, SM.SetBudget(O, oms, imgs)
