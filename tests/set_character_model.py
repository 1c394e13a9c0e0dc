"""The model of the character budget of a shared-palette set (include/snesimage_hip.h: "character budget of a shared-palette
set") in numpy beside character_model.py, whose helpers it reuses, over one unchanged CPU oracle image per member: the oracle
provides the palette_map setter and error(); everything else is counting.  Global tile g = member * ntile + tile."""
import json

import numpy as np

import character_model as M
from character_model import MIN_GAP, REL_ERR  # noqa: F401


def stack_start(O, imgs, count, size, **flags):
    """The set's k-means start as it is defined: the oracle's own initialisers on the member stack (the members top to bottom),
    split back by rows -> (tile_palettes per member, palette)."""
    h = imgs[0].shape[0]
    ntile = 32 * (h // 8)
    st = O.OracleImage(np.concatenate(imgs, axis=0), count, size, **flags)
    st.initialize_tiles()
    st.recalculate_palettes()
    tps = []
    for i in range(len(imgs)):
        tp = np.zeros(1024, np.uint8)
        tp[:ntile] = st.tile_palettes[i * ntile:(i + 1) * ntile]
        tps.append(tp)
    pal = st.palette.copy()
    st.close()
    return tps, pal


def oracle_members(O, imgs, tps, pal, count, size, **flags):
    out = []
    for f, tp in zip(imgs, tps):
        o = O.OracleImage(f, count, size, **flags)
        o.tile_palettes = tp
        o.palette = pal
        o.optimize()
        out.append(o)
    return out


class SetBudget:
    """The joint budget over oracle members `oms` (their palettes and tile palettes are never changed; their maps are the state)."""

    def __init__(self, O, oms, imgs):
        self.oms, self.imgs = oms, imgs
        self.buds = [M.Budget(O, o, img) for o, img in zip(oms, imgs)]
        self.F, self.ntile, self.h = len(oms), self.buds[0].ntile, self.buds[0].h
        self.G = self.F * self.ntile
        self.pinned = np.concatenate([b.pinned for b in self.buds])

    def chars(self):
        return np.concatenate([M.characters(o.palette_map, img) for o, img in zip(self.oms, self.imgs)])

    def state(self):
        chars = self.chars()
        return (chars,) + M.classes(chars)

    def values(self):
        return np.concatenate([M.tiles_of(o.palette_map) for o in self.oms]).astype(np.int64)

    def candidates(self):
        """Every (cost, gt, gb, f) of the definition, sorted."""
        chars, rep, flip, U, size = self.state()
        vals = self.values()
        idx = np.arange(self.G)
        donors = idx[(rep == idx) & ~self.pinned]
        px = np.arange(64)
        out = []
        for g in idx[~self.pinned & (size == 1)]:
            m, t = divmod(int(g), self.ntile)
            tab, ds = self.buds[m].table(t), donors[donors != g]
            for f in range(4):
                cost = tab[px[None, :], M.flip_char(vals[ds], f)].sum(axis=1)
                out.extend((int(c), int(g), int(b), f) for c, b in zip(cost, ds))
        out.sort()
        return out

    def shortlist(self, K):
        return self.candidates()[:K]

    def merged_map(self, gt, gb, f):
        m, t = divmod(gt, self.ntile)
        mb, b = divmod(gb, self.ntile)
        vals = M.tiles_of(self.oms[m].palette_map).copy()
        vals[t] = M.flip_char(M.tiles_of(self.oms[mb].palette_map)[b], f)
        return M.untile(vals, self.h)

    def score(self, gt, gb, f):
        """(member error e, map) of the candidate, scored in the recipient's member; the oracles are left as they were."""
        o = self.oms[gt // self.ntile]
        pm = o.palette_map
        m = self.merged_map(gt, gb, f)
        o.palette_map = m
        e = o.error()
        o.palette_map = pm
        return e, m

    def step(self, K, guard=True):
        """One reduction step -> record dict, or None without an eligible pair."""
        short = self.shortlist(K)
        if not short:
            return None
        incs = [o.error() for o in self.oms]
        scored = [self.score(gt, gb, f) for _, gt, gb, f in short]
        ds = [e - incs[gt // self.ntile] for (e, _), (_, gt, _, _) in zip(scored, short)]
        best = None
        for rank, d in enumerate(ds):
            if d != d:
                continue
            if best is not None and guard:
                check_gap(d, ds[best], scored[rank][0], scored[best][0])
            if best is None or d < ds[best]:
                best = rank
        cost, gt, gb, f = short[best]
        m, t = divmod(gt, self.ntile)
        mb, b = divmod(gb, self.ntile)
        self.oms[m].palette_map = scored[best][1]
        incs_after = list(incs)
        incs_after[m] = scored[best][0]
        E0 = E1 = 0.0
        for i in range(self.F):  # member order, as snesimage_shared_error sums
            E0 = incs[i] if i == 0 else E0 + incs[i]
            E1 = incs_after[i] if i == 0 else E1 + incs_after[i]
        finite = [r for r, (e, _) in enumerate(scored) if e == e]
        return dict(error=E1, member_error=scored[best][0], cost=cost, member=m, tile=t, donor_member=mb, donor=b, flip=f, rank=best,
                    unique=M.classes(self.chars())[2], before=E0, lowest_e_rank=min(finite, key=lambda r: (scored[r][0], r)))

    def reduce(self, max_unique, K, guard=True):
        recs = []
        U = self.state()[3]
        while U > max_unique:
            r = self.step(K, guard)
            if r is None:
                break
            assert r["unique"] == U - 1, "a merge takes exactly one class away"
            U = r["unique"]
            recs.append(r)
        return recs, U

    def tilemap_json(self):
        return set_tilemap_json(self.chars(), [o.tile_palettes for o in self.oms])


def set_tilemap_json(chars, tile_palettes):
    """The set's tilemap: `characters` one list for the whole set, the other keys one list per member (tile_palettes: F arrays)."""
    F = len(tile_palettes)
    n = len(chars) // F
    rep, flip, U, _ = M.classes(chars)
    reps = [g for g in range(len(chars)) if rep[g] == g]
    pos = {g: i for i, g in enumerate(reps)}
    per = lambda v: [[int(x) for x in v[i * n:(i + 1) * n]] for i in range(F)]  # noqa: E731
    d = {"characters": [[int(v) for v in chars[g]] for g in reps], "character": per([pos[int(r)] for r in rep]), "hflip": per(flip & 1), "vflip": per(flip >> 1),
         "palette": [[int(v) for v in tp[:n]] for tp in tile_palettes]}
    return json.dumps(d, separators=(",", ":"), sort_keys=True)


def check_gap(d, d_ref, e, e_ref):
    """The premise of every decision: two increases are equal exactly or differ by more than MIN_GAP times the larger of the two
    errors (a GPU error is within REL_ERR of the oracle's, so an increase is uncertain by about 2 * REL_ERR * e: a factor of fifty)."""
    gap = abs(d - d_ref) / max(e, e_ref)
    assert gap == 0.0 or gap > MIN_GAP, "the input breaks the premise: increase %r against %r (gap %.3e)" % (d, d_ref, gap)


def assert_trajectory_decides(recs):
    """The conditions on the inputs of a trajectory test."""
    assert any(r["rank"] > 0 for r in recs), "the proxy's first choice always wins: nothing shows that the shortlist was scored"
    assert any(r["error"] > r["before"] for r in recs), "no step raises E"
    assert any(r["donor_member"] != r["member"] for r in recs), "no merge takes its donor from another member"
    assert any(r["rank"] != r["lowest_e_rank"] for r in recs), "the winner always has the lowest member error: deciding on d rather than on e does not show"


def unflip_set_tilemap(tm):
    """The `tiles` arrays, member by member, a set's tilemap JSON stands for."""
    ch = np.array(tm["characters"], np.uint8)
    return [[M.flip_char(ch[c], h + 2 * v).tolist() for c, h, v in zip(cs, hs, vs)] for cs, hs, vs in zip(tm["character"], tm["hflip"], tm["vflip"])]


# ---- the inputs of the trajectory tests (tests/test_set_characters.py; their premises: tests/test_set_character_model.py) ----

TRAJECTORIES = {  # name: (frames, h, sub_count, sub_size, flags, image seeds, K, steps)
    "rgb_2x3": (2, 32, 2, 3, {}, (0, 1), 4, 12),
    "dither_1x15": (3, 16, 1, 15, {"dither": True}, (0, 1, 2), 4, 6),
}


def trajectory_inputs(name):
    import backdrop_model as B
    F, h, count, size, flags, seeds, K, steps = TRAJECTORIES[name]
    return [B.image(h, s) for s in seeds], count, size, dict(flags), K, steps
