"""The model of guided calls (include/snesimage_hip.h: "guided call", "guided sweep") in numpy integers over the unchanged CPU
oracle, beside tests/ordered_model.py and tests/backdrop_model.py.

cost(u) for all 32,768 BGR555 colours is the definition word for word: the population's colours are collapsed with np.unique
and weighted by their counts, the floor and the keys are uint32, the sums uint64.  The shortlist goes through the oracle
(score_candidates for the errors, the palette setter and optimize() for a commit).  A plain, perceptual or --dither context
and one with an ordered-dither table run on ordered_model.Model (table None: T is the original), a backdrop context on
backdrop_model.Model at the expanded geometry.  Everything here runs on the CPU."""
import numpy as np

import backdrop_model as BM
import ordered_model as OM

REL_ERR = OM.REL_ERR
MIN_GAP = OM.MIN_GAP
NCOL = 32768
NO_FLOOR = 0xFFFFFFFF


def expand5(v):
    v = np.asarray(v).astype(np.int64)
    return (v * 8 + v // 4) & 255


def red_mean_key(c1, c2):
    """color.hpp: red_mean_key on 8-bit triples (last axis r, g, b), broadcasting -> int64."""
    a, b = np.asarray(c1).astype(np.int64), np.asarray(c2).astype(np.int64)
    rs = a[..., 0] + b[..., 0]
    dr, dg, db = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (1024 + rs) * dr * dr + 2048 * dg * dg + (1534 - rs) * db * db


def unpack_u(u):
    u = np.asarray(u)
    return np.stack([u & 31, (u >> 5) & 31, u >> 10], -1).astype(np.uint8)


def pack_u(rgb5):
    c = np.asarray(rgb5).astype(np.int64)
    return c[..., 0] | (c[..., 1] << 5) | (c[..., 2] << 10)


def costs(T, tile_palettes, palette, C, S, p, i):
    """cost(u), u < 32768, of slot (p, i) of the context (C, S) whose palette (C*S raw 5-bit triples) is `palette`; p == -1:
    the tied slot — every opaque pixel, the floor over the entries j != i of the pixel's own subpalette."""
    h = T.shape[0]
    tp = np.asarray(tile_palettes)[:32 * (h // 8)].reshape(h // 8, 32)
    sub = np.repeat(np.repeat(tp, 8, 0), 8, 1)
    opaque = T[..., 3] > 0
    pal8 = expand5(np.asarray(palette).reshape(C, S, 3))
    total = np.zeros(NCOL, np.uint64)
    for q in (range(C) if p < 0 else [p]):
        px = T[..., :3][opaque & (sub == q)]
        if px.shape[0] == 0:
            continue
        col, cnt = np.unique(px, axis=0, return_counts=True)
        m = np.full(col.shape[0], NO_FLOOR, np.int64)
        for j in range(S):
            if j != i:
                m = np.minimum(m, red_mean_key(col, pal8[q, j]))
        m = m.astype(np.uint32)
        x = col.astype(np.int64)
        v8 = expand5(np.arange(32))
        g_term = (2048 * (x[:, 1, None] - v8[None, :]) ** 2).astype(np.uint32)   # [x, g]
        db2 = ((x[:, 2, None] - v8[None, :]) ** 2).astype(np.uint32)              # [x, b]
        weights = None if (cnt == 1).all() else cnt.astype(np.uint64)[:, None, None]
        out = np.zeros((32, 32, 32), np.uint64)                                    # [b, g, r]: u = r | g << 5 | b << 10
        for r in range(32):  # every term and the key itself fit 32 bits (a key is at most 299,505,150)
            rs = x[:, 0] + v8[r]
            base = ((1024 + rs) * (x[:, 0] - v8[r]) ** 2).astype(np.uint32)
            key = (1534 - rs).astype(np.uint32)[:, None, None] * db2[:, :, None]  # [x, b, 1]
            key = key + g_term[:, None, :]                                         # [x, b, g]
            key += base[:, None, None]
            np.minimum(key, m[:, None, None], out=key)
            out[:, :, r] = key.sum(0, dtype=np.uint64) if weights is None else (key * weights).sum(0)
        total += out.reshape(-1)
    return total


def shortlist(cost, current, K=0):
    """The K (0 = 16) colours lowest in (cost, u) but the current one -> (rgb5[K, 3], costs[K])."""
    K = K or 16
    order = np.argsort(cost, kind="stable")  # stable: equal costs stay in ascending u
    order = order[order != int(pack_u(current))][:K]
    return unpack_u(order), cost[order]


class Model:
    """A context (C, S) in the model's state.  backdrop: the oracle runs at (C, S + 1), column S = B, and slot (C, 0) is tied."""

    def __init__(self, O, img, C, S, flags=None, table=None, backdrop=False):
        self.O, self.C, self.S, self.flags, self.img, self.backdrop = O, C, S, dict(flags or {}), img, backdrop
        self.Si = S + 1 if backdrop else S
        if backdrop:
            assert table is None
            self.bm = BM.Model(O, img, C, S, self.flags)
            self.T = img
        else:
            self.om = OM.Model(O, img, C, S, self.flags, table)
            self.om.kmeans_start()
            self.T = self.om.T
            self.direct = table is None  # T is the original: the target-side oracle scores by itself
        self.min_gap = float("inf")

    def close(self):
        if self.backdrop:
            self.bm.o.close()
        else:
            self.om.close()

    # -- state: the internal (expanded) palette, C * Si entries -------------------------------------------------------------
    @property
    def oracle(self):
        return self.bm.o if self.backdrop else self.om.oT

    @property
    def internal(self):
        return self.oracle.palette

    @property
    def palette(self):
        """What OptimizedImage.palette reports: the regular entries."""
        return self.internal.reshape(self.C, self.Si, 3)[:, :self.S].reshape(-1, 3).copy()

    @property
    def B(self):
        return self.internal[self.S].copy()

    @property
    def tile_palettes(self):
        return self.oracle.tile_palettes

    @property
    def palette_map(self):
        return self.oracle.palette_map

    def error(self):
        return self.bm.error() if self.backdrop else self.om.error()

    def set_tile_palettes(self, tp):
        self.oracle.tile_palettes = tp
        self.oracle.optimize()

    def set_internal(self, pal):
        self.oracle.palette = pal
        self.oracle.optimize()

    def entries(self, p, i):
        tied = self.backdrop and p == self.C
        return ([q * self.Si + self.S for q in range(self.C)] if tied else [p * self.Si + i]), tied

    def slots(self):
        """The schedule's slot order: (p, i) with i inner, the tied slot last."""
        return [(p, i) for p in range(self.C) for i in range(self.S)] + ([(self.C, 0)] if self.backdrop else [])

    # -- the definition -------------------------------------------------------------------------------------------------------
    def costs(self, p, i):
        ent, tied = self.entries(p, i)
        return costs(self.T, self.tile_palettes, self.internal, self.C, self.Si, -1 if tied else p, self.S if tied else i)

    def candidates(self, p, i, K=0):
        ent, _ = self.entries(p, i)
        return shortlist(self.costs(p, i), self.internal[ent[0]], K)

    def score(self, p, i, cand):
        ent, tied = self.entries(p, i)
        if self.backdrop:
            return self.bm.tied_candidates(cand) if tied else self.bm.o.score_candidates(p, i, cand)
        return self.om.oT.score_candidates(p, i, cand) if self.direct else self.om.candidates(ent, cand)

    def call(self, p, i, K=0, guard=True):
        """One guided call -> dict of everything observable afterwards."""
        ent, _ = self.entries(p, i)
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
            self.oracle.optimize()  # lib.rs:237
        return dict(p=p, i=i, cand=cand, costs=cost, errs=np.array(errs), error=best, best_k=best_k, rgb5=self.internal[ent[0]].copy(), changed=int(best_k >= 0),
                    palette=self.palette, B=self.B if self.backdrop else None, pmap=self.palette_map)

    def sweep(self, K=0, n=None, guard=True):
        """Guided calls in the schedule's slot order: one sweep, or n calls (behind the last slot comes the first again)."""
        sl = self.slots()
        return [self.call(*sl[j % len(sl)], K, guard) for j in range(len(sl) if n is None else n)]


def image(h, seed, variant=0):
    from snesimage_amd.synth import synth_image
    return synth_image(seed, 256, h, variant)


# The inputs of the GPU tests' trajectories (tests/test_guided.py), chosen on the CPU: tests/test_guided_model.py asserts on every
# one that the model's guided calls hold the gap premise at every comparison and accept and reject at least one call.
# name -> (h, image seed, C, S, flags, backdrop, K, n: guided calls from the k-means start in slot order, wrapping)
CASES = {
    "plain-2x3": (16, 1, 2, 3, {}, False, 16, 8),
    "plain-4x7": (32, 2, 4, 7, {}, False, 8, 8),
    "perceptual-2x3": (16, 1, 2, 3, dict(perceptual=True), False, 16, 8),
    "dither-2x3": (16, 1, 2, 3, dict(dither=True), False, 16, 8),
    "backdrop-2x3": (16, 1, 2, 3, {}, True, 16, 7),  # one whole sweep, the tied slot last
}


def case_model(O, name):
    h, seed, C, S, flags, backdrop, K, n = CASES[name]
    return Model(O, image(h, seed), C, S, flags, None, backdrop)


_trajectories = {}


def trajectory(O, name):
    """The model's guided calls on a case from the k-means start, computed once and left unchanged ->
    dict(img, tp, pal0, B0, err0, K, recs, min_gap)."""
    if name not in _trajectories:
        h, seed, C, S, flags, backdrop, K, n = CASES[name]
        m = case_model(O, name)
        r = dict(img=m.img, C=C, S=S, flags=flags, backdrop=backdrop, K=K, tp=m.tile_palettes, pal0=m.palette, B0=m.B if backdrop else None, map0=m.palette_map, err0=m.error())
        r["recs"] = m.sweep(K, n)
        r["min_gap"] = m.min_gap
        m.close()
        _trajectories[name] = r
    return _trajectories[name]
