"""The model of the CIELAB proxy of guided calls (include/snesimage_hip.h: "the CIELAB proxy of guided calls"; DESIGN 5f'') over
the unchanged CPU oracle, beside tests/guided_model.py and tests/set_guided_model.py, whose models it reuses for everything but
the table.

d(c, x) comes from oracle_py.distance_cielab(entry, target), called once per (distinct opaque colour of T, u) and cached per
colour in this module: d(c, T) does not depend on the slot.  To keep that affordable the pictures carry at most 16 distinct
opaque colours (`posterise`; an ordered-dither picture uses 2, which its table spreads).  q, the floor and the sums are
integers, uint64.  Everything here runs on the CPU."""
import numpy as np

import guided_model as GM
import ordered_model as OM
import set_backdrop_model as SB
import set_guided_model as SGM

NCOL = GM.NCOL
QMAX = 0xFFFFFF
NO_FLOOR = 0xFFFFFFFF

_RGB8 = GM.expand5(GM.unpack_u(np.arange(NCOL))).astype(np.uint8)  # rgb8(c_u)
_dist = {}


def q(d):
    """min((uint32_t)(d * 65536.0f), 0xFFFFFF) on f32 values -> uint64.  The product by 2^16 is exact in f32."""
    d = np.asarray(d, np.float32)
    return np.minimum((d * np.float32(65536.0)).astype(np.uint64), np.uint64(QMAX))


def distances(O, colour):
    """d(c_u, colour) for all 32,768 u as f32: the oracle's distance_cielab(entry, target), once per colour."""
    key = tuple(int(v) for v in colour)
    if key not in _dist:
        t = np.array(key, np.uint8)
        _dist[key] = np.array([O.distance_cielab(_RGB8[u], t) for u in range(NCOL)], np.float32)
    return _dist[key]


def posterise(img, two=False):
    """At most 16 distinct opaque colours (two: 2): the top bit of r and g and the top two bits of b, with fixed low bits ORed in
    so that no colour is the 8-bit expansion of a BGR555 value.  Alpha is kept."""
    out = img.copy()
    if two:
        hi = img[..., 1] > np.median(img[..., 1])
        out[..., 0], out[..., 1], out[..., 2] = np.where(hi, 0xB3, 0x33), np.where(hi, 0xB3, 0x33), np.where(hi, 0x59, 0x99)
    else:
        out[..., 0] = (img[..., 0] & 0x80) | 0x33
        out[..., 1] = (img[..., 1] & 0x80) | 0x33
        out[..., 2] = (img[..., 2] & 0xC0) | 0x19
    return out


def costs(O, T, tile_palettes, palette, C, S, p, i):
    """cost(u) in Q16 units of slot (p, i); guided_model.costs' arguments and population rules (p == -1: the tied slot)."""
    h = T.shape[0]
    tp = np.asarray(tile_palettes)[:32 * (h // 8)].reshape(h // 8, 32)
    sub = np.repeat(np.repeat(tp, 8, 0), 8, 1)
    opaque = T[..., 3] > 0
    pal_u = GM.pack_u(np.asarray(palette).reshape(C, S, 3))
    total = np.zeros(NCOL, np.uint64)
    for s in (range(C) if p < 0 else [p]):
        px = T[..., :3][opaque & (sub == s)]
        if px.shape[0] == 0:
            continue
        col, cnt = np.unique(px, axis=0, return_counts=True)
        for c, n in zip(col, cnt):
            qd = q(distances(O, c))
            m = np.uint64(NO_FLOOR)
            for j in range(S):
                if j != i:
                    m = min(m, qd[int(pal_u[s, j])])
            total += np.uint64(n) * np.minimum(qd, m)
    return total


class Model(GM.Model):
    """guided_model.Model whose table is the CIELAB one."""
    table = None  # the ordered-dither table of a context made `by_hand`

    def costs(self, p, i):
        _, tied = self.entries(p, i)
        return costs(self.O, self.T, self.tile_palettes, self.internal, self.C, self.Si, -1 if tied else p, self.S if tied else i)

    def redmean_costs(self, p, i):
        return GM.Model.costs(self, p, i)

    @classmethod
    def by_hand(cls, O, img, C, S, flags, table, tile_palettes, palette):
        """A plain context in a state given by hand, where the reference's k-means start does not exist (a picture of 2 colours)."""
        m = cls.__new__(cls)
        m.O, m.C, m.S, m.Si, m.flags, m.img, m.backdrop = O, C, S, S, dict(flags), img, False
        m.om = OM.Model(O, img, C, S, m.flags, table)
        m.om.set_state(tile_palettes, palette)
        m.T, m.direct, m.min_gap, m.table = m.om.T, table is None, float("inf"), table
        return m


class SetModel(SGM.SetModel):
    """set_guided_model.SetModel whose table is the integer sum of the members' CIELAB tables."""

    def costs(self, p, i, Ts=None):
        _, tied = self.entries(p, i)
        total = np.zeros(NCOL, np.uint64)
        for T, tp in zip(self.imgs if Ts is None else Ts, self.tiles):
            total += costs(self.O, T, tp, self.internal, self.C, self.Si, -1 if tied else p, self.S if tied else i)
        return total

    def redmean_costs(self, p, i):
        return SGM.SetModel.costs(self, p, i)


def image(h, seed, variant=0, two=False):
    return posterise(GM.image(h, seed, variant), two)


def frames(F, H):
    return [posterise(f) for f in SB.frames(F, H)]


# ---- the pictures and slots of the GPU tests' table comparisons (tests/test_guided_lab.py) ---------------------------------------
# name -> (h, image seed, C, S, flags, backdrop, table, hole, tiles of subpalette 0 (None: the k-means start's), slots)
TABLE_CASES = {
    "one-slice": (8, 21, 2, 4, dict(perceptual=True), False, None, False, 27, [(1, 0), (1, 3)]),          # subpalette 1: 5 tiles, 320 pixels
    "ragged": (16, 22, 2, 4, dict(perceptual=True), False, None, False, 37, [(0, 1), (1, 2)]),             # 2,368 and 1,728 pixels: 2 and 1 slices and a ragged one
    "whole-slices": (16, 23, 1, 3, dict(perceptual=True), False, None, False, None, [(0, 0), (0, 2)]),     # 4,096 pixels: four whole slices
    "transparent": (16, 24, 2, 4, dict(perceptual=True), False, None, True, None, [(0, 2), (1, 1)]),
    "backdrop": (16, 26, 2, 4, dict(perceptual=True), True, None, False, None, [(1, 1), (2, 0)]),           # a regular slot and the tied one
    "ordered": (16, 27, 2, 4, dict(perceptual=True), False, (2, 48), False, None, [(1, 0)]),
    "plain-context": (8, 28, 2, 4, {}, False, None, False, None, [(0, 3)]),                              # not perceptual: the proxy is legal all the same
}


def no_floor_case():
    """(C, S) = (2, 1): one-entry subpalettes have no other entry, and the reference's k-means start does not exist there.
    -> (img, tile_palettes[1024], palette[2, 3]): 20 tiles of subpalette 0, 12 of subpalette 1."""
    tp = np.zeros(1024, np.uint8)
    tp[20:32] = 1
    return image(8, 25), tp, np.array([[9, 20, 6], [27, 11, 18]], np.uint8)


def table_model(O, name):
    h, seed, C, S, flags, backdrop, table, hole, first, slots = TABLE_CASES[name]
    img = image(h, seed, two=table is not None)
    if hole:
        img = OM.with_hole(img)
    if table is not None:  # two colours: no k-means start; tiles alternate in pairs, the palette is set by hand
        tp = np.zeros(1024, np.uint8)
        tp[:32 * (h // 8)] = (np.arange(32 * (h // 8)) // 2) % C
        pal = np.array([[5, 6, 18], [8, 8, 14], [20, 21, 12], [24, 22, 9], [4, 7, 20], [9, 5, 16], [22, 23, 10], [21, 19, 13]], np.uint8)[:C * S]
        return Model.by_hand(O, img, C, S, flags, OM.bayer(*table), tp, pal)
    m = Model(O, img, C, S, flags, None, backdrop)
    if first is not None:
        tp = m.tile_palettes
        n = 32 * (h // 8)
        tp[:n] = 1
        tp[:first] = 0
        m.set_tile_palettes(tp)
    return m


# ---- the trajectories (tests/test_guided_lab.py, tests/test_set_guided_lab.py, the CLI test) -------------------------------------
# name -> (h, image seed, C, S, flags, backdrop, K, n: guided calls from the k-means start in slot order, wrapping)
CASES = {
    "perceptual-2x4": (16, 31, 2, 4, dict(perceptual=True), False, 16, 16),       # two sweeps
    "perceptual-1x3": (8, 32, 1, 3, dict(perceptual=True), False, 16, 6),         # two sweeps
    "perceptual-dither-2x4": (16, 33, 2, 4, dict(perceptual=True, dither=True), False, 16, 16),
}
# name -> (F, H, C, S, flags, B0 (None: a plain set), K, calls)
SET_CASES = {
    "perceptual-f2-2x4": (2, 8, 2, 4, dict(perceptual=True), None, 16, 8),
    "perceptual-f3-2x4": (3, 8, 2, 4, dict(perceptual=True), None, 16, 8),
    "backdrop-f2-2x4": (2, 8, 2, 4, dict(perceptual=True), (31, 31, 31), 16, 9),  # one whole sweep, the tied slot last
}


def case_model(O, name):
    h, seed, C, S, flags, backdrop, K, n = CASES[name]
    return Model(O, image(h, seed), C, S, flags, None, backdrop)


def set_case_model(O, name):
    F, H, C, S, flags, B0, K, n = SET_CASES[name]
    return SetModel(O, frames(F, H), C, S, flags, B0)


_trajectories = {}


def trajectory(O, name):
    """The model's guided calls under the CIELAB proxy from the k-means start, computed once and left unchanged.  Every record
    carries `red`, the redmean shortlist of the same state."""
    if name not in _trajectories:
        h, seed, C, S, flags, backdrop, K, n = CASES[name]
        m = case_model(O, name)
        r = dict(img=m.img, C=C, S=S, flags=flags, backdrop=backdrop, K=K, tp=m.tile_palettes, pal0=m.palette, B0=m.B if backdrop else None, map0=m.palette_map, err0=m.error(), recs=[])
        sl = m.slots()
        for j in range(n):
            p, i = sl[j % len(sl)]
            red = GM.shortlist(m.redmean_costs(p, i), m.internal[m.entries(p, i)[0][0]], K)[0]
            rec = m.call(p, i, K)
            rec["red"] = red
            r["recs"].append(rec)
        r["min_gap"] = m.min_gap
        m.close()
        _trajectories[name] = r
    return _trajectories[name]


def set_trajectory(O, name):
    if name not in _trajectories:
        F, H, C, S, flags, B0, K, n = SET_CASES[name]
        m = set_case_model(O, name)
        r = dict(imgs=m.imgs, C=C, S=S, flags=flags, backdrop=m.backdrop, K=K, tiles=m.tiles, pal0=m.palette, B0=m.B, maps0=m.pmaps, err0=m.error(), recs=[])
        sl = m.slots()
        for j in range(n):
            p, i = sl[j % len(sl)]
            red = GM.shortlist(m.redmean_costs(p, i), m.internal[m.entries(p, i)[0][0]], K)[0]
            rec = m.call(p, i, K)
            rec["red"] = red
            r["recs"].append(rec)
        r["min_gap"] = m.min_gap
        m.close()
        _trajectories[name] = r
    return _trajectories[name]


# ---- the headless driver's run (tests/test_guided_lab_cli.py) ---------------------------------------------------------------------
CLI_CASE = dict(h=8, seed=41, C=2, S=4, K=8, extra=2)  # --perceptual-palettes --guided 1 --guided-proxy cielab; `extra` calls behind the guided sweep


def cli_trajectory(O):
    """The CLI's loop in the model: scheduled calls of 64 from the k-means start (seed 1, step_id = the call's number), one
    guided sweep under the CIELAB proxy behind the first sweep of the palette, `extra` calls more.
    -> dict(img, calls, json, sweep: the guided sweep's records, min_gap)."""
    if "cli" not in _trajectories:
        c = CLI_CASE
        m = Model(O, image(c["h"], c["seed"]), c["C"], c["S"], dict(perceptual=True))
        sched = O.schedule(c["C"], c["S"], 400)
        end = next(j for j in range(399) if sched[j + 1][4] != sched[j][4])  # the last call of the first sweep of the palette
        calls, sweep = end + 1 + c["extra"], None
        for j in range(calls):
            method, p, i, ch, _ = sched[j]
            m.om.call(method, [p * c["S"] + i], ch, 1, j, 64 if method == 0 else 0)
            if j == end:
                sweep = m.sweep(c["K"])
        _trajectories["cli"] = dict(img=m.img, calls=calls, json=m.om.as_json(), sweep=sweep, min_gap=min(m.min_gap, m.om.min_gap))
        m.close()
    return _trajectories["cli"]
