"""The references of tests/test_level_paths.py: what tests/level_model.py, ordered_model.py, tile_model.py, character_model.py and
refit_model.py say about the OTHER single-image paths on a context with a bank of several tables (include/snesimage_hip.h:
snesimage_set_ordered_dither_bank) — tile moves and reassignment, explicit scoring, the split-phase step, the character budget,
the refit and the tilemap — and about the edges of the level paths' geometry.  Everything here runs on the CPU, on the
unchanged oracle; every reference is computed once per process and left unchanged.  tests/test_level_paths_model.py asserts on
each of them the premises the comparisons rest on (the gap premise at every decision, accepts and rejects, the clamp reached,
the interaction of tile moves and levels, merges and refits accepted, fits against T differing)."""
import numpy as np

import adversarial_images as AI
import backdrop_model as BM
import character_model as CM
import level_model as LM
import ordered_model as OM
import refit_model as RM
import tile_model as TM

REL_ERR, MIN_GAP = LM.REL_ERR, LM.MIN_GAP
_refs = {}


def cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# ---- steps of the model ------------------------------------------------------------------------------------------------------

def snapshot(m):
    """Everything observable of the model's state."""
    return dict(levels=m.levels.copy(), T=m.T, tp=m.tile_palettes, pal=m.palette, map=m.palette_map.copy(), err=m.error())


def tile_sweep(m, first, n):
    """Tile calls on T(level) (tile_model over the slot model's tile oracle; the gap premise is asserted per candidate); the
    level model takes the tile palettes they leave -> [(error, sub, changed)]."""
    sm = m.slot_model()
    log = TM.model_tile_sweep(sm.tile_oracle(), first, n, m.C)
    tp = sm.tile_palettes
    sm.close()
    m.set_state(tp, m.palette)
    return log


def reassign(m):
    """reassign_tiles() against T(level) -> tiles moved."""
    sm = m.slot_model()
    moved = sm.reassign_tiles()
    tp = sm.tile_palettes
    sm.close()
    m.set_state(tp, m.palette)
    return moved


def schedule(O, count, size, backdrop, n):
    """Rows (method, palette, index, channel, step) of a context's schedule; the call number is the row's position."""
    return BM.model_schedule(O, count, size, n) if backdrop else O.schedule(count, size, n)


def slot_calls(O, m, rows, first, seed, n_random):
    """Scheduled calls on regular slots, call numbers first .. : the model takes the palette they leave -> [(error, rgb5, changed)]."""
    sm = m.slot_model()
    out = [sm.call(method, [p * m.S + i], ch, seed, first + j, n_random) for j, (method, p, i, ch, _) in enumerate(rows)]
    pal, gap = sm.palette, sm.min_gap
    sm.close()
    m.min_gap = min(m.min_gap, gap)
    m.set_state(m.tile_palettes, pal)
    return out


def channel_start(rows):
    return next(k for k, c in enumerate(rows) if c[0] == 1)


def mixed_levels(ntile, L, seed):
    lv = np.zeros(1024, np.uint8)
    lv[:ntile] = np.random.default_rng(seed).integers(0, L, ntile)
    return lv


def base(spec, img, bank, start, m, B):
    h, hole, count, size, flags, backdrop, n, amp, L, seed = spec
    return dict(img=img, bank=bank, start=start, B=B, count=count, size=size, flags=flags, backdrop=backdrop, L=L, ntile=m.ntile, msize=m.S,
                tp=m.tile_palettes, pal=m.palette)


# ---- A: values that reach the clamp ------------------------------------------------------------------------------------------

WHOLE = 2  # a wholly transparent tile of clamp_image


def clamp_image():
    """256 x 16 from tests/adversarial_images.py: the Lab extremes (channels at 0 and 255, the neutral ramp's mid greys, near
    black) on the left, the flat colours of pixel_art on the right, alpha of every kind in columns 64..95, tiles 2 and 3 wholly
    and tile 37 half transparent."""
    img = AI.lab_extremes(16)
    img[:, 128:] = AI.pixel_art(16)[:, 128:]
    img[:, 64:96, 3] = AI.alpha_mix(16)[:, 64:96, 3]
    img[0:8, 16:32, 3] = 0
    img[8:16, 40:44, 3] = 0
    rgb, opaque = img[..., :3], img[..., 3] == 255
    assert (rgb[opaque] == 0).any() and (rgb[opaque] == 255).any() and (rgb[opaque] == 128).any()
    assert (img[0:8, 16:24, 3] == 0).all() and 0 < (img[8:16, 40:48, 3] == 0).sum() < 64
    return img


def clamp_bank(n):
    """L = 3: an all-zero table, a table holding -128, 127, 0 and mixed signs, and a third that differs from it in one offset."""
    t1 = OM.bayer(n, 96).copy()
    t1.flat[0], t1.flat[1], t1.flat[2] = -128, 127, 0
    t2 = t1.copy()
    t2.flat[n * n - 1] = -int(t1.flat[n * n - 1]) - 7
    assert (t1 != t2).sum() == 1 and t1.min() == -128 and t1.max() == 127
    return np.stack([np.zeros((n, n), np.int8), t1, t2])


# (n, perceptual) -> (count, size, seed of the mixed levels)
CLAMP = {(2, False): (2, 3, 1), (2, True): (2, 3, 1), (16, False): (4, 7, 1), (16, True): (4, 7, 1)}
CLAMP_START = 1


def unclamped(img, bank, levels):
    """orig + offset per channel without the clamp, (h, 256, 3) int."""
    h = img.shape[0]
    n = bank.shape[1]
    mask = LM.tile_mask(h, levels)
    y, x = np.mgrid[0:h, 0:256]
    d = np.asarray(bank, np.int64)[mask, y % n, x % n]
    return img[..., :3].astype(np.int64) + d[..., None]


def clamp_reference(O, n, perceptual):
    return cached(("clamp", n, perceptual), lambda: _clamp_reference(O, n, perceptual))


def _clamp_reference(O, n, perceptual):
    count, size, seed = CLAMP[(n, perceptual)]
    flags = dict(perceptual=True) if perceptual else {}
    img, bank = clamp_image(), clamp_bank(n)
    m = LM.Model(O, img, count, size, flags, bank, CLAMP_START)
    m.kmeans_start()
    r = base((16, False, count, size, flags, False, n, 0, 3, seed), img, bank, CLAMP_START, m, None)
    r.update(T0=m.T, map0=m.palette_map, err0=m.error())
    mixed = mixed_levels(m.ntile, 3, seed)
    m.set_levels(mixed)
    r.update(mixed=mixed, T_mixed=m.T, map_mixed=m.palette_map, err_mixed=m.error())
    # pairs: every level on two tiles whose sums leave [0, 255] at either end, on the transparent and the half transparent tile
    u = unclamped(img, bank, np.full(1024, 1, np.uint8))
    opaque = img[..., 3] != 0
    low = CM.tiles_of(np.ascontiguousarray(((u < 0).any(axis=2) & opaque).astype(np.int64))).sum(axis=1)
    high = CM.tiles_of(np.ascontiguousarray(((u > 255).any(axis=2) & opaque).astype(np.int64))).sum(axis=1)

    def telling(count):  # the tile with the most clamped pixels among those whose levels give different maps
        for t in np.argsort(-count, kind="stable"):
            if count[t] > 0 and len({m.candidate_map(int(t), l).tobytes() for l in range(3)}) > 1:
                return int(t)
        raise AssertionError("no clamped tile tells the levels apart")
    clamped = [telling(low), telling(high)]
    holes = CM.tiles_of(np.ascontiguousarray((~opaque).astype(np.int64))).sum(axis=1)
    partly = telling(np.where(holes < 64, holes, 0))
    assert holes[WHOLE] == 64 and 0 < holes[partly] < 64
    pairs = [(t, l) for t in clamped + [WHOLE, partly] for l in range(3)]
    scored = {p: ((r["err_mixed"], m.palette_map) if p[1] == mixed[p[0]] else m.candidate(*p)) for p in pairs}
    r.update(pairs=pairs, scored=scored, clamped=clamped, partly=partly)
    # two sweeps, the second from the levels the first left
    r["sweep1"] = m.level_sweep()
    r["state1"] = snapshot(m)
    r["sweep2"] = m.level_sweep()
    r["state2"] = snapshot(m)
    swept = [t for t, (_, _, ch) in enumerate(r["sweep1"]) if ch] + [t for t, (_, _, ch) in enumerate(r["sweep2"]) if ch]
    r.update(swept=swept, unclamped=unclamped(img, bank, m.levels), min_gap=m.min_gap)
    # behind the sweeps: candidates of one slot with their maps (the dense scorer: with `perceptual` its horizontal pass reads the
    # transposed Lab(T)), reassignment, tile moves of swept tiles, one channel call
    sm = m.slot_model()
    cand = O.random_candidates(6, 0, 24)
    cand[5] = m.palette[1]
    errs, maps = sm.candidates([1], cand, want_maps=True)
    sm.close()
    r["dense"] = dict(slot=(0, 1), cand=cand, errs=errs, maps=maps)
    r["moved"] = reassign(m)
    r["state3"] = snapshot(m)
    sm = m.slot_model()
    tp = m.tile_palettes
    moves = [(t, (int(tp[t]) + 1 + j) % count) for j, t in enumerate(swept[:8])]
    r.update(moves=moves, move_scores=[TM.model_candidate(sm.tile_oracle(), t, s) for t, s in moves])
    sm.close()
    rows = schedule(O, count, size, False, 6 * count * size)
    k0 = channel_start(rows)
    r.update(k0=k0, call_state=rows[k0][1:], call=slot_calls(O, m, rows[k0:k0 + 1], k0, 3, 0), state4=snapshot(m))
    m.close()
    return r


# ---- B: geometry edges -------------------------------------------------------------------------------------------------------

# as level_model.CASES: (h, hole, count, size, flags, backdrop, n, amplitude, L, image seed)
GEOMETRY = {
    "L8-n4-h16": (16, False, 2, 3, {}, False, 4, 56, 8, 0),   # seven candidates per call
    "n16-h8-L2": (8, False, 2, 3, {}, False, 16, 64, 2, 0),   # the pattern is taller than the picture
}
FULL = (256, False, 2, 3, {}, False, 16, 64, 2, 30)           # tiles up to 1023
FULL_RANGES = ((0, 8), (1016, 8))


def geometry_reference(O, name):
    return cached(("geometry", name), lambda: _geometry_reference(O, name))


def _geometry_reference(O, name):
    spec = GEOMETRY[name]
    img, bank, start, m, B = LM.setup(O, spec)
    r = base(spec, img, bank, start, m, B)
    r.update(T0=m.T, map0=m.palette_map, err0=m.error())
    rng = np.random.default_rng(21)
    pairs = [(int(rng.integers(m.ntile)), int(rng.integers(spec[8]))) for _ in range(19)] + [(m.ntile - 1, start)]
    r.update(pairs=pairs, scored={p: ((r["err0"], m.palette_map) if p[1] == start else m.candidate(*p)) for p in set(pairs)})
    r["sweep"] = m.level_sweep()
    r.update(state=snapshot(m), min_gap=m.min_gap)
    m.close()
    return r


def full_reference(O):
    return cached("full", lambda: _full_reference(O))


def _full_reference(O):
    img, bank, start, m, B = LM.setup(O, FULL)
    r = base(FULL, img, bank, start, m, B)
    r.update(T0=m.T, map0=m.palette_map, err0=m.error())
    r["sweeps"] = [m.level_sweep(first, n) for first, n in FULL_RANGES]
    r.update(state=snapshot(m), min_gap=m.min_gap)
    sm = m.slot_model()
    tp = m.tile_palettes
    moves = [(t, 1 - int(tp[t])) for t in range(1016, 1024)]
    r.update(moves=moves, move_scores=[TM.model_candidate(sm.tile_oracle(), t, s) for t, s in moves])
    sm.close()
    m.close()
    return r


# ---- C: the other paths on a context with L > 1 --------------------------------------------------------------------------------

PATHS = {
    "hole-4x7-L4": (24, True, 4, 7, {}, False, 8, 64, 4, 1),
    "hole-backdrop-2x3-L2-perceptual": (24, True, 2, 3, dict(perceptual=True), True, 4, 64, 2, 14),
}
PATH_SEED = {"hole-4x7-L4": 1, "hole-backdrop-2x3-L2-perceptual": 1}      # candidate seed of the optimizer calls
BUDGET = {"hole-4x7-L4": (8, 4), "hole-backdrop-2x3-L2-perceptual": (8, 4)}  # (merges, K) of the last stages
STAGES = ("pre", "tiles1", "levels1", "tiles2", "levels2", "post")


def path_start(O, name):
    spec = PATHS[name]
    img, bank, start, m, B = LM.setup(O, spec)
    return spec, m, base(spec, img, bank, start, m, B)


def flow_reference(O, name):
    return cached(("flow", name), lambda: _flow_reference(O, name))


def _flow_reference(O, name):
    """Two scheduled calls, a full tile sweep, a full level sweep, a tile sweep over the first 32 tiles, a level sweep, three
    channel calls on one slot: the log of every stage and the state behind each."""
    spec, m, r = path_start(O, name)
    count, size, backdrop = spec[2], spec[3], spec[5]
    rows = schedule(O, count, size, backdrop, 6 * (count * size + 1))
    k0 = channel_start(rows)
    seed = PATH_SEED[name]
    logs, states = {}, {}

    def stage(key, log):
        logs[key], states[key] = log, snapshot(m)

    stage("pre", slot_calls(O, m, rows[:2], 0, seed, 0))
    stage("tiles1", tile_sweep(m, 0, m.ntile))
    stage("levels1", m.level_sweep())
    stage("tiles2", tile_sweep(m, 0, 32))
    stage("levels2", m.level_sweep())
    stage("post", slot_calls(O, m, rows[k0:k0 + 3], k0, seed, 0))
    r.update(k0=k0, post_state=rows[k0][1:], logs=logs, states=states, min_gap=m.min_gap)
    m.close()
    return r


def reassign_reference(O, name):
    return cached(("reassign", name), lambda: _reassign_reference(O, name))


def _reassign_reference(O, name):
    spec, m, r = path_start(O, name)
    mixed = mixed_levels(m.ntile, spec[8], 12)
    m.set_levels(mixed)
    r.update(mixed=mixed, moved1=reassign(m), state1=snapshot(m))
    r.update(sweep1=m.level_sweep(), state2=snapshot(m))
    r.update(moved2=reassign(m), state3=snapshot(m))
    r.update(sweep2=m.level_sweep(), state4=snapshot(m), min_gap=m.min_gap)
    m.close()
    return r


def candidate_list(O, current, seed):
    """70 candidates (more than a chunk of 64) with the incumbent's colour (32) and duplicates (40 == 7, 69 == 3, 66 == 65)."""
    cand = O.random_candidates(seed, 0, 70)
    cand[32] = current
    cand[40], cand[69], cand[66] = cand[7], cand[3], cand[65]
    return cand


def scoring_reference(O, name):
    return cached(("scoring", name), lambda: _scoring_reference(O, name))


def _scoring_reference(O, name):
    spec, m, r = path_start(O, name)
    count, size, backdrop = spec[2], spec[3], spec[5]
    mixed = mixed_levels(m.ntile, spec[8], 13)
    m.set_levels(mixed)
    r.update(mixed=mixed, state0=snapshot(m))
    sm = m.slot_model()
    p, i = count - 1, size - 1
    cand = candidate_list(O, m.palette[p * m.S + i], 5)
    r.update(slot=(p, i), cand=cand, errs=sm.candidates([p * m.S + i], cand))
    if backdrop:
        tied = [q * m.S + size for q in range(count)]
        cand_b = candidate_list(O, r["B"], 8)
        r.update(cand_b=cand_b, errs_b=sm.candidates(tied, cand_b))
    sm.close()
    # a channel call in two phases and a random call through step_async, then a level sweep straight behind them
    rows = schedule(O, count, size, backdrop, 6 * (count * size + 1))
    k0 = channel_start(rows) + 3  # slot (0, 1), channel 0
    assert rows[k0][:4] == (1, 0, 1, 0)
    r.update(k0=k0, split=slot_calls(O, m, rows[k0:k0 + 1], k0, 4, 0)[0], state1=snapshot(m))
    r.update(step=slot_calls(O, m, [(0, 1, 0, 0, 0)], 7, 4, 0)[0], state2=snapshot(m))
    r.update(sweep=m.level_sweep(), state3=snapshot(m), min_gap=m.min_gap)
    m.close()
    return r


def budget_of(O, m, r):
    """character_model.Budget on the level model's composed map: the oracle over the original holds it."""
    m.oO.palette_map = m.palette_map
    return CM.Budget(O, m.oO, r["img"], r["size"] if r["backdrop"] else None)


def last_reference(O, name):
    return cached(("last", name), lambda: _last_reference(O, name))


def _last_reference(O, name):
    """The last stages as the CLI orders them: a level sweep, the character budget, two refit sweeps, the tilemap."""
    spec, m, r = path_start(O, name)
    merges, K = BUDGET[name]
    r.update(sweep=m.level_sweep(), state=snapshot(m), min_gap=m.min_gap, K=K)
    bud = budget_of(O, m, r)
    o = m.oO
    pm, chars, rep, flip, U, _ = bud.state()
    r.update(chars=chars, rep=rep, flip=flip, U0=U, shortlist=bud.shortlist(K))
    r["short_scores"] = [bud.score(t, b, f) for _, t, b, f in r["shortlist"]]
    # what the proxy and the fit would give if they read T instead of the original
    wrong = CM.Budget(O, o, r["state"]["T"], r["size"] if r["backdrop"] else None)
    r["shortlist_T"] = wrong.shortlist(K)
    r.update(max_unique=U - merges)
    r["merges"], r["U1"] = bud.reduce(U - merges, K)
    r.update(map1=o.palette_map, err1=o.error())
    rf = RM.Refit(bud)
    r["fits"] = [c["fitted"].tolist() for c in rf.snapshot()]
    r["fits_T"] = [c["fitted"].tolist() for c in rf.snapshot(orig=CM.tiles_of_rgb(r["state"]["T"]))]
    r["refits"] = []
    for _ in range(2):
        recs, accepted, U = rf.sweep()
        r["refits"].append(dict(recs=recs, accepted=accepted, U=U, map=o.palette_map, err=o.error()))
    r["tilemap"] = CM.tilemap_json(CM.characters(o.palette_map, r["img"], r["size"] if r["backdrop"] else None), m.tile_palettes)
    m.close()
    return r
