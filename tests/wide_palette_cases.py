"""The wide palette geometries of tests/test_wide_palettes.py: subpalettes of more than 16 entries and more than 16
subpalettes, up to the 253 colours snesimage_create admits.  The case table, the images, the oracle's starting states, the
candidate lists and the short oracle trajectories; tests/test_wide_palettes_model.py checks on the CPU what the GPU tests
take for granted about them.  Everything here runs on the CPU and is computed once per process and left unchanged."""
import numpy as np

import adversarial_images as AI
import ordered_model as OM

MIN_GAP = OM.MIN_GAP
SEED = 0x5EED0010  # image seed of a case: SEED + h, as tests/test_gpu_parity.py::test_small_heights

# id -> (sub_count, sub_size, h); the width is 256.  Heights are the smallest that make the case possible.
CASES = {
    "W1": (1, 253, 8),      # k = 253 palette k-means; the entry search spans four 64-entry stretches; the largest k_merge_proxy table
    "W1h16": (1, 253, 16),  # the same with two rows of tiles (the empty-cluster case)
    "W2": (253, 1, 64),     # k = 253 tile k-means over 256 tiles; one-entry subpalettes at the maximum count
    "W3": (126, 2, 32),     # many subpalettes, the smallest size with a stand-in entry
    "W4": (2, 126, 32),     # sub_size between 64 and 128
    "W4h8": (2, 126, 8),    # (the height --perceptual-palettes is run at)
    "W5": (11, 23, 32),     # test_single_entry_subpalette_and_max_palette's geometry at a height the oracle handles quickly
    "W6": (15, 16, 32),     # a plain 16-entry subpalette: the <16> specialisations without a backdrop
    "W7": (14, 17, 32),     # the first size above the specialisations: the generic body
    "W8": (3, 84, 16),      # sub_size above 64 with more than one subpalette; 252 colours
}
TABLE = ("W1", "W1h16", "W2", "W3", "W4", "W5", "W6", "W7", "W8")  # the k-means and scoring tests
PERCEPTUAL_TABLE = ("W1", "W2", "W3", "W4h8", "W5", "W6", "W7", "W8")  # CIEDE2000 on the CPU is slow: W1 and W4 at 8 rows
KINDS = ("synth", "alpha", "few")
FLAGS = {"rgb": {}, "perceptual": dict(perceptual=True), "dither": dict(dither=True), "dither_perceptual": dict(dither=True, perceptual=True)}


def image(case, kind):
    """synth: the gradient-plus-noise picture.  alpha: one with transparent pixels inside its rows — synth_image's variant 1
    clears rows 96..159, which none of these heights has, so adversarial_images.alpha_mix (it needs 24 rows) or, below that,
    ordered_model.with_hole.  few: adversarial_images.two_tone, three colours: most of a wide palette is duplicates."""
    from snesimage_amd.synth import synth_image
    h = CASES[case][2]
    if kind == "synth":
        return synth_image(SEED + h, 256, h, 0)
    if kind == "alpha":
        img = synth_image(SEED + h, 256, h, 1)
        if (img[..., 3] == 0).any():
            return img
        return AI.alpha_mix(h) if h >= 24 else OM.with_hole(synth_image(SEED + h, 256, h, 0))
    assert kind == "few"
    return AI.two_tone(h)


def batch_images(case):
    """Two pictures for an image batch: the case's gradient picture, and the next seed's with transparent pixels (with_hole)."""
    from snesimage_amd.synth import synth_image
    h = CASES[case][2]
    return [image(case, "synth"), OM.with_hole(synth_image(SEED + h + 1, 256, h, 0))]


BATCH_CALLS = (6, 4)  # an image batch runs six calls and then four more: within ten every batch case accepts a call


def ntile(case):
    return 32 * (CASES[case][2] // 8)


def hand_state(case):
    """A state where the k-means initialisers refuse: every subpalette on some tile, random colours."""
    C, S, h = CASES[case]
    rng = np.random.default_rng(1000 * C + S)
    return AI.hand_tiles(C), rng.integers(0, 32, (C * S, 3), dtype=np.uint8)


_starts = {}


def start(O, case, kind, flags_name):
    """The oracle's starting state of (case, image, flags) -> dict(img, tp, pal, pmap, err, init, recalc): the k-means start
    as far as the reference gets (init / recalc: whether initialize_tiles / recalculate_palettes went through; a refused
    recalculate_palettes leaves the state of initialize_tiles), hand_state + optimize() where initialize_tiles refuses."""
    key = (case, kind, flags_name)
    if key not in _starts:
        C, S, h = CASES[case]
        img = image(case, kind)
        o = O.OracleImage(img, C, S, **FLAGS[flags_name])
        init = recalc = False
        try:
            o.initialize_tiles()
            init = True
            o.recalculate_palettes()
            recalc = True
        except RuntimeError:
            pass
        if not init:
            o.tile_palettes, o.palette = hand_state(case)
            o.optimize()
        elif not recalc:
            o.optimize()  # the map of the palette as it stands, whatever the refused call left
        _starts[key] = dict(img=img, tp=o.tile_palettes, pal=o.palette, pmap=o.palette_map, err=o.error(), init=init, recalc=recalc)
        o.close()
    return _starts[key]


def oracle_at(O, case, kind, flags_name):
    """A fresh oracle in the starting state."""
    C, S, h = CASES[case]
    s = start(O, case, kind, flags_name)
    o = O.OracleImage(s["img"], C, S, **FLAGS[flags_name])
    o.tile_palettes, o.palette, o.palette_map = s["tp"], s["pal"], s["pmap"]
    return o


def slots(case):
    """(first subpalette, first entry), (last subpalette, last entry) and, for sizes above 64, both sides of the first
    64-entry boundary."""
    C, S, h = CASES[case]
    out = [(0, 0), (C - 1, S - 1)]
    if S > 64:
        out += [(C - 1, 63), (0, 64)]
    return [s for k, s in enumerate(out) if s not in out[:k]]


def candidate_list(O, pal, case, p, i, n, seed=7):
    """n (8..24) candidates for slot (p, i): the incumbent, a copy of the next entry of the same subpalette (the tie goes to
    the lower index), a copy of the entry 64 places on where the subpalette has one, black and white, one repeated candidate."""
    C, S, h = CASES[case]
    assert 8 <= n <= 24
    cand = O.random_candidates(seed, p * S + i, n)
    cand[0] = pal[p * S + i]
    cand[1] = pal[p * S + (i + 1) % S]
    if S > 64:
        cand[2] = pal[p * S + (i + 64) % S]
    cand[3] = [0, 0, 0]
    cand[4] = [31, 31, 31]
    cand[n - 1] = cand[5]
    return cand


SCORING_N = {"rgb": 18, "perceptual": 10}  # list lengths of the scoring test (CIEDE2000 on the CPU: 10 candidates cost about 3 s at W1)
REMAP_CHUNK = 4                            # the remap alone runs in chunks of 4, which divides neither: the last chunk is partial


# ---- --dither: what the oracle says about a (case, flags), shared by every kernel family that is run on it -----------------
DITHER_CASES = [(c, "dither") for c in ("W6", "W7", "W8", "W4", "W1", "W2", "W3")] + [(c, "dither_perceptual") for c in ("W6", "W7", "W8", "W4h8", "W1")]
# candidate seed of the calls behind the scored lists, chosen on the CPU so that at least one of them accepts: its committed
# map is then the winner's resumed run, compared bit for bit
DITHER_SEED = {("W3", "dither"): 1, ("W1", "dither_perceptual"): 6}  # (9 elsewhere)
DITHER_LAB_SLOT = {"W4h8": 0}  # with CIEDE2000 the one call is on the last slot, or here on the first (0)

_dither = {}


def dither_reference(O, case, flags_name):
    """The oracle on the picture with transparent pixels, from optimize() of the starting state -> dict(pmap, err, pal, lists,
    calls, min_gap).  lists: per slot (p, i, cand, errors, maps) of candidate_list — 12 candidates on every slot of slots(), with
    CIEDE2000 8 on the first and the last slot.  calls: optimizer calls of that many random candidates behind them (two, with
    CIEDE2000 one, on the last slot or the first) -> (p, i, step_id, error, rgb5, changed, palette, map); every comparison of the acceptance
    is measured (min_gap)."""
    key = (case, flags_name)
    if key not in _dither:
        C, S, h = CASES[case]
        lab = "perceptual" in flags_name
        n = 8 if lab else 12
        o = oracle_at(O, case, "alpha", flags_name)
        o.optimize()
        r = dict(n=n, pmap=o.palette_map, err=o.error(), pal=o.palette, lists=[], calls=[], min_gap=float("inf"), seed=DITHER_SEED.get(key, 9))
        sl = slots(case)[:2] if lab else slots(case)
        for p, i in sl:
            cand = candidate_list(O, r["pal"], case, p, i, n)
            eo, mo = o.score_candidates(p, i, cand, want_maps=True)
            r["lists"].append((p, i, cand, eo, mo))
        for k, (p, i) in enumerate(sl[DITHER_LAB_SLOT.get(case, 1):][:1] if lab else sl[:2]):
            before = o.palette[p * S + i].copy()
            best = o.error()
            for e in o.score_candidates(p, i, O.random_candidates(r["seed"], k, n)):
                gap = abs(e - best) / best
                if gap > 0.0:
                    r["min_gap"] = min(r["min_gap"], gap)
                best = min(best, e)
            e, rgb = o.step(0, p, i, 0, r["seed"], k, n)
            assert e == best
            r["calls"].append((p, i, k, e, rgb.copy(), int(not np.array_equal(rgb, before)), o.palette, o.palette_map))
        o.close()
        _dither[key] = r
    return _dither[key]


# ---- the short trajectories of the step / slot-window tests ---------------------------------------------------------------
N_CALLS, N_RANDOM = 12, 16
# case -> (image kind, candidate seed).  Chosen on the CPU (tests/test_wide_palettes_model.py): the oracle accepts and rejects
# calls on each, and no compared pair of errors is closer than MIN_GAP without being equal.
TRAJECTORIES = {"W1": ("synth", 3), "W2": ("synth", 3), "W3": ("synth", 3), "W6": ("synth", 3), "W8": ("alpha", 3)}


def first_call(case):
    """The schedule's steps 0..3 are random sweeps over the C * S slots, step 4 the channel sweep: six calls before it."""
    C, S, h = CASES[case]
    return 4 * C * S - 6


def call_candidates(O, pal, S, method, p, i, ch, seed, step_id):
    if method == 0:
        return O.random_candidates(seed, step_id, N_RANDOM)
    assert method == 1
    cand = np.repeat(pal[p * S + i][None, :], 32, 0)
    cand[:, ch] = np.arange(32)
    return cand


_trajectories = {}


def trajectory(O, case, flags_name, with_gaps=True):
    """N_CALLS scheduled calls of the oracle from the starting state, the first one call number first_call(case) ->
    dict(sched, recs, accepted, min_gap, pal, pmap, json); recs[j] = (error, rgb5, changed).  with_gaps: every candidate of
    every call is scored on its own as well, so that the gap between any two errors the acceptance compares is known (the CPU
    premise; the GPU tests do without it and min_gap is None)."""
    key = (case, flags_name)
    if key not in _trajectories or (with_gaps and _trajectories[key]["min_gap"] is None):
        C, S, h = CASES[case]
        kind, seed = TRAJECTORIES[case]
        o = oracle_at(O, case, kind, flags_name)
        first = first_call(case)
        sched = O.schedule(C, S, first + N_CALLS + 1)
        recs, min_gap, accepted = [], float("inf"), 0
        for j in range(first, first + N_CALLS):
            method, p, i, ch, _ = sched[j]
            before = o.palette[p * S + i].copy()
            cand = call_candidates(O, o.palette, S, method, p, i, ch, seed, j)
            best = o.error()
            for e in (o.score_candidates(p, i, cand) if with_gaps else []):
                gap = abs(e - best) / best
                if gap > 0.0:
                    min_gap = min(min_gap, gap)
                best = min(best, e)
            e, rgb = o.step(method, p, i, ch, seed, j, N_RANDOM if method == 0 else 0)
            assert not with_gaps or e == best, "the oracle's call is not the acceptance rule over its own scores"
            assert np.array_equal(rgb, o.palette[p * S + i])
            changed = int(not np.array_equal(rgb, before))
            accepted += changed
            recs.append((e, rgb.copy(), changed))
        _trajectories[key] = dict(sched=sched, first=first, seed=seed, kind=kind, recs=recs, accepted=accepted, min_gap=min_gap if with_gaps else None, pal=o.palette, pmap=o.palette_map,
                                  json=o.as_json(), methods=[sched[j][0] for j in range(first, first + N_CALLS)])
        o.close()
    return _trajectories[key]


# ---- the feature layer: each feature's own model, once per wide shape -------------------------------------------------------
# Every function below returns what its model says, computed once and left unchanged; the models assert the gap premise
# (check_gap) at every decision they compare, so a reference that exists holds it.

_features = {}


def _cached(fn):
    def wrapper(O, *key):
        k = (fn.__name__,) + key
        if k not in _features:
            _features[k] = fn(O, *key)
        return _features[k]
    wrapper.__name__ = fn.__name__
    return wrapper


def optimized_oracle(O, case, kind, flags_name):
    """The starting state with palette_map = optimize() of the palette: what the feature layer works on."""
    o = oracle_at(O, case, kind, flags_name)
    o.optimize()
    return o


def tile_pairs(case, n=40, must=()):
    """n (tile, subpalette) pairs; `must`: subpalettes the list has to reach.  (A pair on the tile's own subpalette scores the
    incumbent.)"""
    C, S, h = CASES[case]
    rng = np.random.default_rng(40 + C)
    tiles = rng.integers(0, ntile(case), n)
    subs = rng.integers(0, C, n)
    subs[:len(must)] = must
    return [(int(t), int(s)) for t, s in zip(tiles, subs)]


TILE_STEP_TILE = {"W3": 17}  # the tile of the one tile call: chosen on the CPU so that the call moves it


@_cached
def tile_moves(O, case, flags_name, n):
    """score_tile_moves on tile_pairs and one tile call (rgb only), by tests/tile_model.py."""
    import tile_model as TM
    C, S, h = CASES[case]
    o = optimized_oracle(O, case, "synth", flags_name)
    r = dict(tp=o.tile_palettes, pal=o.palette, pmap=o.palette_map, err=o.error(), img=image(case, "synth"))
    r["pairs"] = tile_pairs(case, n, (0, 63, 64, 125) if C > 125 else (0, C - 1))
    r["scored"] = [TM.model_candidate(o, t, s) for t, s in r["pairs"]]
    if flags_name == "rgb" and case in TILE_STEP_TILE:
        r["tile"] = TILE_STEP_TILE[case]
        r["step"] = TM.model_tile_call(o, r["tile"], C, r["err"])
        r.update(tp_after=o.tile_palettes, pmap_after=o.palette_map, err_after=o.error())
    o.close()
    return r


@_cached
def characters(O, case, merges):
    """The character budget (tests/character_model.py) and one refit sweep behind it (tests/refit_model.py) from the optimized
    start of the synth image: the shortlist of 64, the errors and maps of its first 8, `merges` reduction steps with K = 4."""
    import character_model as CM
    import refit_model as RM
    C, S, h = CASES[case]
    img = image(case, "synth")
    o = optimized_oracle(O, case, "synth", "rgb")
    bud = CM.Budget(O, o, img)
    r = dict(img=img, tp=o.tile_palettes, pal=o.palette, pmap=o.palette_map, err=o.error())
    pm, chars, rep, flip, U0, size = bud.state()
    r.update(chars=chars, rep=rep, flip=flip, U0=U0)
    r["ncand"] = len(bud.candidates())
    r["short"] = bud.shortlist(64)
    r["scored"] = [bud.score(t, b, f) for _, t, b, f in r["short"][:8]]
    r["merges"], r["U"] = bud.reduce(U0 - merges, 4)
    r["pmap_reduced"] = o.palette_map
    r["refit"] = RM.Refit(bud).sweep()
    r["pmap_refit"] = o.palette_map
    o.close()
    return r


LEVEL_TILES = (0, 5, 31, 32, 63, 64, 100, 127)


@_cached
def levels(O, case):
    """Per-tile ordered-dither levels (tests/level_model.py): the ladder of 4 Bayer 4 x 4 tables up to amplitude 64, every tile
    on level 3; score_tile_levels on LEVEL_TILES x one other level each, and one level call."""
    import level_model as LM
    C, S, h = CASES[case]
    img = image(case, "synth")
    bank = LM.ladder(4, 64, 4)
    m = LM.Model(O, img, C, S, {}, bank, 3)
    m.kmeans_start()
    r = dict(img=img, bank=bank, start=3, tp=m.tile_palettes, pal=m.palette, T0=m.T, map0=m.palette_map, err0=m.error())
    r["pairs"] = [(t, k % 3) for k, t in enumerate(LEVEL_TILES)]
    r["scored"] = [m.candidate(t, l) for t, l in r["pairs"]]
    r["tile"] = LEVEL_TILES[3]
    r["step"] = m.level_call(r["tile"], r["err0"])
    r.update(levels=m.levels.copy(), map1=m.palette_map, min_gap=m.min_gap)
    m.close()
    return r


@_cached
def guided(O, case, proxy):
    """Guided calls (tests/guided_model.py; proxy "cielab": tests/guided_lab_model.py on a posterised picture in a state given
    by hand, where k-means has too few colours to start from): all 32,768 costs and the shortlist of 8 for the first and the
    last slot, then one guided call on the first."""
    import guided_lab_model as GL
    import guided_model as GM
    C, S, h = CASES[case]
    if proxy == "cielab":
        img = GL.posterise(image(case, "synth"))
        tp, pal = hand_state(case)
        m = GL.Model.by_hand(O, img, C, S, dict(perceptual=True), None, tp, pal)
    else:
        img = image(case, "synth")
        m = GM.Model(O, img, C, S)
    r = dict(img=img, flags=m.flags, tp=m.tile_palettes, pal=m.palette, pmap=m.palette_map, err=m.error(), slots=[(0, 0), (C - 1, S - 1)])
    r["costs"] = [m.costs(p, i) for p, i in r["slots"]]
    r["cands"] = [m.candidates(p, i, 8) for p, i in r["slots"]]
    r["call"] = m.call(0, 0, 8)
    r["min_gap"] = m.min_gap
    m.close()
    return r


SET_FRAMES, SET_K = 2, 8
SET_CALLS = ((5, 0, 64), (6, 1, 0))  # (candidate seed, subpalette, entry) of the set's random calls


@_cached
def shared_set(O, case):
    """A shared-palette set of two frames (tests/set_guided_model.py): the stacked k-means start, E, the joint errors of a
    candidate list, two random calls and one guided call."""
    import set_backdrop_model as SB
    import set_guided_model as SGM
    C, S, h = CASES[case]
    imgs = SB.frames(SET_FRAMES, h)
    m = SGM.SetModel(O, imgs, C, S)
    r = dict(imgs=imgs, tiles=m.tiles, pal=m.palette, pmaps=m.pmaps, err=m.error())
    p, i = C - 1, S - 1
    cand = candidate_list(O, r["pal"], case, p, i, 12)
    r.update(slot=(p, i), cand=cand, errs=m.score(p, i, cand))
    # two random calls of N_RANDOM candidates: strict <, ascending k, on the summed errors.  SET_CALLS were chosen on the CPU so
    # that the first is rejected and the second accepted: the commit of a random call on the set is compared as well.
    r["steps"] = []
    for step_id, (seed, q, j) in enumerate(SET_CALLS):
        rc = O.random_candidates(seed, step_id, N_RANDOM)
        best, best_k = m.error(), -1
        for k, e in enumerate(m.score(q, j, rc)):
            OM.check_gap(e, best)
            if e < best:
                best, best_k = e, k
        if best_k >= 0:
            pal = m.internal
            pal[q * S + j] = rc[best_k]
            m.set_internal(pal)
        r["steps"].append(dict(seed=seed, step_id=step_id, slot=(q, j), error=best, best_k=best_k, rgb5=m.internal[q * S + j].copy(), pal=m.palette, pmaps=m.pmaps))
    r["guided"] = m.call(0, 0, SET_K)
    r["min_gap"] = m.min_gap
    m.close()
    return r
