"""The refit of shared characters (snesimage_character_fits, snesimage_score_refits, snesimage_refit_characters,
--refit-tiles): after a character reduction every shared character is refitted to all the tiles that use it, each read through
its own subpalette and flip, and error() decides whether the refit stays.  The model is tests/refit_model.py over the
unchanged CPU oracle: everything integer is compared exactly, errors within 1e-11 relative, product against product bit for
bit.  Every decision the model compares carries check_gap (1e-9)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_model as B
import character_model as M
import ordered_model as OM
import refit_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REFIT_FUNCS = ["snesimage_character_fits", "snesimage_score_refits", "snesimage_refit_characters"]
ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


# ---- the model's own checks (no device, no product) -------------------------------------------------------------------------

def hand_class():
    """Two tiles in different subpalettes, the second under flip 3.  Subpalette 0 = (black, mid grey, white), subpalette 1 =
    (red, black, black): entry 2 of subpalette 1 repeats entry 1 (a tie)."""
    pal8 = np.array([[[0, 0, 0], [128, 128, 128], [255, 255, 255]], [[255, 0, 0], [0, 0, 0], [0, 0, 0]]], np.int64)
    orig = np.zeros((2, 64, 3), np.int64)
    orig[0, :32] = [250, 250, 250]            # tile 0: upper half nearly white, lower half nearly black
    orig[0, 32:] = [5, 5, 5]
    orig[1, :] = [1, 1, 1]                    # tile 1 (drawn under flip 3): nearly black everywhere ...
    orig[1, 63] = [255, 10, 10]               # ... except its last pixel, which shows position 0 of the representative
    return orig, pal8, np.array([0, 1]), np.array([0, 1]), np.array([0, 3])


def test_fit_on_a_hand_made_class_with_a_flip_and_two_subpalettes():
    orig, pal8, tp, members, flips = hand_class()
    fitted, gain, cost = R.fit_class(orig, pal8, tp, members, flips, np.zeros(64, np.int64))
    # by hand, per value v: tile 0 reads subpalette 0's entry v, tile 1 reads subpalette 1's entry v.
    #  position 0: tile 0 nearly white, tile 1's pixel 63 nearly red -> v = 0 (black + red): tile 0 pays white-black, tile 1
    #   almost nothing; v = 2 (white + black): tile 0 almost nothing, tile 1 pays red-black: the cheaper of the two is computed
    k = M.red_mean_keys
    c0 = [int(k([250, 250, 250], pal8[0][v]) + k([255, 10, 10], pal8[1][v])) for v in range(3)]
    assert cost[0].tolist() == c0 and fitted[0] == int(np.argmin(c0))
    #  positions 1..31: tile 0 nearly white, tile 1 (pixel 63 - q) nearly black -> v = 2: white for tile 0, black for tile 1
    assert fitted[1:32].tolist() == [2] * 31
    #  positions 32..63: both nearly black -> subpalette 0 wants v = 0 (black), subpalette 1 wants v = 1 or 2 (black): v = 1
    #  costs tile 0 grey-against-black, v = 0 costs tile 1 red-against-black: by hand
    c40 = [int(k([5, 5, 5], pal8[0][v]) + k([1, 1, 1], pal8[1][v])) for v in range(3)]
    assert cost[40].tolist() == c40 and fitted[32:].tolist() == [int(np.argmin(c40))] * 32
    assert fitted[40] == 1  # 128-grey against 5 is far cheaper than 255-red against 1
    # the flip: member 1's pixel q ^ 63 shows position q, so its odd pixel lands on position 0 and nowhere else
    assert cost[63].tolist() == c40 and cost[0].tolist() != c40
    assert R.spread(fitted, 3)[63] == fitted[0] and R.spread(fitted, 3)[0] == fitted[63]
    assert gain == int((cost[R.Q, 0] - cost.min(axis=1)).sum()) and gain > 0


def test_fit_takes_the_lowest_value_of_a_tie_and_lets_the_backdrop_win():
    orig, pal8, tp, members, flips = hand_class()
    # two nearly black tiles in subpalette 1, whose entries 1 and 2 are both black: the lower index, from whatever the map holds
    dark = np.ones((2, 64, 3), np.int64)
    fitted, gain, cost = R.fit_class(dark, pal8, np.array([1, 1]), members, flips, np.full(64, 2, np.int64))
    assert (cost[:, 1] == cost[:, 2]).all() and (cost[:, 1] < cost[:, 0]).all() and fitted.tolist() == [1] * 64
    assert gain == 0  # the fit differs from the character and gains nothing: such a call is scored and never taken
    # a backdrop context: entry S - 1 of every subpalette is B.  With B = the pixels' own colour the backdrop value wins
    S = 4
    pb = np.zeros((2, S, 3), np.int64)
    pb[:, :3] = pal8
    pb[:, S - 1] = [60, 200, 90]
    o2 = orig.copy()
    o2[0, 7] = o2[1, 63 - 7] = [60, 200, 90]  # position 7 in both members (member 1 under flip 3)
    fitted, gain, cost = R.fit_class(o2, pb, tp, members, flips, np.zeros(64, np.int64))
    assert fitted[7] == S - 1 and cost[7, S - 1] == 0 and (fitted[8:32] != S - 1).all()


def test_gain_is_never_negative_and_the_fit_ignores_the_map():
    rng = np.random.default_rng(11)
    orig = rng.integers(0, 256, (6, 64, 3))
    pal8 = rng.integers(0, 256, (3, 5, 3))
    tp = rng.integers(0, 3, 6)
    members, flips = np.array([1, 2, 4, 5]), np.array([0, 1, 2, 3])
    fits = []
    for _ in range(8):
        cur = rng.integers(0, 5, 64)  # whatever the map holds: the fit is the same, the gain is measured from it
        fitted, gain, cost = R.fit_class(orig, pal8, tp, members, flips, cur)
        assert gain >= 0 and gain == int((cost[R.Q, cur] - cost[R.Q, fitted]).sum())
        fits.append(fitted.tolist())
    assert all(f == fits[0] for f in fits)
    fitted, gain, _ = R.fit_class(orig, pal8, tp, members, flips, np.array(fits[0]))
    assert gain == 0  # the fit of a fitted class changes nothing
    other, _, _ = R.fit_class(orig, pal8, tp, members[:3], flips[:3], np.array(fits[0]))
    assert other.tolist() != fits[0]  # membership is what it depends on


# ---- on the MI355X -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def state_of(g):
    return g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.palette.tobytes(), g.error()


# name: sub_count, sub_size, backdrop, h, flags, seed, (budget | -merges), K, ordered table (n, amplitude) or None
CASES = {
    "a": (4, 7, True, 40, {}, 0, 120, 4, None),
    "b": (4, 7, False, 32, {"perceptual": True}, 4, 100, 4, None),
    "c": (2, 3, False, 32, {}, 3, 60, 16, None),
    "d": (1, 40, False, 16, {"dither": True}, 0, 40, 4, None),
    "pb": (4, 7, True, 40, {"perceptual": True}, 0, -12, 4, None),
    "ord": (2, 3, False, 32, {}, 3, -24, 8, (4, 64)),
}
_REDUCED = {}  # name -> the model's map after the reduction (computed once, never changed)


def case_image(name):
    return B.image(CASES[name][3], CASES[name][5])


def model_start(O, name):
    """The model's oracle (the expanded one for a backdrop) in the start state of the case, and its Budget."""
    count, size, backdrop, h, flags, seed, _, _, table = CASES[name]
    img = case_image(name)
    if table:
        m = OM.Model(O, img, count, size, flags, OM.bayer(*table))
        m.kmeans_start()
        m._sync()  # the oracle over the original, holding the map chosen against the target
        o = m.oO
    elif backdrop:
        o = B.Model(O, img, count, size, flags).o
    else:
        o = O.OracleImage(img, count, size, **flags)
        o.initialize_tiles()
        o.recalculate_palettes()
    return img, o, M.Budget(O, o, img, size if backdrop else None)


def model_reduced(O, name):
    """... after the case's reduction (guarded), replayed from the cached map."""
    img, o, bud = model_start(O, name)
    if name not in _REDUCED:
        start = o.palette_map
        U0 = bud.state()[4]
        budget = CASES[name][6]
        recs, U = bud.reduce(budget if budget > 0 else U0 + budget, CASES[name][7])
        assert U == (budget if budget > 0 else U0 + budget) and len(recs) == U0 - U
        _REDUCED[name] = (start, o.palette_map)
    start, reduced = _REDUCED[name]
    assert np.array_equal(o.palette_map, start) or np.array_equal(o.palette_map, reduced)
    o.palette_map = reduced
    return img, o, bud


def product_start(S, name):
    count, size, backdrop, h, flags, seed, _, _, table = CASES[name]
    g = S.OptimizedImage(case_image(name), count, size, backdrop=backdrop, **flags)
    g.initialize_tiles()
    g.recalculate_palettes()
    if table:
        g.set_ordered_dither(S.bayer_offsets(*table))
        g.optimize()
    return g


def reduced_pair(S, O, name):
    """The product and the model in the state behind the model's reduction (palette_map set on both)."""
    img, o, bud = model_reduced(O, name)
    g = product_start(S, name)
    assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, _REDUCED[name][0])
    g.palette_map = o.palette_map
    return g, o, bud, img


def check_records(recs, want):
    assert len(recs) == len(want)
    for j, (r, w) in enumerate(zip(recs, want)):
        got = tuple(int(r[k]) for k in ("rep", "members", "gain", "changed", "scored"))
        assert got == (w["rep"], w["members"], w["gain"], w["changed"], w["scored"]), (j, got, w)
        assert abs(float(r["error"]) - w["error"]) <= M.REL_ERR * w["error"], (j, float(r["error"]), w["error"])


@pytest.mark.gpu
def test_refit_symbols_exported_declared_and_bound():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in REFIT_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    assert "snesimage_refit_result" in text
    assert C.sizeof(_ffi.RefitResult) == 24
    import snesimage_amd as S
    assert S.api.REFIT_LOG_DTYPE.itemsize == 24
    n = C.c_uint32(0)
    assert lib.snesimage_character_fits(None, None, None, None, None, C.byref(n)) == ERR_ARG and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_score_refits(None, None, 0, None, None) == ERR_ARG
    assert lib.snesimage_refit_characters(None, 0, None, 0, None, None, None, None) == ERR_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c", "a", "d", "ord"], ids=["2x3_h32", "4x7_backdrop_h40", "1x40_h16", "2x3_ordered"])
def test_character_fits_are_the_models(S, O, name):
    """Behind a model reduction replayed on the product: reps, members, gains and fits exact; the state unchanged.  With an
    ordered-dither table the fits still read the original: fitting against the target would give other values."""
    g, o, bud, img = reduced_pair(S, O, name)
    snap = R.Refit(bud).snapshot()
    assert len(snap) >= 5 and any(not np.array_equal(c["fitted"], c["cur"]) for c in snap)
    before = state_of(g)
    reps, members, gains, fits = g.character_fits()
    assert reps.tolist() == [c["rep"] for c in snap]
    assert members.tolist() == [len(c["members"]) for c in snap]
    assert gains.tolist() == [c["gain"] for c in snap]
    assert np.array_equal(fits, np.array([c["fitted"] for c in snap], np.uint8))
    assert all(x >= 0 for x in gains.tolist()) and max(members.tolist()) >= 2
    if CASES[name][8]:
        target = g.target_rgba()
        assert np.array_equal(target, OM.target_image(img, OM.bayer(*CASES[name][8]))) and not np.array_equal(target, img)
        other = R.Refit(bud).snapshot(orig=M.tiles_of_rgb(target))  # what a fit against the dither target would be
        assert [c["fitted"].tolist() for c in other] != [c["fitted"].tolist() for c in snap]
    assert state_of(g) == before
    g.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,poison", [("c", False), ("pb", False), ("d", True), ("ord", False)], ids=["rgb", "perceptual_backdrop", "dither_poisoned", "ordered"])
def test_score_refits_matches_the_oracle(S, O, name, poison):
    """Every eligible class, with repeats, against the oracle with the candidate's map set by hand; one class has been refitted
    by hand beforehand, so its fit equals its character: the incumbent bit for bit.  The state is as if the call had not been
    made, and the next two steps go as on a twin context that never made it."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    L.snesimage_debug_poison_alloc(1 if poison else 0)
    try:
        g, o, bud, img = reduced_pair(S, O, name)
        rf = R.Refit(bud)
        first = next(c for c in rf.snapshot() if not np.array_equal(c["fitted"], c["cur"]))
        stored = rf.candidate_map(first)  # a stored map that is no optimize() of anything, with one class already fitted
        g.palette_map = o.palette_map = stored
        snap = rf.snapshot()
        same = [c["rep"] for c in snap if np.array_equal(c["fitted"], c["cur"])]
        assert same and len(same) < len(snap)  # (the class refitted by hand may have become another class's equal)
        inc = g.error()
        assert abs(inc - o.error()) <= M.REL_ERR * inc
        before = state_of(g)
        order = list(range(len(snap))) + [0, len(snap) - 1, 0]
        want = [rf.score(c) for c in snap]
        errs, maps = g.score_refits([snap[i]["rep"] for i in order], want_maps=True)
        for j, i in enumerate(order):
            e, m = want[i]
            assert np.array_equal(maps[j], m), (j, snap[i]["rep"])
            assert abs(errs[j] - e) <= M.REL_ERR * abs(e), (j, snap[i]["rep"], errs[j], e)
            if snap[i]["rep"] in same:
                assert errs[j] == inc and np.array_equal(maps[j], stored)
        assert errs[-1] == errs[0] and errs[-3] == errs[0] and errs[-2] == errs[len(snap) - 1]
        assert len(set(errs.tolist())) > 2
        assert state_of(g) == before
        assert np.array_equal(g.score_refits([snap[i]["rep"] for i in order[:3]]), errs[:3])
        twin = product_start(S, name)
        twin.palette_map = stored
        assert state_of(twin) == before
        for j, index in enumerate((1, 2)):
            e_g, b_g = g.step(S.METHOD_RANDOM, 0, index, 0, 3, j, 16)
            e_t, b_t = twin.step(S.METHOD_RANDOM, 0, index, 0, 3, j, 16)
            assert e_g == e_t and np.array_equal(b_g, b_t)
        assert state_of(g) == state_of(twin)
        twin.close()
        g.close()
        o.close()
    finally:
        L.snesimage_debug_poison_alloc(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "d"], ids=["backdrop_h40", "perceptual_h32", "rgb_h32", "dither_h16"])
def test_refit_sweep_follows_the_models_trajectory(S, O, name):
    """Sweeps until one accepts nothing: records, final map, U, tile_palettes and palette exact, errors within 1e-11.  The
    inputs were chosen so that calls are accepted (all), rejected (a, b, c) and skipped (c); every gap is 0 or > 1e-9."""
    g, o, bud, img = reduced_pair(S, O, name)
    rf = R.Refit(bud)
    tp, pal = g.tile_palettes.tobytes(), g.palette.tobytes()
    U_before = bud.state()[4]
    assert g.characters()[0] == U_before
    for sweep in range(4):
        e_before = o.error()
        want, accepted, U = rf.sweep()
        rejected = sum(w["scored"] and not w["changed"] for w in want)
        skipped = sum(not w["scored"] for w in want)
        if sweep == 0:  # the conditions on the inputs, from the model itself
            assert accepted >= 1 and o.error() < e_before and U <= U_before
            assert rejected >= 1 or name == "d"
            assert skipped >= 1 or name != "c"
        before = state_of(g)
        recs, acc, unique = g.refit_characters()
        check_records(recs, want)
        assert (acc, unique) == (accepted, U) and U <= U_before
        assert np.array_equal(g.palette_map, o.palette_map)
        assert g.tile_palettes.tobytes() == tp and g.palette.tobytes() == pal and np.array_equal(g.tile_palettes, o.tile_palettes)
        assert g.error() == float(recs[-1]["error"]) and g.characters()[0] == U
        assert abs(g.error() - o.error()) <= M.REL_ERR * o.error()
        if accepted == 0:  # one more sweep accepts nothing and leaves the state bit for bit
            assert state_of(g) == before and sweep >= 1
            break
    else:
        raise AssertionError("the sweeps do not come to rest")
    if name == "a":
        assert sweep == 2  # two sweeps accept, the third does not
    if not CASES[name][2]:
        assert np.array_equal(g.palette, o.palette)
    assert np.array_equal(g.as_rgba(), o.as_rgba())
    g.close()
    o.close()


@pytest.mark.gpu
def test_refit_windows_are_bit_identical(S, O):
    """Configuration a with window = 1, 0 and 4 on three contexts, two sweeps each: records, maps and incumbents bit for bit."""
    ctxs = []
    for window in (1, 0, 4):
        g, o, bud, img = reduced_pair(S, O, "a")
        o.close()
        ctxs.append((window, g))
    ref = None
    for sweep in range(2):
        got = []
        for window, g in ctxs:
            recs, acc, unique, stats = g.refit_characters(window, want_stats=True)
            scored = int(recs["scored"].sum())
            assert stats["useful"] <= stats["scored"] and stats["useful"] == scored and stats["calls"] == len(recs) and stats["accepted"] == acc
            if window == 1:
                assert stats["windows"] == scored == stats["scored"]
            got.append((recs.tobytes(), acc, unique, g.palette_map.tobytes(), g.error()))
        assert got[0] == got[1] == got[2]
        assert got[0][1] >= 1
    for _, g in ctxs:
        g.close()


def planted(S, img, count, size, backdrop, vals, tp=None):
    g = S.OptimizedImage(img, count, size, backdrop=backdrop)
    g.initialize_tiles()
    g.recalculate_palettes()
    if tp is not None:
        g.tile_palettes = tp
    g.palette_map = M.untile(vals, img.shape[0])
    return g


@pytest.mark.gpu
def test_refit_with_nothing_to_do_and_pinned_tiles(S):
    # (a) straight from k-means, no character shared: 0 calls, the state identical
    g = S.OptimizedImage(B.image(16, 0), 1, 40)
    g.initialize_tiles()
    g.recalculate_palettes()
    assert g.characters()[0] == 64
    before = state_of(g)
    recs, acc, unique = g.refit_characters()
    assert len(recs) == 0 and acc == 0 and unique == 64 and len(g.character_fits()[0]) == 0
    assert state_of(g) == before
    g.close()
    # (b) alpha_mix: the fully transparent tiles are one class, but pinned; a pinned tile is in no eligible class
    from adversarial_images import alpha_mix
    img = alpha_mix(32)
    g = S.OptimizedImage(img, 4, 7)
    g.initialize_tiles()
    g.recalculate_palettes()
    pinned = M.pinned_tiles(img)
    U, rep, _, _ = g.characters()
    assert np.bincount(rep).max() >= 2
    before = state_of(g)
    reps = g.character_fits()[0]
    assert not pinned[reps].any() and not pinned[np.isin(rep, reps)].any()
    recs, acc, unique = g.refit_characters()
    assert M.tiles_of(g.palette_map)[pinned].tobytes() == M.tiles_of(np.frombuffer(before[1], np.uint8).reshape(32, 256))[pinned].tobytes()
    if len(reps) == 0:
        assert len(recs) == 0 and state_of(g) == before
    g.close()
    # (c) the hand-made pair of the planted-map test: tile 2 has a transparent pixel, tile 7 shows the backdrop there, tile 9 is
    # tile 7 flipped: one class, not eligible.  Tiles 20, 21 and 22 share a character under flips: eligible
    h, count, size = 16, 4, 7
    img = B.image(h, 2).copy()
    img[0, 16, 3] = 0
    rng = np.random.default_rng(6)
    vals = rng.integers(0, size + 1, (64, 64)).astype(np.uint8)
    vals[2] = vals[7]
    vals[2, 0], vals[7, 0] = 4, size
    vals[9] = M.flip_char(vals[7], 1)
    vals[21], vals[22] = M.flip_char(vals[20], 1), M.flip_char(vals[20], 2)
    g = planted(S, img, count, size, True, vals)
    U, rep, flip, _ = g.characters()
    assert rep[7] == 2 and rep[9] == 2 and rep[21] == 20 and rep[22] == 20
    reps, members, gains, fits = g.character_fits()
    assert reps.tolist() == [20] and members.tolist() == [3] and gains[0] > 0
    e0 = g.error()
    recs, acc, unique = g.refit_characters()
    assert len(recs) == 1 and int(recs[0]["rep"]) == 20 and int(recs[0]["scored"]) == 1 and unique <= U
    after = M.tiles_of(g.palette_map)
    keep = np.ones(64, bool)
    keep[[20, 21, 22]] = False
    assert np.array_equal(after[keep], vals[keep])
    if acc:
        assert g.error() < e0 and np.array_equal(after[20], fits[0]) and np.array_equal(after[21], M.flip_char(fits[0], 1)) and np.array_equal(after[22], M.flip_char(fits[0], 2))
    else:
        assert g.error() == e0 and np.array_equal(after, vals)
    with pytest.raises(S.SnesImageError) as ei:
        g.score_refits([2])  # the representative of a class with a pinned tile
    assert ei.value.code == ERR_ARG
    g.close()
    # (d) a fully pinned image: 0 calls
    holes = B.image(16, 3).copy()
    holes[::8, ::8, 3] = 0
    p = S.OptimizedImage(holes, 2, 3)
    p.initialize_tiles()
    p.recalculate_palettes()
    before = state_of(p)
    recs, acc, unique = p.refit_characters()
    assert len(recs) == 0 and acc == 0 and unique == p.characters()[0] and state_of(p) == before
    p.close()


def shared_vals(img, count, size, seed):
    """A map with planted shared characters (tiles 10..13 = tile 3 under every flip, tiles 41 and 42 = tile 40)."""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, size, (img.shape[0] // 8 * 32, 64)).astype(np.uint8)
    for f in range(4):
        vals[10 + f] = M.flip_char(vals[3], f)
    vals[41] = vals[42] = vals[40]
    return vals


def refused(S, call, code):
    with pytest.raises(S.SnesImageError) as e:
        call()
    assert e.value.code == code, str(e.value)


def refit_calls(x):
    return (lambda: x.character_fits(), lambda: x.score_refits([3]), lambda: x.refit_characters())


@pytest.mark.gpu
def test_refit_refusals(S):
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    h, count, size = 16, 2, 3
    img = B.image(h, 6)
    vals = shared_vals(img, count, size, 12)
    g = planted(S, img, count, size, False, vals)
    assert g.character_fits()[0].tolist() == [3, 40]
    # SNES_ERR_ARG: a rep beyond the image, a tile that is no representative, the representative of a class of one
    for call in (lambda: g.score_refits([64]), lambda: g.score_refits([3, 1000]), lambda: g.score_refits([10]), lambda: g.score_refits([5]), lambda: g.score_refits([3, 41])):
        refused(S, call, ERR_ARG)
    assert len(g.score_refits([])) == 0
    # SNES_ERR_STATE: between the phases of a split-phase step and of a split-phase window ...
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    for call in refit_calls(g):
        refused(S, call, ERR_STATE)
    g.step_commit(buf.ptr)
    taken, _ = g.slots_begin(4, 1, 1, (0, 1, 0, 0))
    for call in refit_calls(g):
        refused(S, call, ERR_STATE)
    g.slots_commit(0, taken)
    # ... and on a context lent to a batch, a set or a group
    a, b = S.OptimizedImage(img, count, size), S.OptimizedImage(img, count, size)
    for create, destroy in ((L.snesimage_batch_create, L.snesimage_batch_destroy), (L.snesimage_shared_create, L.snesimage_shared_destroy)):
        arr = (C.c_void_p * 2)(a._c, b._c)
        hnd = C.c_void_p()
        assert create(arr, 2, C.byref(hnd)) == 0, L.snesimage_last_error()
        for call in refit_calls(a) + refit_calls(b):
            refused(S, call, ERR_STATE)
        destroy(hnd)
    arr1 = (C.c_void_p * 1)(a._c)
    hnd = C.c_void_p()
    assert L.snesimage_group_create(arr1, 1, C.byref(hnd)) == 0, L.snesimage_last_error()
    for call in refit_calls(a):
        refused(S, call, ERR_STATE)
    L.snesimage_group_destroy(hnd)
    for x in (a, b, g):
        x.close()


@pytest.mark.gpu
def test_failed_refit_workspace_allocation_leaves_the_context_usable(S):
    """snesimage_debug_fail_alloc(0): SNES_ERR_HIP, the state unchanged, and the next call goes as on a context that never failed."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    h, count, size = 16, 2, 3
    img = B.image(h, 6)
    vals = shared_vals(img, count, size, 12)
    f, ref = planted(S, img, count, size, False, vals), planted(S, img, count, size, False, vals)
    before = state_of(f)
    assert before == state_of(ref)
    L.snesimage_debug_fail_alloc(0)
    try:
        refused(S, lambda: f.refit_characters(), ERR_HIP)
    finally:
        L.snesimage_debug_fail_alloc(-1)
    assert state_of(f) == before
    recs, acc, unique = f.refit_characters()
    want, acc_r, unique_r = ref.refit_characters()
    assert recs.tobytes() == want.tobytes() and (acc, unique) == (acc_r, unique_r) and state_of(f) == state_of(ref) and len(recs) == 2
    f.close()
    ref.close()


@pytest.mark.gpu
def test_cli_refit_tiles(tmp_path):
    from test_png_io import encode_png
    h = 32
    src = str(tmp_path / "src.png")
    open(src, "wb").write(encode_png(B.image(h, 7).astype(np.int64), 6, 8))
    common = ["-c", "2", "-s", "3", "--calls", "6", "--candidates", "16"]
    plain = str(tmp_path / "plain.json")
    r = cli(src, plain, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    N = M.count_unique(json.load(open(plain))["tiles"]) - 9
    out, tm = str(tmp_path / "out.json"), str(tmp_path / "tm.json")
    r = cli(src, out, *common, "--max-tiles", str(N), "--merge-shortlist", "4", "--refit-tiles", "3", "--tilemap", tm)
    assert r.returncode == 0, r.stdout + r.stderr
    js, t1 = json.load(open(out)), json.load(open(tm))
    assert M.unflip_tilemap(t1) == js["tiles"] and len(t1["characters"]) <= N and M.count_unique(js["tiles"]) <= N
    assert js["palette"] == json.load(open(plain))["palette"] and js["tile_palettes"] == json.load(open(plain))["tile_palettes"]
    sweeps = re.findall(r"Refit sweep (\d+): (\d+) calls, (\d+) accepted, (\d+) skipped; error (\S+) -> (\S+); (\d+) characters", r.stdout)
    assert 1 <= len(sweeps) <= 3 and [int(s[0]) for s in sweeps] == list(range(1, len(sweeps) + 1)), r.stdout
    merged = float(re.search(r"Error: \S+ -> (\S+)", r.stdout).group(1))
    assert float(sweeps[0][4]) == merged
    for j, s in enumerate(sweeps):
        assert float(s[5]) <= float(s[4]) and int(s[6]) <= N and int(s[2]) + int(s[3]) <= int(s[1])
        assert (float(s[5]) < float(s[4])) == (int(s[2]) > 0)
        if j:
            assert float(s[4]) == float(sweeps[j - 1][5])
    assert all(int(s[2]) > 0 for s in sweeps[:-1]) and (len(sweeps) == 3 or int(sweeps[-1][2]) == 0)
    assert r.stdout.index("Refit sweep 1") > r.stdout.index("Characters:") and r.stdout.index("Refit sweep 1") < r.stdout.index("Writing output")
    # without --max-tiles it runs behind the last optimizer call
    r = cli(src, str(tmp_path / "o3.json"), *common, "--refit-tiles", "1")
    assert r.returncode == 0 and "Refit sweep 1" in r.stdout and "Characters:" not in r.stdout, r.stdout + r.stderr
    # refused while parsing (exit code 2, before any file or device is touched: the source does not exist)
    missing, o2 = str(tmp_path / "none.png"), str(tmp_path / "o2.json")
    for extra in (["--refit-tiles", "2", "--share", "a=b"], ["--refit-tiles", "2", "--devices", "0,1"], ["--refit-tiles", "0"], ["--refit-tiles", "17"],
                  ["--refit-tiles", "x"], ["--refit-tiles", "2x"], ["--refit-tiles", "-1"], ["--refit-tiles"]):
        r = cli(missing, o2, *extra)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
    assert not os.path.exists(o2)
    assert "--refit-tiles" in cli("--help").stderr
