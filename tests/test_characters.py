"""The character budget (snesimage_characters, snesimage_merge_shortlist, snesimage_score_merges,
snesimage_reduce_characters, snesimage_as_tilemap_json): counting the distinct characters of a result, merging tiles until a
budget is met — every merge chosen by error() among the proxy's shortlist — and the tilemap that follows.  The model is
tests/character_model.py over the unchanged CPU oracle: everything integer is compared exactly, errors within 1e-11 relative,
product against product bit for bit."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_model as B
import character_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
CHAR_FUNCS = ["snesimage_characters", "snesimage_merge_shortlist", "snesimage_score_merges", "snesimage_reduce_characters", "snesimage_as_tilemap_json"]
ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3
# a character that is its own image under a horizontal flip and under no other: values 0 .. 2
HSYM = np.array([[(min(x, 7 - x) + y) % 3 for x in range(8)] for y in range(8)], np.uint8).reshape(64)


# ---- the model's own checks (no device, no product) -------------------------------------------------------------------------

def test_flips_compose_as_a_group():
    c = np.arange(64, dtype=np.uint8)
    for f in range(4):
        for g in range(4):
            assert np.array_equal(M.flip_char(M.flip_char(c, f), g), M.flip_char(c, f ^ g))
    assert M.flip_char(c, 1)[0] == 7 and M.flip_char(c, 2)[0] == 56 and M.flip_char(c, 3)[0] == 63  # bit 0 horizontal, bit 1 vertical
    many = np.arange(128, dtype=np.uint8).reshape(2, 64)
    assert np.array_equal(M.flip_char(many, 3)[1], M.flip_char(many[1], 3))


def test_class_counting_on_hand_made_characters():
    rng = np.random.default_rng(1)
    a, b = rng.integers(1, 5, 64).astype(np.uint8), rng.integers(1, 5, 64).astype(np.uint8)
    flat = np.full(64, 3, np.uint8)
    hsym = HSYM + 1
    assert np.array_equal(M.flip_char(hsym, 1), hsym) and not np.array_equal(M.flip_char(hsym, 2), hsym)
    chars = np.stack([a, b, M.flip_char(a, 1), flat, M.flip_char(a, 2), M.flip_char(b, 3), flat, M.flip_char(hsym, 2), a, hsym, np.zeros(64, np.uint8)])
    rep, flip, U, size = M.classes(chars)
    assert rep.tolist() == [0, 1, 0, 3, 0, 1, 3, 7, 0, 7, 10]
    assert flip.tolist() == [0, 0, 1, 0, 2, 3, 0, 0, 0, 2, 0]  # a flat tile is its own image under all flips: flip_of = 0; hsym: 2, not 3
    assert U == 5 and size.tolist() == [4, 2, 4, 2, 4, 2, 2, 2, 4, 2, 1]
    assert M.count_unique(chars) == 5
    tm = json.loads(M.tilemap_json(chars, np.zeros(11, np.uint8)))
    assert M.unflip_tilemap(tm) == chars.tolist() and len(tm["characters"]) == 5 and list(tm) == ["character", "characters", "hflip", "palette", "vflip"]


def test_packed_key_order_equals_the_tuple_order():
    rng = np.random.default_rng(2)
    tup = [(int(rng.integers(0, 3)) * int(rng.integers(0, 1 << 36)), int(rng.integers(1024)), int(rng.integers(1024)), int(rng.integers(4))) for _ in range(4000)]
    tup += [((1 << 37) - 1, 1023, 1023, 3), (0, 0, 0, 0), (5, 1023, 0, 0), (5, 0, 1023, 3), (6, 0, 0, 0)]
    keys = [M.pack_key(*t) for t in tup]
    assert max(keys) < 1 << 59
    assert [t for _, t in sorted(zip(keys, tup))] == sorted(tup)
    assert len(set(keys)) == len(set(tup))


def test_model_key_is_the_oracles(O):
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 256, (200, 3)), rng.integers(0, 256, (200, 3))
    a[:2], b[:2] = [[255, 0, 255], [0, 0, 0]], [[0, 255, 0], [255, 255, 255]]
    want = [O.red_mean_key(x, y) for x, y in zip(a.astype(np.uint8), b.astype(np.uint8))]
    assert M.red_mean_keys(a, b).tolist() == want
    assert 64 * max(want) < 1 << 37


# ---- on the MI355X -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def state_of(g):
    return g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.palette.tobytes(), g.error()


GEOMETRY = {  # name: (sub_count, sub_size, backdrop, h)
    "2x3": (2, 3, False, 32),
    "4x7_backdrop": (4, 7, True, 40),
    "1x40": (1, 40, False, 16),
}


def make_pair(S, O, img, count, size, backdrop, flags):
    """A product context and the model's oracle (the expanded one for a backdrop) in the k-means start."""
    g = S.OptimizedImage(img, count, size, backdrop=backdrop, **flags)
    g.initialize_tiles()
    g.recalculate_palettes()
    if backdrop:
        o = B.Model(O, img, count, size, flags).o
    else:
        o = O.OracleImage(img, count, size, **flags)
        o.initialize_tiles()
        o.recalculate_palettes()
    assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, o.palette_map)
    return g, o, M.Budget(O, o, img, size if backdrop else None)


def check_characters(g, img, zero_at=None):
    """snesimage_characters, the tilemap JSON and as_json's tiles against numpy."""
    chars = M.characters(g.palette_map, img, zero_at)
    rep, flip, U, _ = M.classes(chars)
    u, r, f, c = g.characters()
    assert np.array_equal(c, chars)
    assert u == U and np.array_equal(r, rep) and np.array_equal(f, flip)
    tiles = json.loads(g.as_json())["tiles"]
    assert tiles == chars.tolist() and M.count_unique(tiles) == U
    tm = g.as_tilemap_json()
    assert tm == M.tilemap_json(chars, g.tile_palettes)
    assert M.unflip_tilemap(json.loads(tm)) == tiles
    return U, rep, flip, chars


@pytest.mark.gpu
def test_character_symbols_exported_declared_and_bound():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in CHAR_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    assert "snesimage_merge_result" in text
    assert C.sizeof(_ffi.MergeResult) == 24
    import snesimage_amd as S
    assert S.api.MERGE_LOG_DTYPE.itemsize == 24
    n = C.c_uint32(0)
    assert lib.snesimage_characters(None, C.byref(n), None, None, None) == ERR_ARG and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_merge_shortlist(None, 1, None, None, None, None, C.byref(n)) == ERR_ARG
    assert lib.snesimage_score_merges(None, None, None, None, 0, None, None) == ERR_ARG
    assert lib.snesimage_reduce_characters(None, 1, 0, None, 0, None, None) == ERR_ARG
    assert lib.snesimage_as_tilemap_json(None, None, 0) == ERR_ARG


@pytest.mark.gpu
def test_characters_of_planted_maps(S):
    """Duplicates under each flip, in the same and in different subpalettes, symmetric characters; U, rep, flip and chars exact."""
    h, count, size = 16, 2, 3
    img = B.image(h, 1)
    rng = np.random.default_rng(5)
    vals = rng.integers(0, size, (64, 64)).astype(np.uint8)
    tp = np.zeros(1024, np.uint8)
    tp[:64] = rng.integers(0, count, 64)
    for f in range(4):
        vals[10 + f] = M.flip_char(vals[3], f)      # tiles 10..13: tile 3 under every flip ...
        vals[40 + f] = M.flip_char(vals[20], 3 - f)
    tp[10:14] = tp[3]                               # ... in tile 3's subpalette
    tp[40:44] = 1 - tp[20]                          # ... and in the other one
    vals[30] = vals[31] = 2                         # flat
    vals[50] = HSYM                                 # symmetric under a horizontal flip
    vals[51] = M.flip_char(vals[50], 2)
    vals[60] = M.flip_char(vals[61], 3)             # the higher tile first: rep is the lower index all the same
    g = S.OptimizedImage(img, count, size)
    g.tile_palettes = tp
    g.palette_map = M.untile(vals, h)
    U, rep, flip, _ = check_characters(g, img)
    assert rep[10:14].tolist() == [3, 3, 3, 3] and flip[10:14].tolist() == [0, 1, 2, 3]
    assert rep[40:44].tolist() == [20] * 4 and flip[40:44].tolist() == [3, 2, 1, 0]
    assert rep[31] == 30 and flip[31] == 0 and rep[51] == 50 and flip[51] == 2 and rep[61] == 60 and flip[61] == 3
    assert U == 64 - 11
    g.close()


@pytest.mark.gpu
def test_characters_with_transparency_and_backdrop(S):
    """An alpha_mix image: pinned tiles and a run of fully transparent tiles (one class).  A backdrop context: a backdrop pixel
    and a transparent pixel both read 0, so such tiles share a character."""
    from adversarial_images import alpha_mix
    img = alpha_mix(32)
    g = S.OptimizedImage(img, 4, 7)
    g.initialize_tiles()
    g.recalculate_palettes()
    U, rep, flip, chars = check_characters(g, img)
    clear = np.flatnonzero(~M.tiles_of(np.ascontiguousarray(img[..., 3])).any(axis=1))
    assert len(clear) >= 2 and (rep[clear] == clear[0]).all() and not chars[clear].any()
    assert M.pinned_tiles(img).sum() > len(clear)
    g.close()
    h, count, size = 16, 4, 7
    img = B.image(h, 2).copy()
    img[0, 16, 3] = 0                                # tile 2, pixel 0: transparent
    g = S.OptimizedImage(img, count, size, backdrop=True)
    rng = np.random.default_rng(6)
    vals = rng.integers(0, size + 1, (64, 64)).astype(np.uint8)  # size = the backdrop
    vals[2] = vals[7]
    vals[2, 0], vals[7, 0] = 4, size                 # the map value under a transparent pixel does not matter; tile 7 shows the backdrop there
    vals[9] = M.flip_char(vals[7], 1)
    g.palette_map = M.untile(vals, h)
    U, rep, flip, chars = check_characters(g, img, zero_at=size)
    assert chars[2, 0] == 0 and chars[7, 0] == 0 and rep[7] == 2 and rep[9] == 2 and flip[9] == 1
    assert (chars[vals == size] == 0).all() and U == 62
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", list(GEOMETRY))
def test_merge_shortlist_is_the_models(S, O, geometry):
    """K = 1, 16 and 64 from the k-means start: tiles, donors, flips and costs exact, min(K, candidates) of them; state unchanged."""
    count, size, backdrop, h = GEOMETRY[geometry]
    img = B.image(h, 0)
    g, o, bud = make_pair(S, O, img, count, size, backdrop, {})
    cand = bud.candidates()
    assert len(cand) > 64
    before = state_of(g)
    for K in (1, 16, 64):
        t, b, f, cost = g.merge_shortlist(K)
        assert list(zip(cost.tolist(), t.tolist(), b.tolist(), f.tolist())) == cand[:K], K
    assert len(g.merge_shortlist()[0]) == 16  # 0 = the default
    assert state_of(g) == before
    g.close()
    o.close()


@pytest.mark.gpu
def test_merge_shortlist_few_candidates_pinned_tiles_and_an_ordered_table(S, O):
    h, count, size = 16, 2, 3
    img = B.image(h, 3)
    # (a) fewer candidates than K: two distinct unpinned characters, everything else a copy of tile 0 -> recipients 1 and 2
    g = S.OptimizedImage(img, count, size)
    o = O.OracleImage(img, count, size)
    for x in (g, o):
        x.initialize_tiles()
        x.recalculate_palettes()
    vals = M.tiles_of(g.palette_map).copy()
    vals[:] = vals[0]
    vals[1], vals[2] = (vals[0] + 1) % size, (vals[0] + 2) % size
    g.palette_map = o.palette_map = M.untile(vals, h)
    cand = M.Budget(O, o, img).candidates()
    assert 0 < len(cand) < 64 and len(cand) == 2 * 2 * 4  # recipients 1, 2; donors 0 and the other one
    t, b, f, cost = g.merge_shortlist(64)
    assert list(zip(cost.tolist(), t.tolist(), b.tolist(), f.tolist())) == cand
    g.close()
    # (b) only pinned tiles: nothing to merge, and that is no error
    holes = img.copy()
    holes[::8, ::8, 3] = 0
    p = S.OptimizedImage(holes, count, size)
    p.initialize_tiles()
    p.recalculate_palettes()
    assert [len(a) for a in p.merge_shortlist(16)] == [0, 0, 0, 0]
    before = state_of(p)
    recs, U = p.reduce_characters(1, 4)
    assert len(recs) == 0 and U == p.characters()[0] and state_of(p) == before
    with pytest.raises(S.SnesImageError) as ei:
        p.score_merges([0], [1], [0])
    assert ei.value.code == ERR_ARG
    p.close()
    # (c) with an ordered-dither table the proxy still reads the original image
    d = S.OptimizedImage(img, count, size)
    d.initialize_tiles()
    d.recalculate_palettes()
    d.set_ordered_dither(S.bayer_offsets(4, 96))
    d.optimize()
    o.tile_palettes, o.palette = d.tile_palettes, d.palette
    o.palette_map = d.palette_map
    want = M.Budget(O, o, img).shortlist(16)
    t, b, f, cost = d.merge_shortlist(16)
    assert list(zip(cost.tolist(), t.tolist(), b.tolist(), f.tolist())) == want
    other = M.Budget(O, o, d.target_rgba()).shortlist(16)  # what a proxy on the dither target would have listed
    assert [c[0] for c in other] != [c[0] for c in want]
    d.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,geometry,flags,ordered,alpha,poison", [
    ("rgb", "2x3", {}, False, True, False),
    ("perceptual", "4x7_backdrop", {"perceptual": True}, False, False, False),
    ("dither", "1x40", {"dither": True}, False, False, True),
    ("ordered", "2x3", {}, True, False, False),
], ids=["rgb", "perceptual_backdrop", "dither_poisoned", "ordered"])
def test_score_merges_matches_the_oracle(S, O, name, geometry, flags, ordered, alpha, poison):
    """Explicit candidates — shortlisted ones, arbitrary unpinned pairs, repeats, one that changes nothing — against the oracle
    with the candidate's map set by hand; the state is as if the call had not been made."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    count, size, backdrop, h = GEOMETRY[geometry]
    h = min(h, 32)
    img = B.image(h, 4).copy()
    if alpha:
        img[8:16, 40:52, 3] = 0  # tile 37 loses every pixel, tile 38 half of them: both pinned
    L.snesimage_debug_poison_alloc(1 if poison else 0)
    try:
        g, o, bud = make_pair(S, O, img, count, size, backdrop, flags)
        if ordered:
            g.set_ordered_dither(S.bayer_offsets(4, 64))
            g.optimize()
        # a stored map that is no optimize() of anything: tile 1 := tile 0 flipped vertically
        vals = M.tiles_of(g.palette_map).copy()
        vals[1] = M.flip_char(vals[0], 2)
        g.palette_map = o.palette_map = M.untile(vals, h)
        inc = g.error()
        assert abs(inc - o.error()) <= M.REL_ERR * inc
        before = state_of(g)
        rng = np.random.default_rng(9)
        free = np.flatnonzero(~bud.pinned)
        cands = [(t, b, f) for _, t, b, f in bud.shortlist(5)]
        cands += [(int(t), int(b), int(rng.integers(4))) for t, b in rng.choice(free, (6, 2), replace=False)]
        cands += [(1, 0, 2), (0, 1, 2), cands[0], (int(free[-1]), int(free[0]), 3)]
        want = {c: bud.score(*c) for c in set(cands)}
        errs, maps = g.score_merges([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], want_maps=True)
        for j, c in enumerate(cands):
            e, m = want[c]
            assert np.array_equal(maps[j], m), (j, c)
            assert abs(errs[j] - e) <= M.REL_ERR * abs(e), (j, c, errs[j], e)
        assert errs[11] == inc and errs[12] == inc  # tile 1 already is tile 0 under flip 2, and the other way round: the incumbent bit for bit
        assert errs[13] == errs[0]
        assert len(set(errs.tolist())) > 8
        assert state_of(g) == before
        assert np.array_equal(g.score_merges([c[0] for c in cands[:3]], [c[1] for c in cands[:3]], [c[2] for c in cands[:3]]), errs[:3])
        # `epoch` has no getter in the ABI: what it guards (the pack, B's run a call ahead) shows in the next step, which goes
        # bit for bit as on a twin context that never scored a merge
        twin = S.OptimizedImage(img, count, size, backdrop=backdrop, **flags)
        twin.initialize_tiles()
        twin.recalculate_palettes()
        if ordered:
            twin.set_ordered_dither(S.bayer_offsets(4, 64))
            twin.optimize()
        twin.palette_map = M.untile(vals, h)
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
def test_score_merges_beyond_a_launch_group(S):
    """600 candidates with set_chunk(512): two launch groups give what the candidates give one by one."""
    h = 16
    img = B.image(h, 5)
    g = S.OptimizedImage(img, 2, 3)
    g.initialize_tiles()
    g.recalculate_palettes()
    g.set_chunk(512)
    rng = np.random.default_rng(10)
    pool = [(int(t), int(b), int(rng.integers(4))) for t, b in (rng.choice(64, 2, replace=False) for _ in range(12))]
    pick = rng.integers(len(pool), size=600)
    ref = g.score_merges([p[0] for p in pool], [p[1] for p in pool], [p[2] for p in pool])
    errs = g.score_merges([pool[i][0] for i in pick], [pool[i][1] for i in pick], [pool[i][2] for i in pick])
    assert np.array_equal(errs, ref[pick]) and np.isfinite(errs).all()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,flags,seed,merges", [
    ("2x3", {}, 0, 12),
    ("4x7_backdrop", {"perceptual": True}, 0, 12),
    ("1x40", {"dither": True}, 0, 6),
], ids=["rgb_h32", "perceptual_backdrop_h40", "dither_h16"])
def test_reduce_characters_follows_the_models_trajectory(S, O, geometry, flags, seed, merges):
    """From the k-means start to U0 - merges with K = 4: every record exact (errors within 1e-11), the final map exact, error()
    afterwards the last record's bits, as_json's tiles deduplicating to the reported U.  The inputs were chosen so that the
    objective overrules the proxy (a winner of rank > 0) and a step raises the error; every decision's gap is 0 or > 1e-9."""
    count, size, backdrop, h = GEOMETRY[geometry]
    img = B.image(h, seed)
    g, o, bud = make_pair(S, O, img, count, size, backdrop, flags)
    U0 = bud.state()[4]
    assert g.characters()[0] == U0
    want, U = bud.reduce(U0 - merges, 4)
    assert len(want) == merges and U == U0 - merges
    M.assert_trajectory_decides(want)
    recs, unique = g.reduce_characters(U0 - merges, 4)
    assert unique == U and len(recs) == merges
    for j, (r, w) in enumerate(zip(recs, want)):
        got = tuple(int(r[k]) for k in ("tile", "donor", "flip", "rank", "cost", "unique"))
        assert got == (w["tile"], w["donor"], w["flip"], w["rank"], w["cost"], w["unique"]), (j, got, w)
        assert abs(float(r["error"]) - w["error"]) <= M.REL_ERR * w["error"], (j, float(r["error"]), w["error"])
    assert np.array_equal(g.palette_map, o.palette_map)
    assert g.error() == float(recs[-1]["error"])
    U1, _, _, _ = check_characters(g, img, size if backdrop else None)
    assert U1 == unique
    assert np.array_equal(g.as_rgba(), o.as_rgba())
    # a further call on the reduced state goes on from it: one more step of the model
    w = bud.step(4)
    recs, unique = g.reduce_characters(U - 1, 4)
    assert len(recs) == 1 and unique == U - 1 and (int(recs[0]["tile"]), int(recs[0]["donor"]), int(recs[0]["flip"])) == (w["tile"], w["donor"], w["flip"])
    assert np.array_equal(g.palette_map, o.palette_map)
    g.close()
    o.close()


BUDGET_GEOMETRY = (16, 2, 3)  # h, sub_count, sub_size of the three tests below


def budget_image():
    img = B.image(BUDGET_GEOMETRY[0], 6).copy()
    img[0, 0, 3] = 0  # tile 0 is pinned
    return img


def budget_ctx(S, img, init=True):
    c = S.OptimizedImage(img, BUDGET_GEOMETRY[1], BUDGET_GEOMETRY[2])
    if init:
        c.initialize_tiles()
        c.recalculate_palettes()
    return c


def refused(S, call, code):
    with pytest.raises(S.SnesImageError) as e:
        call()
    assert e.value.code == code, str(e.value)


def budget_calls(x):
    return (lambda: x.characters(), lambda: x.merge_shortlist(4), lambda: x.score_merges([5], [6], [1]), lambda: x.reduce_characters(10, 4), lambda: x.as_tilemap_json())


@pytest.mark.gpu
def test_failed_character_workspace_allocation_leaves_the_context_usable(S):
    """snesimage_debug_fail_alloc during the first call: SNES_ERR_HIP, the context unchanged, and the next call succeeds."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = budget_image()
    g, ref = budget_ctx(S, img), budget_ctx(S, img)
    before = state_of(g)
    failures = 0
    for nth in (0, 3, 8, 12, 20, 40):
        L.snesimage_debug_fail_alloc(nth)
        try:
            g.reduce_characters(1, 4)
            ok = True
        except S.SnesImageError as e:
            assert e.code == ERR_HIP
            ok = False
            failures += 1
        finally:
            L.snesimage_debug_fail_alloc(-1)
        if ok:
            break
        assert state_of(g) == before
        assert g.characters()[0] == ref.characters()[0]  # the next call succeeds
    assert failures >= 2
    if not ok:  # every attempt failed: the reduction itself still goes as on a context that never saw a failure
        recs, U = g.reduce_characters(ref.characters()[0] - 3, 4)
        want, U_ref = ref.reduce_characters(ref.characters()[0] - 3, 4)
        assert recs.tobytes() == want.tobytes() and U == U_ref and state_of(g) == state_of(ref)
    g.close()
    ref.close()


@pytest.mark.gpu
def test_budget_already_met_and_optimize_afterwards(S):
    """A budget already met takes no step and leaves the state untouched bit for bit; optimize() after a reduction restores the
    unreduced map."""
    img = budget_image()
    g, ref = budget_ctx(S, img), budget_ctx(S, img)
    U0 = g.characters()[0]
    before = state_of(g)
    assert before == state_of(ref)
    for budget in (U0, U0 + 5, 5000):
        recs, U = g.reduce_characters(budget)
        assert len(recs) == 0 and U == U0
    assert state_of(g) == before
    e_g, b_g = g.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)  # and the context steps as one never asked
    e_r, b_r = ref.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)
    assert e_g == e_r and np.array_equal(b_g, b_r) and np.array_equal(g.palette_map, ref.palette_map)
    unreduced, U1 = g.palette_map, g.characters()[0]
    recs, U = g.reduce_characters(U1 - 3, 4)
    assert len(recs) == 3 and U == U1 - 3 and not np.array_equal(g.palette_map, unreduced)
    g.optimize()
    assert np.array_equal(g.palette_map, unreduced) and g.characters()[0] == U1
    g.close()
    ref.close()


@pytest.mark.gpu
def test_character_refusals(S):
    """Every refusal of the header returns its code, and the context is welcome again afterwards."""
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = budget_image()
    g = budget_ctx(S, img)
    U0 = g.characters()[0]
    # SNES_ERR_ARG: a tile beyond the image, a pinned tile named explicitly, t == b, f > 3, max_unique == 0, shortlist > 64
    for call in (lambda: g.score_merges([64], [1], [0]), lambda: g.score_merges([1], [64], [0]), lambda: g.score_merges([0], [1], [0]),
                 lambda: g.score_merges([1], [0], [0]), lambda: g.score_merges([5], [5], [0]), lambda: g.score_merges([5], [6], [4]),
                 lambda: g.reduce_characters(0), lambda: g.reduce_characters(10, 65), lambda: g.merge_shortlist(65)):
        refused(S, call, ERR_ARG)
    # SNES_ERR_STATE: between the phases of a split-phase step and of a split-phase window ...
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    for call in budget_calls(g):
        refused(S, call, ERR_STATE)
    g.step_commit(buf.ptr)
    taken, _ = g.slots_begin(4, 1, 1, (0, 1, 0, 0))
    for call in budget_calls(g):
        refused(S, call, ERR_STATE)
    g.slots_commit(0, taken)
    g.characters()
    # ... and on a context lent to a batch, a set or a group
    a, b = budget_ctx(S, img, init=False), budget_ctx(S, img, init=False)
    for create, destroy in ((L.snesimage_batch_create, L.snesimage_batch_destroy), (L.snesimage_shared_create, L.snesimage_shared_destroy)):
        arr = (C.c_void_p * 2)(a._c, b._c)
        hnd = C.c_void_p()
        assert create(arr, 2, C.byref(hnd)) == 0, L.snesimage_last_error()
        for call in budget_calls(a) + budget_calls(b):
            refused(S, call, ERR_STATE)
        destroy(hnd)
    arr1 = (C.c_void_p * 1)(a._c)
    hnd = C.c_void_p()
    assert L.snesimage_group_create(arr1, 1, C.byref(hnd)) == 0, L.snesimage_last_error()
    for call in budget_calls(a):
        refused(S, call, ERR_STATE)
    L.snesimage_group_destroy(hnd)
    a.initialize_tiles()  # the contexts are their own again
    a.recalculate_palettes()
    assert a.characters()[0] == U0
    for x in (a, b, g):
        x.close()


@pytest.mark.gpu
def test_cli_max_tiles_and_tilemap(tmp_path):
    h = 32
    raw = str(tmp_path / "src.rgba")
    B.image(h, 7).tofile(raw)
    common = [raw, "-c", "2", "-s", "3", "--calls", "6", "--candidates", "16"]
    plain, plain2, tm0 = str(tmp_path / "plain.json"), str(tmp_path / "plain2.json"), str(tmp_path / "tm0.json")
    r = cli(common[0], plain, *common[1:])
    assert r.returncode == 0, r.stdout + r.stderr
    r = cli(common[0], plain2, *common[1:], "--tilemap", tm0)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(plain2, "rb").read() == open(plain, "rb").read()  # the JSON it writes today, byte for byte
    tiles0 = json.load(open(plain))["tiles"]
    U0 = M.count_unique(tiles0)
    t0 = json.load(open(tm0))
    assert M.unflip_tilemap(t0) == tiles0 and len(t0["characters"]) == U0 and t0["palette"] == json.load(open(plain))["tile_palettes"]
    N = U0 - 9
    out, tm = str(tmp_path / "out.json"), str(tmp_path / "tm.json")
    r = cli(common[0], out, *common[1:], "--max-tiles", str(N), "--merge-shortlist", "4", "--tilemap", tm)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Characters: %d -> %d in 9 merges" % (U0, N) in r.stdout and re.search(r"Error: \S+ -> \S+", r.stdout), r.stdout
    js = json.load(open(out))
    assert M.count_unique(js["tiles"]) <= N and js["palette"] == json.load(open(plain))["palette"]
    t1 = json.load(open(tm))
    assert M.unflip_tilemap(t1) == js["tiles"] and len(t1["characters"]) == N
    # refused while parsing (exit code 2, before any file or device is touched: the source does not exist)
    missing, o2 = str(tmp_path / "none.png"), str(tmp_path / "o2.json")
    for extra in (["--max-tiles", "10", "--share", "a=b"], ["--max-tiles", "10", "--devices", "0,1"], ["--merge-shortlist", "4"], ["--max-tiles", "0"],
                  ["--max-tiles", "10", "--merge-shortlist", "65"], ["--max-tiles"]):
        r = cli(missing, o2, *extra)
        assert r.returncode == 2, (extra, r.stdout, r.stderr)
    assert not os.path.exists(o2)
    r = cli("--help")
    assert all(k in r.stderr for k in ("--max-tiles", "--merge-shortlist", "--tilemap"))
