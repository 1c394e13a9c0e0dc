"""The character budget of a shared-palette set (snesimage_shared_characters, _merge_shortlist, _score_merges,
_reduce_characters, _as_tilemap_json): the characters of all members counted together, merges whose donor may sit in another
member, each step decided on the increase of the recipient member's error.  The model is tests/set_character_model.py over
the unchanged CPU oracle (its premises: tests/test_set_character_model.py): everything integer is compared exactly, errors
within 1e-11 relative, product against product bit for bit."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_model as B
import character_model as M
import set_character_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
SET_FUNCS = ["snesimage_shared_characters", "snesimage_shared_merge_shortlist", "snesimage_shared_score_merges", "snesimage_shared_reduce_characters",
             "snesimage_shared_as_tilemap_json"]
ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -5
REC_INTS = ("cost", "member", "tile", "donor_member", "donor", "flip", "rank", "unique")


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def tile_px(img, t):
    return img[(t // 32) * 8:(t // 32) * 8 + 8, (t % 32) * 8:(t % 32) * 8 + 8]


def flip_px(px, f):
    px = px[::-1] if f & 2 else px
    return px[:, ::-1] if f & 1 else px


def explicit_palette(count, size, seed, first=None):
    pal = np.random.default_rng(seed).integers(0, 32, (count * size, 3)).astype(np.uint8)
    if first is not None:
        pal[::size] = first  # entry 0 of every subpalette
    return pal


def make_set(S, O, imgs, count, size, flags=None, start="oracle", ordered=None, seed=0, first=None):
    """A set with every context at set_chunk(64) and the model's oracles in the same state.  start: "oracle" = the oracle's
    initialisers on the member stack, handed to the members; "gpu" = the set's own initialisers; "explicit" = a random palette
    and random tile palettes."""
    flags = dict(flags or {})
    h = imgs[0].shape[0]
    ctxs = [S.OptimizedImage(f, count, size, device=0, **flags) for f in imgs]
    for c in ctxs:
        c.set_chunk(64)
    if start == "oracle":
        tps, pal = SM.stack_start(O, imgs, count, size, **flags)
    elif start == "explicit":
        rng = np.random.default_rng(seed + 100)
        pal = explicit_palette(count, size, seed, first)
        tps = []
        for _ in imgs:
            tp = np.zeros(1024, np.uint8)
            tp[:32 * (h // 8)] = rng.integers(0, count, 32 * (h // 8))
            tps.append(tp)
    if start != "gpu":
        for c, tp in zip(ctxs, tps):
            c.tile_palettes = tp
            c.palette = pal
    sp = S.SharedPalette(ctxs, ordered_dither=ordered)
    if start == "gpu":
        sp.initialize_tiles()
        sp.recalculate_palettes()
        tps, pal = [c.tile_palettes for c in ctxs], sp.palette
    oms = SM.oracle_members(O, imgs, tps, pal, count, size, **flags)
    for c, o in zip(ctxs, oms):
        if ordered is not None:
            o.palette_map = c.palette_map  # (the oracle knows no ordered table: the map is the product's, error() the oracle's)
        assert np.array_equal(c.palette_map, o.palette_map) and np.array_equal(c.tile_palettes, o.tile_palettes)
    return ctxs, sp, oms, SM.SetBudget(O, oms, imgs)


def close_all(sp, ctxs, oms=()):
    sp.close()
    for c in ctxs:
        c.close()
    for o in oms:
        o.close()


def state_of(sp, ctxs):
    return [(c.tile_palettes.tobytes(), c.palette_map.tobytes(), c.palette.tobytes(), c.error()) for c in ctxs], sp.error()


def short_tuples(sp, K, ntile):
    mem, t, dmem, d, f, cost = sp.merge_shortlist(K)
    return [(int(c), int(m) * ntile + int(tt), int(dm) * ntile + int(dd), int(ff)) for c, m, tt, dm, dd, ff in zip(cost, mem, t, dmem, d, f)]


def check_characters(sp, ctxs, imgs):
    """snesimage_shared_characters and the set's tilemap JSON against numpy, and against the members' own JSON."""
    chars = np.concatenate([M.characters(c.palette_map, img) for c, img in zip(ctxs, imgs)])
    rep, flip, U, _ = M.classes(chars)
    u, r, f, c = sp.characters()
    assert np.array_equal(c, chars)
    assert u == U and np.array_equal(r, rep) and np.array_equal(f, flip)
    tiles = [json.loads(x.as_json())["tiles"] for x in ctxs]
    assert [t for m in tiles for t in m] == chars.tolist()
    tm = sp.as_tilemap_json()
    assert tm == SM.set_tilemap_json(chars, [x.tile_palettes for x in ctxs])
    d = json.loads(tm)
    assert list(d) == ["character", "characters", "hflip", "palette", "vflip"] and len(d["characters"]) == U
    assert SM.unflip_set_tilemap(d) == tiles
    return U, rep, flip, chars


def assert_record(got, want, j=None):
    for k in REC_INTS:
        assert int(got[k]) == want[k], (j, k, got, want)
    for k in ("error", "member_error"):
        assert abs(float(got[k]) - want[k]) <= M.REL_ERR * abs(want[k]), (j, k, got[k], want[k])


# ---- symbols ---------------------------------------------------------------------------------------------------------------

def test_set_character_symbols_exported_declared_and_bound(S):
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in SET_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    assert "snesimage_shared_merge_result" in text
    assert C.sizeof(_ffi.SharedMergeResult) == 40 and S.shared.SHARED_MERGE_LOG_DTYPE.names[:2] == ("error", "member_error")
    n = C.c_uint32(0)
    assert lib.snesimage_shared_characters(None, C.byref(n), None, None, None) == ERR_ARG and b"null set" in lib.snesimage_last_error()
    assert lib.snesimage_shared_merge_shortlist(None, 1, None, None, None, None, None, None, C.byref(n)) == ERR_ARG
    assert lib.snesimage_shared_score_merges(None, None, None, None, None, None, 0, None, None) == ERR_ARG
    assert lib.snesimage_shared_reduce_characters(None, 1, 0, None, 0, None, None) == ERR_ARG
    assert lib.snesimage_shared_as_tilemap_json(None, None, 0) == ERR_ARG


def test_argument_refusals(S, O):
    imgs = [B.image(16, 30).copy(), B.image(16, 31)]
    tile_px(imgs[0], 9)[..., 3] = 0  # tile 9 of member 0 is pinned
    ctxs, sp, oms, sb = make_set(S, O, imgs, 1, 7, start="explicit", seed=3)
    before = state_of(sp, ctxs)
    for args in [([2], [0], [0], [1], [0]), ([0], [64], [0], [1], [0]), ([0], [0], [2], [1], [0]), ([0], [0], [1], [64], [0]),  # member or tile out of range
                 ([0], [9], [1], [1], [0]), ([1], [1], [0], [9], [0]),                                                          # a pinned tile named
                 ([1], [5], [1], [5], [0]), ([0], [0], [1], [1], [4])]:                                                         # gt == gb, f > 3
        with pytest.raises(S.SnesImageError) as ei:
            sp.score_merges(*args)
        assert ei.value.code == ERR_ARG, args
    assert np.isfinite(sp.score_merges([0], [5], [1], [5], [0])).all()  # the same tile number in another member is another tile
    for call in (lambda: sp.reduce_characters(0), lambda: sp.reduce_characters(4, 65), lambda: sp.merge_shortlist(65)):
        with pytest.raises(S.SnesImageError) as ei:
            call()
        assert ei.value.code == ERR_ARG
    assert state_of(sp, ctxs) == before
    close_all(sp, ctxs, oms)


# ---- classes across members ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [2, 3])
def test_classes_across_members(S, O, F):
    """Frame 1 holds pixel copies of four of frame 0's tiles at other positions, one per flip (1 x 7 without dithering: a tile's
    indices depend on its pixels alone); a fully transparent tile in each of two members forms one class of pinned tiles."""
    h = 16
    imgs = [B.image(h, 10 + i).copy() for i in range(F)]
    for f in range(4):
        tile_px(imgs[1], 20 + 5 * f)[:] = flip_px(tile_px(imgs[0], 3 + f), f)
    tile_px(imgs[0], 9)[..., 3] = 0
    tile_px(imgs[F - 1], 40)[..., 3] = 0
    ctxs, sp, oms, sb = make_set(S, O, imgs, 1, 7, start="explicit", seed=1)
    before = state_of(sp, ctxs)
    U, rep, flip, chars = check_characters(sp, ctxs, imgs)
    ntile = 64
    for f in range(4):
        assert rep[ntile + 20 + 5 * f] == 3 + f and flip[ntile + 20 + 5 * f] == f
    g_clear = (F - 1) * ntile + 40
    assert rep[g_clear] == 9 and not chars[9].any() and not chars[g_clear].any()
    own = [M.classes(chars[i * ntile:(i + 1) * ntile])[2] for i in range(F)]
    assert U < sum(own), "the premise: a character occurs in two members"
    assert state_of(sp, ctxs) == before
    close_all(sp, ctxs, oms)


# ---- past 1,024 global tiles -----------------------------------------------------------------------------------------------

def frames_past_1024():
    h, F, ntile = 96, 3, 384
    base = B.image(h, 20)
    pool = [tile_px(base, t).copy() for t in (0, 37, 150, 222, 383)]
    odd = tile_px(base, 100)
    unique = {0: (3, 100), 1: (7, 200), 2: (260, 270, 300, 310, 350, 383)}
    imgs, u = [], 0
    for i in range(F):
        img = np.zeros_like(base)
        for t in range(ntile):
            tile_px(img, t)[:] = pool[(t + i) % 5]
        for t in unique[i]:
            tile_px(img, t)[:] = odd
            y, x = u % 8, (3 * u + u // 8) % 8
            tile_px(img, t)[y, x, :3] = 255 - odd[y, x, :3]
            u += 1
        imgs.append(img)
    return imgs, ntile


def test_characters_and_shortlist_past_1024_global_tiles(S, O):
    """Three frames of 96 rows (G = 1,152) in the k-means start, most tiles pixel copies of five, so that few are recipients:
    characters, classes and the shortlist (K = 4 and 64) are the model's; nothing is scored.  The other tiles are one more
    tile with one pixel inverted, a different one each: they are each other's cheapest donors, most of them in member 2."""
    imgs, ntile = frames_past_1024()
    ctxs, sp, oms, sb = make_set(S, O, imgs, 1, 7, start="gpu")
    before = state_of(sp, ctxs)
    U, rep, flip, chars = check_characters(sp, ctxs, imgs)
    assert U <= 5 + 10
    cand = sb.candidates()
    assert len(cand) > 64
    for K in (4, 64):
        assert short_tuples(sp, K, ntile) == cand[:K], K
    assert any(gt > 1023 for _, gt, _, _ in cand[:64]) and any(gb > 1023 for _, _, gb, _ in cand[:64]), "the premise: indices beyond the single-image kernels' range"
    assert state_of(sp, ctxs) == before
    close_all(sp, ctxs, oms)


# ---- shortlist edge cases --------------------------------------------------------------------------------------------------

def test_shortlist_with_few_and_with_no_candidates(S, O):
    h = 16
    base = B.image(h, 25)
    # (a) every tile a copy of one, but one tile in each member: recipients those two, donors the common tile and the other one
    imgs = []
    for i in range(2):
        img = np.zeros_like(base)
        for t in range(64):
            tile_px(img, t)[:] = tile_px(base, 0)
        tile_px(img, 10 + 30 * i)[:] = tile_px(base, (40, 63)[i])
        imgs.append(img)
    ctxs, sp, oms, sb = make_set(S, O, imgs, 1, 7, start="explicit", seed=2)
    cand = sb.candidates()
    assert len(cand) == 2 * 2 * 4
    assert short_tuples(sp, 64, 64) == cand and short_tuples(sp, 4, 64) == cand[:4]
    assert {gt for _, gt, _, _ in cand} == {10, 64 + 40}
    close_all(sp, ctxs, oms)
    # (b) every unpinned tile already shared: nothing to merge, and that is no error
    imgs = []
    for i in range(2):
        img = np.zeros_like(base)
        for t in range(64):
            tile_px(img, t)[:] = tile_px(base, 0)
        imgs.append(img)
    ctxs, sp, oms, sb = make_set(S, O, imgs, 1, 7, start="explicit", seed=2)
    assert sp.characters()[0] == 1 and [len(a) for a in sp.merge_shortlist(16)] == [0] * 6
    before = state_of(sp, ctxs)
    recs, U = sp.reduce_characters(1, 4)
    assert len(recs) == 0 and U == 1
    imgs2 = [imgs[0], B.image(h, 26).copy()]  # and a budget that cannot be met: every tile of member 1 pinned
    close_all(sp, ctxs, oms)
    imgs2[1][::8, ::8, 3] = 0
    ctxs, sp, oms, sb = make_set(S, O, imgs2, 1, 7, start="explicit", seed=2)
    U0 = sp.characters()[0]
    before = state_of(sp, ctxs)
    recs, U = sp.reduce_characters(1, 4)
    assert U0 > 1 and len(recs) == 0 and U == U0 and state_of(sp, ctxs) == before
    close_all(sp, ctxs, oms)


# ---- score_merges against the oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,flags,ordered", [
    ("rgb", {}, False), ("perceptual", {"perceptual": True}, False), ("dither", {"dither": True}, False), ("ordered", {}, True),
], ids=["rgb", "perceptual", "dither", "ordered"])
def test_score_merges_matches_the_oracle(S, O, name, flags, ordered):
    """Explicit candidates — a donor in the other member under each flip, pairs inside a member, shortlisted ones, two that change
    nothing — against the oracle with the candidate's map set by hand; set and members are as if the call had not been made."""
    h, count, size, ntile = 16, 2, 3, 64
    X = np.array([10, 20, 5], np.uint8)
    flat = np.array(list(O.snes_as_rgba(X)[:3]) + [255], np.uint8)
    imgs = [B.image(h, 40).copy(), B.image(h, 41).copy()]
    for i, t in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1)):  # the top-left tiles are flat in a colour the palette holds at entry 0 of every
        tile_px(imgs[i], t)[:] = flat                      # subpalette: equal indices whatever the flags (the last one of each row of flat
                                                           # tiles keeps the diffused error of its neighbour away from the others)
    table = S.bayer_offsets(4, 64) if ordered else None

    def build():
        return make_set(S, O, imgs, count, size, flags, start="explicit", ordered=table, seed=7, first=X)
    ctxs, sp, oms, sb = build()
    chars = sb.chars()
    assert np.array_equal(chars[0], chars[1]) and np.array_equal(chars[0], chars[ntile])
    before = state_of(sp, ctxs)
    incs = [c.error() for c in ctxs]
    for c, o in zip(ctxs, oms):
        assert abs(c.error() - o.error()) <= M.REL_ERR * o.error()
    cands = [(0, 3, 1, 10, f) for f in range(4)] + [(1, 5, 0, 7, 2), (0, 8, 0, 9, 1), (1, 63, 1, 2, 3)]
    cands += [(gt // ntile, gt % ntile, gb // ntile, gb % ntile, f) for _, gt, gb, f in sb.shortlist(4)]
    cands += [(0, 1, 0, 0, 0), (1, 0, 0, 1, 0), cands[0]]
    cols = [[c[k] for c in cands] for k in range(5)]
    errs, maps = sp.score_merges(*cols, want_maps=True)
    for j, (m, t, dm, d, f) in enumerate(cands):
        e, mp = sb.score(m * ntile + t, dm * ntile + d, f)
        assert np.array_equal(maps[j], mp), (j, cands[j])
        assert abs(errs[j] - e) <= M.REL_ERR * abs(e), (j, cands[j], errs[j], e)
    assert errs[11] == incs[0] and errs[12] == incs[1]  # nothing changes: the member's incumbent bit for bit
    assert errs[13] == errs[0] and len(set(errs.tolist())) > 8
    assert state_of(sp, ctxs) == before
    assert np.array_equal(sp.score_merges(*[c[:3] for c in cols]), errs[:3])
    # the epochs have no getter: the set still takes a call (it is intact), and the call goes as on a twin that never scored
    ctxs2, sp2, oms2, _ = build()
    assert state_of(sp2, ctxs2) == before
    for j, index in enumerate((1, 2)):
        e_g, b_g = sp.step(S.METHOD_RANDOM, 0, index, 0, 3, j, 16)
        e_t, b_t = sp2.step(S.METHOD_RANDOM, 0, index, 0, 3, j, 16)
        assert e_g == e_t and np.array_equal(b_g, b_t)
    assert state_of(sp, ctxs) == state_of(sp2, ctxs2)
    close_all(sp2, ctxs2, oms2)
    close_all(sp, ctxs, oms)


# ---- the reduction ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SM.TRAJECTORIES))
def test_reduce_characters_follows_the_models_trajectory(S, O, name):
    """From the k-means start of the member stack: every record exact in its integers, member_error and error within 1e-11,
    every member's final map exact, sp.error() the last record's bits, U that of the members' JSON tiles deduplicated together;
    a further call goes on from the reduced state by one more model step."""
    imgs, count, size, flags, K, steps = SM.trajectory_inputs(name)
    ctxs, sp, oms, sb = make_set(S, O, imgs, count, size, flags)
    U0 = sb.state()[3]
    assert sp.characters()[0] == U0
    want, Uw = sb.reduce(U0 - steps, K)
    SM.assert_trajectory_decides(want)
    recs, U = sp.reduce_characters(U0 - steps, K)
    assert len(recs) == len(want) == steps and U == Uw == U0 - steps
    for j, (g, w) in enumerate(zip(recs, want)):
        assert_record(g, w, j)
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette_map, o.palette_map) and json.loads(c.as_json())["tiles"] == json.loads(o.as_json())["tiles"]
    assert sp.error() == recs[-1]["error"]
    tiles = [t for c in ctxs for t in json.loads(c.as_json())["tiles"]]
    assert M.count_unique(tiles) == U and sp.characters()[0] == U
    assert SM.unflip_set_tilemap(json.loads(sp.as_tilemap_json())) == [json.loads(c.as_json())["tiles"] for c in ctxs]
    more, U2 = sp.reduce_characters(U - 1, K)
    w = sb.step(K)
    assert len(more) == 1 and U2 == U - 1
    assert_record(more[0], w, "further")
    assert sp.error() == more[0]["error"]
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette_map, o.palette_map)
    close_all(sp, ctxs, oms)


# ---- state rules -----------------------------------------------------------------------------------------------------------

def test_budget_met_and_the_state_after_a_reduction(S, O):
    from snesimage_amd import _ffi
    L = _ffi.load()
    imgs, count, size, flags, K, _ = SM.trajectory_inputs("rgb_2x3")
    ctxs, sp, oms, sb = make_set(S, O, imgs, count, size, flags)
    twin_ctxs, twin, twin_oms, _ = make_set(S, O, imgs, count, size, flags)
    U0 = sb.state()[3]
    before = state_of(sp, ctxs)
    assert before == state_of(twin, twin_ctxs)
    # a failed workspace allocation (the set's own arrays on first use; then a member's scoring workspace): usable and unchanged
    for n in (0, 3):
        L.snesimage_debug_fail_alloc(n)
        try:
            with pytest.raises(S.SnesImageError) as ei:
                sp.reduce_characters(U0 - 2, K)
        finally:
            L.snesimage_debug_fail_alloc(-1)
        assert ei.value.code == ERR_HIP and state_of(sp, ctxs) == before
        assert sp.characters()[0] == U0  # (allocates the set's arrays: the second round fails behind them)
    for budget in (U0, U0 + 5, 8192):  # a budget already met: untouched bit for bit
        recs, U = sp.reduce_characters(budget, K)
        assert len(recs) == 0 and U == U0 and state_of(sp, ctxs) == before
    recs, U = sp.reduce_characters(U0 - 3, K)
    assert len(recs) == 3 and U == U0 - 3 and sp.error() == recs[-1]["error"] and sp.error() != before[1]
    for j, w in enumerate(sb.reduce(U0 - 3, K)[0]):
        assert_record(recs[j], w, j)
    with pytest.raises(S.SnesImageError) as ei:  # a member stays lent to the set
        ctxs[0].reduce_characters(4)
    assert ei.value.code == ERR_STATE
    E = sp.error()
    cand = S.random_candidates(5, 0, 4)  # remapped from the palette, no stored map read: the twin's E_k, and the merged maps stay
    assert np.array_equal(sp.score_candidates(0, 1, cand), twin.score_candidates(0, 1, cand)) and sp.error() == E
    # reduction is the last stage of a run: a set call that optimizes goes as on the twin that never reduced
    assert sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)[0] == twin.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)[0]
    assert state_of(sp, ctxs) == state_of(twin, twin_ctxs)
    sp.reduce_characters(U0 - 2, K)
    got = sp.run_slots(5, seed=4, first_step_id=1, n_random=16)
    ref = twin.run_slots(5, seed=4, first_step_id=1, n_random=16)
    assert [(g[0], g[1], g[2].tolist(), g[3]) for g in got[0]] == [(r[0], r[1], r[2].tolist(), r[3]) for r in ref[0]] and got[1] == ref[1]
    assert state_of(sp, ctxs) == state_of(twin, twin_ctxs)
    close_all(twin, twin_ctxs, twin_oms)
    close_all(sp, ctxs, oms)


def test_a_destroyed_member_retires_the_set_for_the_character_calls(S):
    """As every set call: SNES_ERR_STATE, said before any member is looked at."""
    imgs = [B.image(16, 30), B.image(16, 31)]
    ctxs = [S.OptimizedImage(f, 1, 7, device=0) for f in imgs]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    assert sp.characters()[0] > 1
    ctxs[1].close()
    for call in (sp.characters, sp.merge_shortlist, lambda: sp.score_merges([0], [0], [1], [1], [0]), lambda: sp.score_merges([], [], [], [], []),
                 lambda: sp.reduce_characters(4), sp.as_tilemap_json):
        with pytest.raises(S.SnesImageError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    sp.close()
    ctxs[0].close()


def test_more_than_8192_global_tiles_are_refused(S):
    """Nine members of 256 x 256: G = 9,216.  Every new entry point answers SNES_ERR_UNSUPPORTED."""
    from snesimage_amd.synth import synth_image
    img = synth_image(0x5EED5A00, 256, 256, 0)
    ctxs = [S.OptimizedImage(img, 1, 3, device=0) for _ in range(9)]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    for call in (sp.characters, sp.merge_shortlist, lambda: sp.score_merges([0], [0], [1], [1], [0]), lambda: sp.reduce_characters(100), sp.as_tilemap_json):
        with pytest.raises(S.SnesImageError) as ei:
            call()
        assert ei.value.code == ERR_UNSUPPORTED
    sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 8)
    close_all(sp, ctxs)


# ---- the headless driver ---------------------------------------------------------------------------------------------------

def test_cli_max_set_tiles_and_set_tilemap(tmp_path):
    from snesimage_amd.synth import synth_image
    imgs = [synth_image(0x5EED5B00 + i, 256, 32, 0) for i in range(2)]
    for i, f in enumerate(imgs):
        (tmp_path / ("f%d.rgba" % i)).write_bytes(f.tobytes())

    def args(tag):
        return [str(tmp_path / "f0.rgba"), str(tmp_path / ("%s0.json" % tag)), "--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / ("%s1.json" % tag)),
                "-c", "2", "-s", "3", "--calls", "12", "--candidates", "8"]
    r0 = cli(*args("p"))
    assert r0.returncode == 0, r0.stdout + r0.stderr
    # without the new flags: byte for byte what the parent commit's CLI writes.  The reference is a recorded fixture, not a parent
    # binary built by the test: tests/golden/set_cli_frame{0,1}.json are the two files the CLI of the commit before this feature
    # wrote for these frames and these arguments on an MI355X.
    for i in range(2):
        assert (tmp_path / ("p%d.json" % i)).read_bytes() == open(os.path.join(ROOT, "tests", "golden", "set_cli_frame%d.json" % i), "rb").read(), i
    plain = [json.loads((tmp_path / ("p%d.json" % i)).read_text()) for i in range(2)]
    U0 = M.count_unique([t for p in plain for t in p["tiles"]])
    N = U0 - 8
    tm_file = tmp_path / "set.tilemap.json"
    r = cli(*args("o"), "--max-set-tiles", str(N), "--merge-shortlist", "4", "--set-tilemap", str(tm_file))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Characters of the set: %d -> %d in 8 merges (budget %d)" % (U0, N, N) in r.stdout
    outs = [json.loads((tmp_path / ("o%d.json" % i)).read_text()) for i in range(2)]
    assert M.count_unique([t for o in outs for t in o["tiles"]]) <= N
    tm = json.loads(tm_file.read_text())
    assert SM.unflip_set_tilemap(tm) == [o["tiles"] for o in outs] and len(tm["characters"]) == N
    assert [o["palette"] for o in outs] == [p["palette"] for p in plain] and [o["tile_palettes"] for o in outs] == [p["tile_palettes"] for p in plain]
    # the tilemap alone, without a budget: the plain run's tiles
    r2 = cli(*args("q"), "--set-tilemap", str(tmp_path / "q.tilemap.json"))
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert [(tmp_path / ("q%d.json" % i)).read_text() for i in range(2)] == [(tmp_path / ("p%d.json" % i)).read_text() for i in range(2)]
    assert SM.unflip_set_tilemap(json.loads((tmp_path / "q.tilemap.json").read_text())) == [p["tiles"] for p in plain]
    # a budget nobody can meet is reported, not an error
    r3 = cli(*args("u"), "--max-set-tiles", "1")
    assert r3.returncode == 0 and "the budget is not met" in r3.stdout
    # wrong combinations and values: exit code 2, nothing written
    share = ["--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / "x1.json")]
    out = tmp_path / "x0.json"
    for extra in (["--max-set-tiles", "10"], ["--set-tilemap", str(tmp_path / "x.tm")], share + ["--max-set-tiles", "0"], share + ["--max-set-tiles", "8193"],
                  share + ["--max-set-tiles", "ten"], share + ["--max-set-tiles", "10", "--devices", "0,1"], share + ["--max-set-tiles", "10", "--merge-shortlist", "65"],
                  share + ["--max-set-tiles"], share + ["--max-tiles", "10"], share + ["--refit-tiles", "1"], share + ["--tilemap", str(tmp_path / "x.tm")],
                  share + ["--merge-shortlist", "4"]):
        rr = cli(str(tmp_path / "f0.rgba"), str(out), *extra, "-c", "2", "-s", "3")
        assert rr.returncode == 2, (extra, rr.stdout, rr.stderr)
        assert not out.exists() and not (tmp_path / "x1.json").exists() and not (tmp_path / "x.tm").exists()
    h = cli("--help")
    assert all(k in h.stderr for k in ("--max-set-tiles", "--set-tilemap"))
