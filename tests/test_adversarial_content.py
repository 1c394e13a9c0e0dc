"""Parity on flat, tied, transparent and extreme-colour images (tests/adversarial_images.py), the content the gradient
family of snesimage_amd/synth.py never shows: duplicate leading k-means points (NaN centres that become black),
subpalettes the initialisers cannot fill (error -4), the tile-mean filter, alpha other than 0 / 255 and transparent
borders, palettes full of duplicate entries (ties on every pixel), candidates that change nothing (errors bit-equal to
the incumbent's), neutral / blue-violet / near-black colours in the two sure "no"s of CIEDE2000, and a 1-pixel
checkerboard that drives Floyd-Steinberg into its clamp.

Bars as in test_gpu_parity.py: palettes, tile palettes and maps bit for bit, errors within REL_ERR = 1e-11 of the CPU
oracle, product path against product path bit for bit.  Every comparison against the oracle stays within 16 calls of 8
candidates; long lists and long runs are GPU against GPU.  The CPU tests pin the premises the GPU tests stand on."""
import hashlib

import numpy as np
import pytest

from adversarial_images import IMAGES, flat_tiles, hand_tiles
from tile_model import assert_log_matches, model_tile_sweep

REL_ERR = 1e-11
GEOMETRIES = [(2, 3), (4, 7), (8, 15)]
NAMES = list(IMAGES)
FLAGSETS = {"rgb": {}, "perceptual": {"perceptual": True}, "dither": {"dither": True},
            "dither_perceptual": {"dither": True, "perceptual": True}}
ALL_IMAGES = dict(IMAGES, flat_tiles=flat_tiles)

SHA256 = {
    ("pixel_art", 32): "37ff4065739d8532a47ba3b74869df47d33679d1cc9896ecf154d3389d364f5a",
    ("pixel_art", 64): "80db0b46c5be33bd73f897ef992f3c2e9afbeb89f1f1f17242f74f3a9ecec382",
    ("alpha_mix", 32): "2a8bed7f92cd3fcb734ea0d2a4d6c0ccd3aa370d7f1ca7ef24ca4452630c62d5",
    ("alpha_mix", 64): "38c37b7d75b932b742b605814460c7052b91bb67f7c1a80511a07ff7a06b4b0e",
    ("two_tone", 32): "3253f58cb6751819c6ab490ed888f3e8120eb8263c895da263cdc337ac85f545",
    ("two_tone", 64): "6fa8e4d0426cccc802827a4adcbffd6b186259d58043bed71f7cdce12ae565cb",
    ("lab_extremes", 32): "64f31f7d4fa59f81a4d8de005a8ce5ebc985de524a0b8d1564638af60a748d7b",
    ("lab_extremes", 64): "394464dd8bd967718676e93ec6d5daf8936c98ec00da9f64d727957aa4526937",
    ("flat_tiles", 32): "c5e4208faec91db4338449a33be029d5bfb80e76076a320c76c03c389150cd64",
    ("flat_tiles", 64): "eb6ae6397082d93a07f3df144757f79f8a88017a1e951d6d781ecb172e6a5839",
}

# (image, flags, geometry) where the oracle's initialize_tiles succeeds and its recalculate_palettes then fails cogset's
# precondition 2 <= k < n (a subpalette left with no tiles or too few points); everywhere else both succeed.
RAISES = ({("two_tone", f, g) for f in ("rgb", "perceptual") for g in GEOMETRIES} |
          {("pixel_art", "rgb", (8, 15)), ("lab_extremes", "rgb", (4, 7)), ("lab_extremes", "rgb", (8, 15)),
           ("alpha_mix", "perceptual", (8, 15)), ("lab_extremes", "perceptual", (8, 15))})

# 12 calls of the reference's schedule at 2 x 3 from the hand_tiles state, 8 random candidates a call, stream seed
# TRAJECTORY_SEED: calls of the 12 the oracle accepts (chosen on the CPU among seeds 1..8 so that every image but
# two_tone has accepted and rejected calls under every flag set)
TRAJECTORY_SEED = 4
ACCEPTED = {("pixel_art", "rgb"): 8, ("pixel_art", "dither"): 6, ("pixel_art", "perceptual"): 5,
            ("alpha_mix", "rgb"): 2, ("alpha_mix", "dither"): 2, ("alpha_mix", "perceptual"): 5,
            ("two_tone", "rgb"): 0, ("two_tone", "dither"): 2, ("two_tone", "perceptual"): 0,
            ("lab_extremes", "rgb"): 7, ("lab_extremes", "dither"): 8, ("lab_extremes", "perceptual"): 7}

# 40 calls of the reference's schedule at 4 x 7 from the hand_tiles state, 64 candidates a call, stream seed 3: calls the
# oracle accepts (counted on the CPU, about 15 s a row: too long for the suite, so the GPU test holds the product to them)
WINDOW_ACCEPTED = {("pixel_art", "rgb"): 31, ("pixel_art", "dither"): 29, ("alpha_mix", "rgb"): 21, ("alpha_mix", "dither"): 23,
                   ("two_tone", "rgb"): 7, ("two_tone", "dither"): 10, ("lab_extremes", "rgb"): 31, ("lab_extremes", "dither"): 34}

_cache = {}


def image(name, h=32):
    if (name, h) not in _cache:
        a = ALL_IMAGES[name](h)
        a.setflags(write=False)
        _cache[name, h] = a
    return _cache[name, h]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def oracle_hand(O, name, flagkey, count, size, h=32):
    """An oracle on `name` with hand_tiles and the palette recalculate_palettes makes of them (duplicates included)."""
    o = O.OracleImage(image(name, h), count, size, **FLAGSETS[flagkey])
    o.tile_palettes = hand_tiles(count)
    o.recalculate_palettes()
    return o


def product_like(S, o, name, flagkey, count, size, h=32):
    """A product context in the oracle's state, the map made by its own optimize()."""
    g = S.OptimizedImage(image(name, h), count, size, **FLAGSETS[flagkey])
    g.tile_palettes, g.palette = o.tile_palettes, o.palette
    g.optimize()
    return g


def oracle_outcome(O, name, flagkey, count, size):
    """'ok', or the initialiser that raised."""
    o = O.OracleImage(image(name), count, size, **FLAGSETS[flagkey])
    try:
        o.initialize_tiles()
    except RuntimeError:
        return "initialize_tiles"
    try:
        o.recalculate_palettes()
    except RuntimeError:
        return "recalculate_palettes"
    return "ok"


def pick_slots(pal, count, size):
    """-> [a slot whose entry is black and repeats a lower entry of its subpalette (a NaN centre; absent where k-means left
    none empty), a slot whose entry is the only one of its colour in its subpalette, (0, 0)], without repeats."""
    p = pal.reshape(count, size, 3)
    dup = uniq = None
    for sp in range(count - 1, -1, -1):
        for si in range(size):
            same = [bool((p[sp, j] == p[sp, si]).all()) for j in range(size)]
            if dup is None and si > 0 and not p[sp, si].any() and any(same[:si]):
                dup = (sp, si)
            if uniq is None and sum(same) == 1 and (sp, si) != (0, 0):
                uniq = (sp, si)
    return [s for s in (dup, uniq, (0, 0)) if s is not None]


def own_colours(img):
    """Up to 12 of the image's own opaque colours, spread over the sorted list, as 5-bit values."""
    u = np.unique(img[..., :3][img[..., 3] > 0], axis=0)
    return u[np.linspace(0, len(u) - 1, min(12, len(u))).astype(int)] >> 3


def duplicated_colour(pal, size, slot):
    """-> (colour, copies): the colour most of the slot's neighbours (the other entries of its subpalette) hold, the lowest
    entry first among equals, and how many of them hold it; copies == 1 where no two neighbours are equal."""
    sp, si = slot
    others = [pal[sp * size + j] for j in range(size) if j != si]
    copies = [sum(bool((a == b).all()) for b in others) for a in others]
    k = int(np.argmax(copies))
    return others[k], copies[k]


def candidate_list(S, img, pal, size, slot, n):
    """The incumbent, the colour its neighbours duplicate (held by two or more of them wherever the subpalette has
    duplicates: test_oracle_initialiser_outcomes), black, white, the component-32 quirk, the image's own colours, random
    colours."""
    sp, si = slot
    cand = S.random_candidates(29, sp * size + si, n)
    head = np.concatenate([[pal[sp * size + si], duplicated_colour(pal, size, slot)[0], [0, 0, 0], [31, 31, 31], [32, 5, 32]],
                           own_colours(img)]).astype(np.uint8)[:n]
    cand[:len(head)] = head
    return cand


# ---- CPU: the images and the premises of the GPU tests ---------------------------------------------------------------------

def test_images_are_pinned():
    for (name, h), want in SHA256.items():
        a = ALL_IMAGES[name](h)
        assert a.shape == (h, 256, 4) and a.dtype == np.uint8
        assert hashlib.sha256(a.tobytes()).hexdigest() == want, (name, h)
    for name in ("pixel_art", "two_tone", "lab_extremes"):
        assert (image(name)[..., 3] == 255).all()
    a = image("alpha_mix")
    assert set(np.unique(a[..., 3])) == {0, 1, 127, 128, 200, 254, 255}
    assert not a[0, :, 3].any() and not a[-1, :, 3].any() and not a[:, 0, 3].any() and not a[:, -1, 3].any()
    t11, t21 = a[8:16, 8:16, 3], a[8:16, 16:24, 3]
    assert np.count_nonzero(t11) == 1 and t11[0, 0] == 200 and np.count_nonzero(t21) == 1 and t21[7, 7] == 1
    assert not a[16:24, 64:128, 3].any()
    p = image("pixel_art")
    assert (p[:, 0:4] == p[0, 0]).all(axis=-1)[:8].all() and (p[:8, 4:8] == p[0, 4]).all()  # flat halves: equal leading points
    f = image("flat_tiles")
    assert not f[0:8, 24:32, :3].any() and (f[0:8, 40:48, :3] == (0, 0, 128)).all() and not f[24:32, 248:256, :3].any()
    assert [hand_tiles(4)[t] for t in (0, 1, 2, 31, 32, 1023)] == [0, 0, 1, 3, 1, 2]


def test_tile_mean_filter_is_reached(O):
    """The filter `sum[0] + sum[1] + sum[2] > 0.0f` of initialize_tiles drops an opaque all-black tile, and with Lab sums a
    dark-blue one as well (L + a + b < 0 for (0, 0, 128)): flat_tiles has both, far from the threshold."""
    lab = {rgb: O.srgb8_to_lab(rgb).astype(np.float64).sum() for rgb in ((0, 0, 0), (0, 0, 128), (0, 0, 40))}
    assert lab[0, 0, 0] == 0.0 and lab[0, 0, 128] < -1.0
    img = image("flat_tiles")
    colours = [tuple(int(v) for v in c) for c in np.unique(img[..., :3].reshape(-1, 3), axis=0)]
    weight = {False: {c: float(sum(c)) for c in colours},
              True: {c: float(O.srgb8_to_lab(c).astype(np.float64).sum()) for c in colours}}
    dropped = {}
    for perceptual in (False, True):
        dropped[perceptual] = []
        for t in range(128):
            ty, tx = divmod(t, 32)
            s = sum(weight[perceptual][tuple(int(v) for v in c)] for c in img[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8, :3].reshape(-1, 3))
            assert s == 0.0 or abs(s) > 1.0, (tx, ty, s)  # float32 summation cannot change the side
            if not s > 0.0:
                dropped[perceptual].append(t)
    assert dropped[False] == [3, 127] and {3, 5, 127} <= set(dropped[True]), dropped


def test_oracle_initialiser_outcomes(O):
    """Where the initialisers succeed and where recalculate_palettes fails its precondition: both occur, at the places the
    GPU tests were designed around; from hand_tiles recalculate_palettes always succeeds, and on pixel_art it leaves NaN
    centres, which become black entries."""
    table = {(name, fk, geo): oracle_outcome(O, name, fk, *geo) for name in NAMES for fk in ("rgb", "perceptual") for geo in GEOMETRIES}
    assert "initialize_tiles" not in table.values()
    assert {k for k, v in table.items() if v == "recalculate_palettes"} == RAISES
    assert 0 < len(RAISES) < len(table)
    for fk in ("rgb", "perceptual"):
        for geo in GEOMETRIES:
            assert oracle_outcome(O, "flat_tiles", fk, *geo) != "initialize_tiles"
    for name in NAMES:
        for fk in ("rgb", "perceptual"):
            for count, size in GEOMETRIES:
                o = oracle_hand(O, name, fk, count, size)  # raises if the precondition fails
                e = o.error()
                assert 30.0 < e < 500.0, (name, fk, count, size, e)  # far from 0: relative comparisons are well conditioned
                if (name, count, size) == ("pixel_art", 4, 7):
                    assert int((o.palette == 0).all(axis=1).sum()) >= 20
                    assert len(pick_slots(o.palette, count, size)) == 3
    for name in ("pixel_art", "two_tone", "lab_extremes"):
        for fk in ("rgb", "perceptual"):
            pal = oracle_hand(O, name, fk, 4, 7).palette
            slots = pick_slots(pal, 4, 7)
            (sp, si), (up, ui) = slots[:2]
            assert not pal[sp * 7 + si].any() and si > 0 and (up, ui) != (sp, si)
            for slot in slots:  # the second candidate of every list is a colour two or more neighbours of the slot hold
                colour, copies = duplicated_colour(pal, 7, slot)
                assert copies >= 2 and not colour.any(), (name, fk, slot)


def test_oracle_trajectories_accept_and_reject(O):
    """The 12-call trajectories the GPU is held to contain accepted and rejected calls on every image but two_tone, whose
    RGB run rejects everything.  The RGB rows here; the GPU test asserts every row of ACCEPTED on the oracle it runs."""
    sched = O.schedule(2, 3, 12)
    for (name, fk), want in ACCEPTED.items():
        if fk != "rgb":
            assert name == "two_tone" or 1 <= want <= 11
            continue
        o = oracle_hand(O, name, fk, 2, 3)
        got = 0
        for j, (m, p, i, ch, _) in enumerate(sched):
            before = o.palette
            o.step(m, p, i, ch, TRAJECTORY_SEED, j, 8 if m == 0 else 0)
            got += not np.array_equal(before, o.palette)
        assert got == want, (name, fk, got)
        assert name == "two_tone" or 1 <= got <= 11
    assert ACCEPTED["two_tone", "rgb"] == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def assert_same_state(g, o, what=None):
    assert np.array_equal(g.tile_palettes, o.tile_palettes), what
    assert np.array_equal(g.palette, o.palette), what
    assert np.array_equal(g.palette_map, o.palette_map), what


def assert_same_outputs(g, o, what=None):
    assert_same_state(g, o, what)
    assert g.as_json() == o.as_json(), what
    assert np.array_equal(g.as_rgba(), o.as_rgba()), what
    assert np.array_equal(g.palette_u16, o.palette_u16), what
    assert rel(g.error(), o.error()) < REL_ERR, what


# a. initialisers
INIT_CASES = [(name, fk, geo, False) for name in NAMES + ["flat_tiles"] for fk in ("rgb", "perceptual") for geo in GEOMETRIES] + \
             [("pixel_art", "rgb", (2, 3), True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,flagkey,geo,nes", INIT_CASES, ids=lambda v: v if isinstance(v, str) else ("%dx%d" % v if isinstance(v, tuple) else ("nes" if v else "snes")))
def test_initialisers_match_oracle_and_fail_where_it_fails(S, O, name, flagkey, geo, nes):
    """initialize_tiles against the oracle (flat tiles: equal tile means, empty clusters; dropped tiles keep subpalette 0);
    recalculate_palettes raises -4 exactly where the oracle raises, else equal outputs (NaN centres as black entries);
    after a raise the same context takes hand_tiles and recalculates as the oracle does."""
    count, size = geo
    flags = dict(FLAGSETS[flagkey], nes=nes)
    img = image(name)
    g, o = S.OptimizedImage(img, count, size, **flags), O.OracleImage(img, count, size, **flags)
    g.initialize_tiles()
    o.initialize_tiles()  # succeeds on every case (test_oracle_initialiser_outcomes)
    assert_same_state(g, o, "initialize_tiles")
    try:
        o.recalculate_palettes()
        raised = False
    except RuntimeError:
        raised = True
    if not nes and name in NAMES:
        assert raised == ((name, flagkey, geo) in RAISES)
    if raised:
        with pytest.raises(S.SnesImageError) as e:
            g.recalculate_palettes()
        assert e.value.code == -4
    else:
        g.recalculate_palettes()
        assert_same_outputs(g, o, "recalculate_palettes")
    o = O.OracleImage(img, count, size, **flags)
    for x in (g, o):
        x.tile_palettes = hand_tiles(count)
        x.recalculate_palettes()
    assert_same_outputs(g, o, "hand_tiles")
    g.close()


# b. remap
@pytest.mark.gpu
@pytest.mark.parametrize("flagkey", list(FLAGSETS))
@pytest.mark.parametrize("name", NAMES)
def test_remap_of_duplicate_filled_palettes(S, O, name, flagkey):
    """optimize() on palettes full of duplicate entries (every tie goes to the lowest index), partial alpha, transparent
    borders and, with dither, the clamp of the diffused target on every pixel of the checkerboard."""
    for count, size in GEOMETRIES:
        o = oracle_hand(O, name, flagkey, count, size)
        g = product_like(S, o, name, flagkey, count, size)
        assert np.array_equal(g.palette_map, o.palette_map), (count, size)
        assert rel(g.error(), o.error()) < REL_ERR
        g.optimize()
        assert np.array_equal(g.palette_map, o.palette_map), (count, size)
        assert np.array_equal(g.as_rgba(), o.as_rgba())
        g.close()


# c. candidate scoring, dense and sparse
SCORE_CASES = [(name, fk, 32) for name in NAMES for fk in FLAGSETS] + [("lab_extremes", "perceptual", 64), ("pixel_art", "dither", 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,flagkey,h", SCORE_CASES)
def test_candidate_scoring_dense_sparse_and_oracle(S, O, name, flagkey, h, monkeypatch):
    """150 candidates on a NaN-black duplicate slot, a unique slot and (0, 0): the group-sparse path equals the dense path bit
    for bit (lists full of candidates that change nothing: their error is the incumbent's, bit for bit); the first 8 —
    incumbent, neighbour, black, white, the component-32 quirk, the image's own colours — against the oracle with maps."""
    from hipmem import DeviceArray
    count, size, n, no = 4, 7, 150, 8
    img = image(name, h)
    o = oracle_hand(O, name, flagkey, count, size, h)
    monkeypatch.setenv("SNES_SPARSE", "0")
    dense = product_like(S, o, name, flagkey, count, size, h)
    monkeypatch.setenv("SNES_SPARSE", "1")
    monkeypatch.setenv("SNES_SPARSE_MIN", "1")
    g = product_like(S, o, name, flagkey, count, size, h)
    assert np.array_equal(g.palette_map, o.palette_map) and np.array_equal(dense.palette_map, o.palette_map)
    pal = o.palette
    slots = pick_slots(pal, count, size)
    assert len(slots) == 3 or name == "alpha_mix"  # (its subpalettes have no empty cluster)
    inc = g.error()
    for sp, si in slots:
        cand = candidate_list(S, img, pal, size, (sp, si), n)
        ed, es = dense.score_candidates(sp, si, cand), g.score_candidates(sp, si, cand)
        assert np.array_equal(ed, es), (sp, si, int(np.argmax(ed != es)), float(np.max(np.abs(ed - es))))
        eo, mo = o.score_candidates(sp, si, cand[:no], want_maps=True)
        d_c = DeviceArray.from_numpy(cand[:no])
        d_e = DeviceArray(no, np.float64, fill=0)
        d_m = DeviceArray((no, h, 256), np.uint8, fill=0)
        g.score_candidates_device(sp, si, d_c.ptr, no, d_e.ptr, d_m.ptr)
        g.sync()
        maps, errors = d_m.numpy(), d_e.numpy()
        for k in range(no):
            assert np.array_equal(maps[k], mo[k]), (sp, si, k, cand[k].tolist())
        assert rel(errors, eo) < REL_ERR, (sp, si)
        assert rel(es[:no], eo) < REL_ERR, (sp, si)
        assert rel(errors[0], g.error()) == 0.0 and rel(eo[0], o.error()) == 0.0
        same = np.nonzero(eo == eo[0])[0]  # what the oracle scores exactly as the incumbent, the product must too (strict <)
        assert (errors[same] == errors[0]).all() and (es[same] == es[0]).all(), (sp, si, same)
    assert g.error() == inc and np.array_equal(g.palette, pal) and np.array_equal(g.palette_map, o.palette_map)  # state untouched
    dense.close()
    g.close()


# d. perceptual remap alone
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lab_extremes", "pixel_art"])
def test_perceptual_remap_alone_equals_the_scoring_path_maps(S, O, name):
    """remap_candidates_device (win tests over the contested pixels only, most ruled out by the two sure "no"s) against the
    maps of score_candidates_device (every pixel searched) for 300 candidates on neutrals, blue-violets and near-blacks."""
    from hipmem import DeviceArray
    count, size, n, h = 4, 7, 300, 32
    o = oracle_hand(O, name, "perceptual", count, size)
    g = product_like(S, o, name, "perceptual", count, size)
    for sp, si in pick_slots(o.palette, count, size):
        cand = candidate_list(S, image(name), o.palette, size, (sp, si), n)
        d_c = DeviceArray.from_numpy(cand)
        d_e = DeviceArray(n, np.float64, fill=0)
        d_m = DeviceArray((n, h, 256), np.uint8, fill=0)
        d_r = DeviceArray((n, h, 256), np.uint8, fill=7)
        g.score_candidates_device(sp, si, d_c.ptr, n, d_e.ptr, d_m.ptr)
        g.remap_candidates_device(sp, si, d_c.ptr, n, d_r.ptr)
        g.sync()
        a, b = d_m.numpy(), d_r.numpy()
        assert np.array_equal(a, b), ((sp, si), int(np.argmax((a != b).reshape(n, -1).any(axis=1))))
        _, mo = o.score_candidates(sp, si, cand[:8], want_maps=True)
        assert np.array_equal(b[:8], mo)
    g.close()


# e. trajectories
@pytest.mark.gpu
@pytest.mark.parametrize("flagkey", ["rgb", "dither", "perceptual"])
@pytest.mark.parametrize("name", NAMES)
def test_trajectory_matches_oracle_step_by_step(S, O, name, flagkey):
    """12 calls of the reference's schedule, 8 random candidates each, against the oracle call by call: accepted and
    rejected calls on every image (test_oracle_trajectories_accept_and_reject); two_tone with RGB rejects all 12."""
    count, size = 2, 3
    o = oracle_hand(O, name, flagkey, count, size)
    g = product_like(S, o, name, flagkey, count, size)
    pal0 = o.palette
    accepted = 0
    for j, (m, p, i, ch, _) in enumerate(S.schedule(count, size, 12)):
        before = o.palette
        eo, bo = o.step(m, p, i, ch, TRAJECTORY_SEED, j, 8 if m == S.METHOD_RANDOM else 0)
        eg, bg = g.step(m, p, i, ch, TRAJECTORY_SEED, j, 8 if m == S.METHOD_RANDOM else 0)
        assert np.array_equal(bg, bo), (j, bg.tolist(), bo.tolist(), eg, eo)
        assert rel(eg, eo) < REL_ERR, (j, eg, eo)
        assert np.array_equal(g.palette, o.palette) and np.array_equal(g.palette_map, o.palette_map), j
        accepted += not np.array_equal(before, o.palette)
    assert accepted == ACCEPTED[name, flagkey]
    if ACCEPTED[name, flagkey] == 0:
        assert np.array_equal(g.palette, pal0)
    assert g.as_json() == o.as_json()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flagkey", ["rgb", "dither"])
@pytest.mark.parametrize("name", NAMES)
def test_slot_windows_equal_call_by_call_and_sparse_equals_dense(S, O, name, flagkey, monkeypatch):
    """40 scheduled calls of 64 candidates: run_slots with windows 0 (adaptive) and 7 on the group-sparse path against
    step() one by one on the dense path, bit for bit.  The calls the oracle accepts from the same state (WINDOW_ACCEPTED,
    counted on the CPU) are what the product must accept: on two_tone most windows of 7 go through whole, on pixel_art
    and lab_extremes three calls of four are accepted and the rest of their windows is thrown away."""
    count, size, calls, seed = 4, 7, 40, 3
    o = oracle_hand(O, name, flagkey, count, size)
    monkeypatch.setenv("SNES_SPARSE", "0")
    dense = product_like(S, o, name, flagkey, count, size)
    monkeypatch.setenv("SNES_SPARSE", "1")
    monkeypatch.setenv("SNES_SPARSE_MIN", "1")
    sched = S.schedule(count, size, calls)
    logs = []
    for window in (0, 7):
        w = product_like(S, o, name, flagkey, count, size)
        log, _, stats = w.run_slots(calls, seed=seed, first_step_id=0, state=sched[0][1:], window=window)
        assert stats["calls"] == calls
        assert stats["accepted"] == sum(r[3] for r in log) == WINDOW_ACCEPTED[name, flagkey], (window, stats)
        if window == 7 and name == "two_tone":
            assert stats["windows"] < calls, stats           # windows that take several rejected calls at once
        if window == 7 and name in ("pixel_art", "lab_extremes"):
            assert stats["scored"] > stats["useful"], stats  # calls scored behind an accepted one, then void
        logs.append((window, log, w))
    for j, (m, p, i, ch, _) in enumerate(sched):
        e, b = dense.step(m, p, i, ch, seed, j, 0)
        for window, log, _ in logs:
            assert (e, b.tolist()) == (log[j][0], log[j][2].tolist()), (window, j)
    for window, _, w in logs:
        assert np.array_equal(dense.palette, w.palette) and np.array_equal(dense.palette_map, w.palette_map), window
        assert dense.error() == w.error()
        w.close()
    dense.close()


# f. tiles
@pytest.mark.gpu
@pytest.mark.parametrize("flagkey", ["rgb", "perceptual"])
@pytest.mark.parametrize("name", ["pixel_art", "alpha_mix"])
def test_reassign_tiles_matches_oracle(S, O, name, flagkey):
    """Identical subpalettes (their costs tie: the lowest index wins), tiles with a single opaque pixel, transparent tiles."""
    count, size = 4, 7
    o = oracle_hand(O, name, flagkey, count, size)
    g = product_like(S, o, name, flagkey, count, size)
    for rnd in range(2):
        mg, mo = g.reassign_tiles(), o.reassign_tiles()
        assert mg == mo and (mo > 0) == (rnd == 0)
        assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, o.palette_map)
        assert rel(g.error(), o.error()) < REL_ERR
    assert g.as_json() == o.as_json()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pixel_art", "alpha_mix"])
def test_tile_sweep_matches_the_model(S, O, name):
    """One sweep of objective-scored tile moves over tiles 32..79 (on alpha_mix: the two single-pixel tiles 33 and 34 and the
    transparent tiles 72..79) against tests/tile_model.py over the oracle; moves to an identical subpalette are never taken."""
    count, size, first, n = 4, 7, 32, 48
    o = oracle_hand(O, name, "rgb", count, size)
    g = product_like(S, o, name, "rgb", count, size)
    want = model_tile_sweep(o, first, n, count)
    accepted = sum(ch for _, _, ch in want)
    assert 3 <= accepted <= n - 3
    log, stats = g.tile_sweep(first, n)
    assert_log_matches(log, want)
    assert stats["calls"] == n and stats["accepted"] == accepted
    assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, o.palette_map)
    assert rel(g.error(), o.error()) < REL_ERR and g.as_json() == o.as_json()
    g.close()


# g. the two sure "no"s of CIEDE2000, directly
@pytest.mark.gpu
def test_sure_noes_never_fire_at_a_pairs_own_distance(S):
    """color.hpp's ciede2000_cannot_beat and ciede2000_cannot_beat_ab (debug ops 7 and 8) with the bound set to the pair's own
    distance, the tie that still wins; both are monotone in the bound, so a 0 here covers every larger bound.  All 32,768
    BGR555 candidates against 201 targets: neutrals (the zero-chroma branch), the blue-violet ramp (hues around 275 degrees,
    where R_T is largest), near-blacks and random colours."""
    v = np.arange(32)
    e8 = (v * 8 + v // 4).astype(np.float32)
    r, gg, b = np.meshgrid(e8, e8, e8, indexing="ij")
    cand_rgb = np.stack([r, gg, b], axis=-1).reshape(-1, 3)
    x = np.append(np.arange(0, 256, 8), 255)
    dark = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), axis=-1).reshape(-1, 3)[::50]
    rng = np.random.default_rng(17)
    tgt_rgb = np.concatenate([np.stack([x, x, x], 1), np.stack([x, x // 2, np.full_like(x, 255)], 1), dark,
                              rng.integers(0, 256, (100, 3))]).astype(np.float32)
    assert len(cand_rgb) == 32768 and len(tgt_rgb) == 33 + 33 + 35 + 100
    cand = S.debug_math(6, cand_rgb).reshape(-1, 3)
    tgt = S.debug_math(6, tgt_rgb).reshape(-1, 3)
    assert np.isfinite(cand).all() and np.isfinite(tgt).all()
    step = 16
    for t0 in range(0, len(tgt), step):
        t = tgt[t0:t0 + step]
        xs = np.tile(cand, (len(t), 1))
        ys = np.repeat(t, len(cand), axis=0)
        for op in (7, 8):
            out = S.debug_math(op, xs, ys)
            assert out.shape == (len(xs),)
            bad = np.nonzero(out != 0.0)[0]
            assert bad.size == 0, (op, bad.size, cand_rgb[bad[0] % len(cand)].tolist(), tgt_rgb[t0 + bad[0] // len(cand)].tolist())
