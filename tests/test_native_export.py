"""The native export on the GPU (include/snesimage_hip.h: "Native export"): CGRAM, CHR and MAP byte for byte against the numpy
model (native_model.py) fed from the same context, the renderer against the model's decode and against as_rgba(), the state
left untouched, the refusals, sets, and the CLI's files.  Every comparison is exact.  All cases run at 256 x 8 or 256 x 16, the
smallest shapes with one and two tile rows (a vertical flip needs two)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import character_model as M
import native_model as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def image(h, seed):
    from snesimage_amd.synth import synth_image
    return synth_image(0x5EED0E10 + seed, 256, h)


def started(S, img, count, size, **flags):
    g = S.OptimizedImage(img, count, size, **flags)
    g.initialize_tiles()
    g.recalculate_palettes()
    return g


def model_of(g, **lay):
    """The model's encoding of the context's own characters(), tile_palettes, palette_u16 and backdrop."""
    u, rep, flip, chars = g.characters()
    ntile = 32 * (g.h // 8)
    pal = g.palette_u16.reshape(g.sub_count, g.sub_size)
    return N.encode(chars, rep, flip, g.tile_palettes[:ntile], pal, g.backdrop if g.has_backdrop else None, N.layout(**lay)) + (u, flip)


def assert_renders_as(g, ex, want_rgba, lay):
    """render_native of exported bytes: the model's decode; as_rgba() where the source is opaque, CGRAM word 0 elsewhere."""
    lay = dict(lay, bpp=ex["bpp"])
    drawn = g.render_native(ex["cgram"], ex["chr"], ex["map"], **lay)
    assert np.array_equal(drawn, N.decode(ex["cgram"], ex["chr"], ex["map"], N.layout(**lay), g.h))
    opaque = want_rgba[..., 3] != 0
    assert np.array_equal(drawn[opaque][:, :3], want_rgba[opaque][:, :3])
    assert (drawn[~opaque][:, :3] == N.rgb_of_word(np.frombuffer(ex["cgram"], "<u2")[0])).all()
    assert (drawn[..., 3] == 255).all()


def check_export(g, **lay):
    cgram, chr_, words, bpp, u, flip = model_of(g, **lay)
    ex = g.export_native(**lay)
    assert ex["bpp"] == bpp and ex["unique"] == u
    assert ex["cgram"] == cgram
    assert ex["chr"] == chr_
    assert ex["map"].dtype == np.uint16 and np.array_equal(ex["map"], words)
    assert_renders_as(g, ex, g.as_rgba(), lay)
    return ex, flip


# ---- bytes against the model, and the renderer -------------------------------------------------------------------------------

@pytest.mark.parametrize("name,h,count,size,flags,lay,bpp", [
    ("2x3", 16, 2, 3, {}, {}, 2),
    ("2x3_bpp4", 16, 2, 3, {}, dict(bpp=4), 4),
    ("8x15", 16, 8, 15, {}, dict(char_base=0x100, palette_base=0, priority=1), 4),
    ("1x20", 8, 1, 20, {}, {}, 8),
    ("2x3_backdrop", 16, 2, 3, dict(backdrop=True), {}, 2),
    ("2x3_backdrop_based", 16, 2, 3, dict(backdrop=True), dict(bpp=4, palette_base=6, char_base=960), 4),
    ("dither", 16, 2, 3, dict(dither=True), {}, 2),
])
def test_export_is_the_models_encoding(S, name, h, count, size, flags, lay, bpp):
    g = started(S, image(h, len(name)), count, size, **flags)
    ex, _ = check_export(g, **lay)
    assert ex["bpp"] == bpp and len(ex["chr"]) == ex["unique"] * 8 * bpp and ex["map"].shape == (32 * (h // 8),)
    if flags.get("backdrop"):
        assert any(0 in g.characters()[3][t] for t in range(32)), "the input breaks the premise: no pixel takes the backdrop colour"
    if bpp == 4 and not lay.get("palette_base"):  # CGRAM is the JSON's palette rows, zero-padded
        rows = json.loads(g.as_json())["palette"]
        cg = np.frombuffer(ex["cgram"], "<u2")
        assert cg[:len(rows)].tolist() == rows and not cg[len(rows):].any()
    g.close()


def test_export_with_a_pinned_and_a_fully_transparent_tile(S):
    img = N.transparent_block_image()
    g = started(S, img, 2, 3)
    chars = g.characters()[3]
    assert not chars[11].any() and (chars[10] == 0).any() and chars[10].any()
    check_export(g)
    check_export(g, bpp=4, palette_base=3, char_base=5)
    g.close()


def test_export_of_the_mirrored_image_carries_all_four_flips(S):
    g = N.mirrored_state(S.OptimizedImage(N.mirrored_image(), *N.MIRROR_GEOMETRY))
    ex, flip = check_export(g)
    assert sorted(set(flip.tolist())) == [0, 1, 2, 3]  # a condition on the input (test_native_model.py shows it on the oracle)
    assert sorted(set((ex["map"] >> 14).tolist())) == [0, 1, 2, 3]
    assert ex["unique"] == M.classes(g.characters()[3][:16])[2]
    g.close()


def test_export_after_a_character_reduction(S):
    g = started(S, image(16, 40), 2, 3)
    U0 = g.characters()[0]
    _, U1 = g.reduce_characters(U0 - 4, 4)
    assert U1 == U0 - 4
    ex, _ = check_export(g, char_base=1024 - U1)
    assert ex["unique"] == U1 and int((ex["map"] & 1023).max()) == 1023
    g.close()


# ---- state ---------------------------------------------------------------------------------------------------------------

def test_export_leaves_the_state_bit_identical(S):
    g = started(S, image(16, 50), 2, 3)
    before = (g.error(), g.palette_map.tobytes(), g.as_json(), [np.asarray(a).tobytes() if i else a for i, a in enumerate(g.characters())])
    g.export_native()
    g.export_native(bpp=4, char_base=3, palette_base=1, priority=1)
    after = (g.error(), g.palette_map.tobytes(), g.as_json(), [np.asarray(a).tobytes() if i else a for i, a in enumerate(g.characters())])
    assert before == after
    g.close()


def test_export_behind_a_step_runs_the_owed_optimize(S):
    """An export right after a step() that left the map pending equals the export after an explicit optimize()."""
    img = image(16, 51)
    a, b = started(S, img, 2, 3), started(S, img, 2, 3)
    pal0 = a.palette.copy()
    for j, (method, p, i, ch, _) in enumerate(S.schedule(2, 3, 3)):
        ea, _ = a.step(method, p, i, ch, 1, j)
        eb, _ = b.step(method, p, i, ch, 1, j)
        assert ea == eb
    assert not np.array_equal(a.palette, pal0), "the input breaks the premise: no call changed the palette"
    b.optimize()
    ex_a, ex_b = a.export_native(), b.export_native()
    assert ex_a["cgram"] == ex_b["cgram"] and ex_a["chr"] == ex_b["chr"] and np.array_equal(ex_a["map"], ex_b["map"])
    assert np.array_equal(a.palette_map, b.palette_map) and a.error() == b.error()
    check_export(a)
    a.close()
    b.close()


def test_sizes_only_call(S):
    from snesimage_amd import _ffi
    g = started(S, image(16, 52), 2, 3)
    for bpp in (0, 2, 4):
        lay, info = _ffi.NativeLayout(bpp, 0, 0, 0, 0, 0), _ffi.NativeInfo()
        assert g._L.snesimage_export_native(g._c, C.byref(lay), None, None, 0, None, C.byref(info)) == 0
        assert info.bpp == (bpp or 2) and info.unique == g.characters()[0]
        assert info.chr_bytes == info.unique * 8 * info.bpp and info.map_words == 64
    info = _ffi.NativeInfo()
    assert g._L.snesimage_export_native(g._c, None, None, None, 0, None, C.byref(info)) == 0 and info.bpp == 2  # a null layout: all zero
    g.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------

def refused(S, call, code):
    with pytest.raises(S.SnesImageError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals_leave_the_context_usable(S):
    from snesimage_amd import _ffi
    g15 = started(S, image(16, 60), 2, 15)
    refused(S, lambda: g15.export_native(bpp=2), ERR_ARG)  # S = 15 does not fit 2bpp
    check_export(g15)
    g15.close()
    g = started(S, image(16, 61), 2, 3)
    assert "2 subpalettes" in refused(S, lambda: g.export_native(bpp=8), ERR_UNSUPPORTED)  # the message names the geometry
    refused(S, lambda: g.export_native(palette_base=7), ERR_ARG)  # 7 + 2 > 8
    U = g.characters()[0]
    assert U >= 2
    msg = refused(S, lambda: g.export_native(char_base=1023), ERR_ARG)
    assert "U = %d" % U in msg and "snesimage_reduce_characters" in msg
    refused(S, lambda: g.export_native(bpp=3), ERR_ARG)
    refused(S, lambda: g.export_native(priority=2), ERR_ARG)
    refused(S, lambda: g.export_native(char_base=1024), ERR_ARG)
    ex, _ = check_export(g)
    # chr_cap too small
    lay, info = _ffi.NativeLayout(), _ffi.NativeInfo()
    small = np.zeros(len(ex["chr"]) - 1, np.uint8)
    assert g._L.snesimage_export_native(g._c, C.byref(lay), None, small.ctypes.data_as(_ffi._u8p), small.size, None, C.byref(info)) == ERR_ARG
    assert not small.any()
    # a map word pointing past chr, and one below char_base: refused before anything is launched
    words = ex["map"].copy()
    words[5] = (words[5] & ~np.uint16(1023)) | np.uint16(ex["unique"])
    refused(S, lambda: g.render_native(ex["cgram"], ex["chr"], words, bpp=2), ERR_ARG)
    refused(S, lambda: g.render_native(ex["cgram"], ex["chr"], ex["map"], bpp=2, char_base=1), ERR_ARG)
    refused(S, lambda: g.render_native(ex["cgram"], ex["chr"][:-1], ex["map"], bpp=2), ERR_ARG)
    check_export(g)
    # a context lent to a set
    other = started(S, image(16, 61), 2, 3)
    sp = S.SharedPalette([g, other])
    refused(S, lambda: g.export_native(), ERR_STATE)
    assert sp.export_native()["unique"] == U  # two equal frames: the set's characters are frame 0's
    sp.close()
    check_export(g)
    g.close()
    other.close()


# ---- sets ------------------------------------------------------------------------------------------------------------------

def test_set_export_one_chr_and_a_map_per_member(S):
    """Two frames of 256 x 8, frame 1 the horizontal mirror of frame 0 with mirrored tile_palettes: one CHR serves both."""
    f0 = image(8, 70)
    f1 = np.ascontiguousarray(f0[:, ::-1])
    tp0 = np.zeros(1024, np.uint8)
    tp0[:32] = (np.arange(32) // 3) % 2
    tp1 = tp0.copy()
    tp1[:32] = tp0[:32][::-1]
    ctxs = [S.OptimizedImage(f, *N.MIRROR_GEOMETRY) for f in (f0, f1)]
    for c, tp in zip(ctxs, (tp0, tp1)):
        c.set_chunk(64)
        c.tile_palettes = tp
        c.palette = N.MIRROR_PALETTE
        c.optimize()
    own_U = ctxs[0].characters()[0]
    sp = S.SharedPalette(ctxs)
    u, rep, flip, chars = sp.characters()
    assert u == own_U, "the input breaks the premise: the mirrored frame adds characters"
    for lay in ({}, dict(bpp=4, char_base=100, palette_base=2, priority=1)):
        ex = sp.export_native(**lay)
        tps = np.concatenate([c.tile_palettes[:32] for c in ctxs])
        cgram, chr_, words, bpp = N.encode(chars, rep, flip, tps, ctxs[0].palette_u16.reshape(*N.MIRROR_GEOMETRY), None, N.layout(**lay))
        assert ex["bpp"] == bpp and ex["unique"] == u
        assert ex["cgram"] == cgram and ex["chr"] == chr_ and ex["map"].shape == (2, 32) and np.array_equal(ex["map"].reshape(-1), words)
        assert ((ex["map"][1] >> 14) & 1).any()  # the mirrored frame draws frame 0's characters flipped
        for m, c in enumerate(ctxs):  # each member's map, rendered with that member's context
            assert_renders_as(c, dict(ex, map=ex["map"][m]), c.as_rgba(), lay)
    e0 = sp.error()
    sp.export_native()
    assert sp.error() == e0
    sp.close()
    for c in ctxs:
        c.close()


def test_backdrop_set_is_refused_by_name_and_still_steps(S):
    ctxs = [S.OptimizedImage(image(8, 71 + i), 2, 3, backdrop=True) for i in range(2)]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs, backdrop=True)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    assert "snesimage_shared_export_native" in refused(S, lambda: sp.export_native(), ERR_UNSUPPORTED)
    e, _ = sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 8)
    assert np.isfinite(e) and e > 0
    sp.close()
    for c in ctxs:
        c.close()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------

def pieces_of_json(js, tm, frames):
    """What encode is fed, from the run's own JSON(s) and tilemap JSON: the tiles the tilemap stands for, classed anew."""
    if frames == 1:
        tm = dict(tm, character=[tm["character"]], hflip=[tm["hflip"]], vflip=[tm["vflip"]], palette=[tm["palette"]])
    ch = np.array(tm["characters"], np.uint8)
    chars = np.concatenate([np.array([M.flip_char(ch[c], hf + 2 * vf) for c, hf, vf in zip(tm["character"][m], tm["hflip"][m], tm["vflip"][m])], np.uint8) for m in range(frames)])
    rep, flip, U, _ = M.classes(chars)
    assert U == len(ch)
    return chars, rep, flip, np.concatenate([np.array(tm["palette"][m], np.uint8) for m in range(frames)])


def test_cli_writes_the_models_encoding_of_its_own_json(tmp_path):
    raw, raw2 = str(tmp_path / "a.rgba"), str(tmp_path / "b.rgba")
    image(16, 80).tofile(raw)
    image(16, 81).tofile(raw2)
    p = lambda n: str(tmp_path / n)
    common = ["-c", "2", "-s", "3", "--calls", "4", "--candidates", "16"]
    r = cli(raw, p("one.json"), *common, "--tilemap", p("one_tm.json"), "--export-cgram", p("one.cgram"), "--export-chr", p("one.chr"), "--export-map", p("one.map"))
    assert r.returncode == 0 and "Wrote native data" in r.stdout, r.stdout + r.stderr
    js, tm = json.load(open(p("one.json"))), json.load(open(p("one_tm.json")))
    pal = np.array(js["palette"], np.uint16).reshape(2, 16)[:, 1:4]
    chars, rep, flip, tps = pieces_of_json(js, tm, 1)
    assert chars.tolist() == js["tiles"]
    cgram, chr_, words, bpp = N.encode(chars, rep, flip, tps, pal, None, N.layout())
    assert bpp == 2 and open(p("one.cgram"), "rb").read() == cgram and open(p("one.chr"), "rb").read() == chr_
    assert open(p("one.map"), "rb").read() == words.astype("<u2").tobytes()
    # any subset, and a layout
    r = cli(raw, p("two.json"), *common, "--export-map", p("two.map"), "--export-bpp", "4", "--export-char-base", "512", "--export-palette-base", "6", "--export-priority", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    lay = N.layout(4, 512, 6, 1)
    assert open(p("two.map"), "rb").read() == N.encode(chars, rep, flip, tps, pal, None, lay)[2].astype("<u2").tobytes()
    assert open(p("two.json"), "rb").read() == open(p("one.json"), "rb").read() and not os.path.exists(p("two.chr"))
    # a state that cannot be exported: exit 1 with the library's message, nothing written
    r = cli(raw, p("three.json"), *common, "--export-chr", p("three.chr"), "--export-char-base", "1023")
    assert r.returncode == 1 and "char_base + U" in r.stdout and not os.path.exists(p("three.chr")), r.stdout + r.stderr
    # the same with --share and the set trio
    r = cli(raw, p("s0.json"), *common, "--share", raw2 + "=" + p("s1.json"), "--set-tilemap", p("set_tm.json"), "--set-export-cgram", p("set.cgram"), "--set-export-chr", p("set.chr"),
            "--set-export-map", p("set.map"))
    assert r.returncode == 0 and "Wrote native data of the set" in r.stdout, r.stdout + r.stderr
    js0, js1, stm = json.load(open(p("s0.json"))), json.load(open(p("s1.json"))), json.load(open(p("set_tm.json")))
    assert js0["palette"] == js1["palette"]
    pal = np.array(js0["palette"], np.uint16).reshape(2, 16)[:, 1:4]
    chars, rep, flip, tps = pieces_of_json(js0, stm, 2)
    assert chars.tolist() == js0["tiles"] + js1["tiles"]
    cgram, chr_, words, bpp = N.encode(chars, rep, flip, tps, pal, None, N.layout())
    assert open(p("set.cgram"), "rb").read() == cgram and open(p("set.chr"), "rb").read() == chr_
    assert len(words) == 128 and open(p("set.map"), "rb").read() == words.astype("<u2").tobytes()  # the members' maps one after another
