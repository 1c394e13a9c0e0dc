"""The native import on the GPU (include/snesimage_hip.h: "Native import"): an import is the four setters in one step, fed by the
numpy model's parse (native_import_model.py) of the same bytes; a reduced map survives export and import; foreign bytes load to
the state the model reads from them; refusals name the lowest tile and change nothing; sets; the CLI.  Every comparison is exact.
All cases run at 256 x 8 or 256 x 16, the smallest shapes with one and two tile rows (a vertical flip needs two)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import native_import_cases as K
import native_import_model as I
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
    return synth_image(0x5EED0F10 + seed, 256, h)


def started(S, img, count, size, **flags):
    g = S.OptimizedImage(img, count, size, **flags)
    g.initialize_tiles()
    g.recalculate_palettes()
    return g


def refused(S, call, code):
    with pytest.raises(S.SnesImageError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def observe(g, img):
    """Everything the contract lists, as comparable values."""
    opaque = img[..., 3] != 0
    nt = 32 * (g.h // 8)
    u, rep, flip, chars = g.characters()
    return dict(palette=g.palette.tobytes(), backdrop=g.backdrop.tobytes() if g.has_backdrop else None, tp=g.tile_palettes[:nt].tobytes(), map=g.palette_map[opaque].tobytes(),
                error=g.error(), rgba=g.as_rgba().tobytes(), json=g.as_json(), chars=(u, rep.tobytes(), flip.tobytes(), chars.tobytes()))


def by_hand(g, state):
    """parse()'s state through the four setters."""
    pal, b, tps, pm = state
    g.palette = pal
    if b is not None:
        g.backdrop = b
    tp = g.tile_palettes
    tp[:len(tps)] = tps
    g.tile_palettes = tp
    g.palette_map = pm
    return g


def slots(g, n=4):
    log, state, _ = g.run_slots(n, seed=3, n_random=16)
    return [(e, k, rgb.tolist(), ch) for e, k, rgb, ch in log], state


def assert_state_is(g, state, img):
    pal, b, tps, pm = state
    opaque = img[..., 3] != 0
    assert np.array_equal(g.palette, pal) and np.array_equal(g.tile_palettes[:len(tps)], tps) and np.array_equal(g.palette_map[opaque], pm[opaque])
    if b is not None:
        assert np.array_equal(g.backdrop, b)


# ---- 1. an import is the setters, in one step ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,h,count,size,flags,lay", [
    ("2x3", 16, 2, 3, {}, {}),
    ("8x15", 16, 8, 15, {}, dict(char_base=0x100, palette_base=0)),
    ("1x20", 8, 1, 20, {}, {}),
    ("2x3_backdrop", 16, 2, 3, dict(backdrop=True), {}),
    ("2x3_backdrop_based", 16, 2, 3, dict(backdrop=True), dict(bpp=4, palette_base=6, char_base=960)),
    ("transparent_block", 16, 2, 3, {}, dict(bpp=4, palette_base=3, char_base=5)),
    ("mirrored", 16, 2, 3, {}, {}),
])
def test_import_is_the_four_setters_in_one_step(S, name, h, count, size, flags, lay):
    if name == "mirrored":  # the input on which all four flips occur (test_native_model.py shows it on the oracle)
        img = N.mirrored_image()
        a = N.mirrored_state(S.OptimizedImage(img, count, size))
    else:
        img = N.transparent_block_image() if name == "transparent_block" else image(h, len(name))
        a = started(S, img, count, size, **flags)
    ex = a.export_native(priority=1, **lay)  # (the priority bit is not read back)
    if name == "mirrored":
        assert sorted(set((ex["map"] >> 14).tolist())) == [0, 1, 2, 3]
    full = N.layout(**dict(lay, bpp=ex["bpp"]))
    state = I.parse(ex["cgram"], ex["chr"], ex["map"], full, size, count, bool(flags.get("backdrop")), img[..., 3])
    assert len(state) == 4, state
    if flags.get("backdrop"):
        assert (state[3] == size).any(), "the input breaks the premise: no pixel takes the backdrop colour"
    x, y = S.OptimizedImage(img, count, size, **flags), S.OptimizedImage(img, count, size, **flags)
    info = x.import_native(ex["cgram"], ex["chr"], ex["map"], **lay)
    assert info == dict(bpp=ex["bpp"], unique=ex["unique"], chr_bytes=len(ex["chr"]), map_words=32 * (h // 8))
    by_hand(y, state)
    assert_state_is(x, state, img)
    ox, oy, oa = observe(x, img), observe(y, img), observe(a, img)
    assert ox == oy
    assert ox == oa  # ... and both are the state the bytes were exported from
    lx, ly = slots(x), slots(y)
    assert lx == ly and np.array_equal(x.palette, y.palette) and np.array_equal(x.palette_map, y.palette_map) and x.error() == y.error()
    for g in (a, x, y):
        g.close()


# ---- 2. what optimize() cannot rebuild ---------------------------------------------------------------------------------------

def test_a_reduced_map_survives_export_and_import(S):
    img = image(16, 40)
    a = started(S, img, 2, 3)
    m0, U0 = a.palette_map.copy(), a.characters()[0]
    recs, U1 = a.reduce_characters(U0 // 2, 4)
    assert U1 == U0 // 2 and len(recs) == U0 - U1
    assert not np.array_equal(a.palette_map, m0), "the input breaks the premise: the merges left optimize()'s map"
    ex = a.export_native()
    b = S.OptimizedImage(img, 2, 3)
    b.import_native(ex["cgram"], ex["chr"], ex["map"])
    assert b.error() == recs[-1]["error"] == a.error()  # the incumbent of the reduction, bit for bit
    assert b.characters()[0] == U1 and b.as_tilemap_json() == a.as_tilemap_json() and b.as_json() == a.as_json()
    ex_b = b.export_native()
    assert ex_b["cgram"] == ex["cgram"] and ex_b["chr"] == ex["chr"] and np.array_equal(ex_b["map"], ex["map"])
    ra, rb = a.refit_characters(), b.refit_characters()
    assert len(ra[0]) > 0 and ra[0].tobytes() == rb[0].tobytes() and ra[1:] == rb[1:]
    assert np.array_equal(a.palette_map, b.palette_map) and a.error() == b.error()
    a.close()
    b.close()


# ---- 3. foreign bytes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backdrop", [False, True])
def test_foreign_bytes_load_to_the_state_the_model_reads(S, backdrop):
    img = N.transparent_block_image()
    a = started(S, img, 2, 3, backdrop=backdrop)
    u, rep, flip, chars = a.characters()
    bpp = 4 if backdrop else 2
    cgram, chr_, words, lay = K.foreign(chars, rep, flip, a.tile_palettes[:64], a.palette_u16.reshape(2, 3), a.backdrop if backdrop else None, bpp, seed=int(backdrop))
    assert ((words >> 14) != flip).any() and (words & 0x2000).any() and len(chr_) == (u + 2) * 8 * bpp
    state = I.parse(cgram, chr_, words, lay, 3, 2, backdrop, img[..., 3])
    assert len(state) == 4, state
    x = S.OptimizedImage(img, 2, 3, backdrop=backdrop)
    kw = dict(bpp=lay["bpp"], char_base=lay["char_base"], palette_base=lay["palette_base"])
    assert x.import_native(cgram, chr_, words, **kw)["unique"] == u + 2
    assert_state_is(x, state, img)
    opaque = img[..., 3] != 0
    drawn, want = x.render_native(cgram, chr_, words, **kw), x.as_rgba()
    assert np.array_equal(drawn[opaque][:, :3], want[opaque][:, :3])
    assert observe(x, img) == observe(a, img)
    a.close()
    x.close()


# ---- 4. refusals change nothing ------------------------------------------------------------------------------------------------

KW = dict(bpp=K.LAYOUT["bpp"], char_base=K.LAYOUT["char_base"], palette_base=K.LAYOUT["palette_base"])


@pytest.mark.parametrize("backdrop", [False, True])
def test_refusals_name_the_lowest_tile_and_change_nothing(S, backdrop):
    img = K.refusal_image()
    g = started(S, img, K.C, K.S, backdrop=backdrop)
    before = observe(g, img)
    cgram, cases = K.refusal_cases()
    accepted = []
    for name, words, chr_, plain, bd in cases:
        want = bd if backdrop else plain
        if want is None:
            accepted.append((words, chr_))
            continue
        msg = refused(S, lambda: g.import_native(cgram, chr_, words, **KW), ERR_ARG)
        assert I.REASON_TEXT[want[1]] in msg, (name, msg)
        if want[0] is not None:
            assert "tile %d " % want[0] in msg, (name, msg)
    assert "2 subpalettes" in refused(S, lambda: g.import_native(cgram, K.refusal_bytes()[1] * 4, cases[0][1], bpp=8), ERR_UNSUPPORTED)  # the layout's own refusals
    refused(S, lambda: g.import_native(cgram, cases[0][2], cases[0][1], bpp=2, palette_base=7), ERR_ARG)
    assert observe(g, img) == before
    assert len(accepted) == (1 if backdrop else 0)
    for words, chr_ in accepted:  # value 0 on the opaque tile 9: the backdrop colour shows
        g.import_native(cgram, chr_, words, **KW)
        assert (g.palette_map[0:8, 72:80] == K.S).all() and (g.palette_map[8:16] == 0).all()
    g.close()


def test_null_pointers_pending_phases_and_lent_contexts(S):
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    img = K.refusal_image()
    g = started(S, img, K.C, K.S)
    cgram, chr_, words = K.refusal_bytes()
    cg, ch = np.frombuffer(cgram, np.uint8), np.frombuffer(chr_, np.uint8)
    lay, info = _ffi.NativeLayout(2, 2, 0, 0, 4, 0), _ffi.NativeInfo()
    p8, p16 = lambda a: a.ctypes.data_as(_ffi._u8p), lambda a: a.ctypes.data_as(_ffi._u16p)
    call = g._L.snesimage_import_native
    assert call(g._c, C.byref(lay), None, p8(ch), ch.size, p16(words), C.byref(info)) == ERR_ARG
    assert call(g._c, C.byref(lay), p8(cg), None, ch.size, p16(words), C.byref(info)) == ERR_ARG
    assert call(g._c, C.byref(lay), p8(cg), p8(ch), ch.size, None, C.byref(info)) == ERR_ARG
    assert call(g._c, C.byref(lay), p8(cg), p8(ch), ch.size, p16(words), None) == 0  # info is optional; the bytes are a state
    g.close()
    g = started(S, img, K.C, K.S)
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    refused(S, lambda: g.import_native(cgram, chr_, words, **KW), ERR_STATE)
    g.step_commit(buf.ptr)
    taken, _ = g.slots_begin(4, 1, 1, (0, 1, 0, 0))
    refused(S, lambda: g.import_native(cgram, chr_, words, **KW), ERR_STATE)
    g.slots_commit(0, taken)
    other = started(S, img, K.C, K.S)
    other.palette = g.palette
    sp = S.SharedPalette([g, other])
    refused(S, lambda: g.import_native(cgram, chr_, words, **KW), ERR_STATE)
    sp.close()
    g.import_native(cgram, chr_, words, **KW)  # usable afterwards
    assert g.tile_palettes[K.CLEAR_TILE] == 1
    g.close()
    other.close()


def test_a_refusal_leaves_an_owed_optimize_owed(S):
    """A context whose last call left optimize() pending behaves after a refused import exactly as a twin never asked."""
    img = K.refusal_image()
    a, b = started(S, img, K.C, K.S), started(S, img, K.C, K.S)
    pal0 = a.palette.copy()
    for j, (method, p, i, ch, _) in enumerate(S.schedule(K.C, K.S, 4)):
        ea, _ = a.step(method, p, i, ch, 1, j)
        eb, _ = b.step(method, p, i, ch, 1, j)
        assert ea == eb
    assert not np.array_equal(a.palette, pal0), "the input breaks the premise: no call changed the palette"
    cgram, cases = K.refusal_cases()
    refused(S, lambda: a.import_native(cgram, cases[4][2], cases[4][1], **KW), ERR_ARG)
    la, lb = slots(a), slots(b)
    assert la == lb
    assert observe(a, img) == observe(b, img)
    a.close()
    b.close()


# ---- 5. sets -----------------------------------------------------------------------------------------------------------------

def fresh_set(S, frames, **flags):
    ctxs = [S.OptimizedImage(f, 2, 3, **flags) for f in frames]
    for c in ctxs:
        c.set_chunk(64)
    return ctxs


def close_all(sp, ctxs):
    sp.close()
    for c in ctxs:
        c.close()


def set_slots(sp, n=4):
    log, state, _ = sp.run_slots(n, seed=5, n_random=16)
    return [(e, k, rgb.tolist(), ch) for e, k, rgb, ch in log], state


def test_set_round_trip_and_the_calls_that_follow(S):
    frames = [image(16, 70), image(16, 71)]
    ctxs = fresh_set(S, frames)
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    U0 = sp.characters()[0]
    before = [c.palette_map.copy() for c in ctxs]
    recs, U1 = sp.reduce_characters(U0 - 12, 4)
    assert U1 == U0 - 12 and any(not np.array_equal(c.palette_map, m) for c, m in zip(ctxs, before))
    E, ex, tm = sp.error(), sp.export_native(), sp.as_tilemap_json()
    assert ex["map"].shape == (2, 64)
    # into a fresh set of the same frames
    ctxs2 = fresh_set(S, frames)
    sp2 = S.SharedPalette(ctxs2)
    info = sp2.import_native(ex["cgram"], ex["chr"], ex["map"])
    assert info == dict(bpp=2, unique=U1, chr_bytes=len(ex["chr"]), map_words=128)
    assert sp2.error() == E
    for c, c2 in zip(ctxs, ctxs2):
        assert np.array_equal(c.palette_map, c2.palette_map) and np.array_equal(c.tile_palettes[:64], c2.tile_palettes[:64]) and np.array_equal(c.palette, c2.palette)
    ex2 = sp2.export_native()
    assert sp2.as_tilemap_json() == tm and ex2["cgram"] == ex["cgram"] and ex2["chr"] == ex["chr"] and np.array_equal(ex2["map"], ex["map"])
    # a bad word in frame 1 leaves frame 0 (and everything else) untouched
    bad = ex["map"].copy()
    bad[1, 7] |= 7 << 10
    bad[1, 9] = 1023
    msg = refused(S, lambda: sp2.import_native(ex["cgram"], ex["chr"], bad), ERR_ARG)
    assert "tile 7 of member 1" in msg and I.REASON_TEXT[I.PALETTE] in msg
    for c, c2 in zip(ctxs, ctxs2):
        assert np.array_equal(c.palette_map, c2.palette_map)
    assert sp2.error() == E
    # the calls that follow: as on a set whose members got the parsed state by hand
    state = I.parse(ex["cgram"], ex["chr"], ex["map"].reshape(-1), N.layout(2), 3, 2, False, np.stack([f[..., 3] for f in frames]))
    assert len(state) == 4, state
    ctxs3 = fresh_set(S, frames)
    for m, c in enumerate(ctxs3):
        by_hand(c, (state[0], None, state[2][64 * m:64 * m + 64], state[3][m]))
    sp3 = S.SharedPalette(ctxs3)
    l2, l3 = set_slots(sp2), set_slots(sp3)
    assert l2 == l3 and np.array_equal(sp2.palette, sp3.palette)
    for c2, c3 in zip(ctxs2, ctxs3):
        assert np.array_equal(c2.palette_map, c3.palette_map)
    assert sp2.error() == sp3.error()  # the set stays intact
    close_all(sp, ctxs)
    close_all(sp2, ctxs2)
    close_all(sp3, ctxs3)


def test_backdrop_set_is_refused_by_name_and_still_steps(S):
    ctxs = fresh_set(S, [image(8, 72), image(8, 73)], backdrop=True)
    sp = S.SharedPalette(ctxs, backdrop=True)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    words = np.zeros((2, 32), np.uint16)
    assert "snesimage_shared_import_native" in refused(S, lambda: sp.import_native(bytes(512), bytes(16), words), ERR_UNSUPPORTED)
    e, _ = sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 8)
    assert np.isfinite(e) and e > 0
    close_all(sp, ctxs)


# ---- 6. the CLI ----------------------------------------------------------------------------------------------------------------

def test_cli_continues_from_native_files(tmp_path):
    raw, raw2 = str(tmp_path / "a.rgba"), str(tmp_path / "b.rgba")
    image(16, 80).tofile(raw)
    image(16, 81).tofile(raw2)
    p = lambda n: str(tmp_path / n)
    read = lambda n: open(p(n), "rb").read()
    geom = ["-c", "2", "-s", "3"]
    exports = lambda stem: ["--export-cgram", p(stem + ".cgram"), "--export-chr", p(stem + ".chr"), "--export-map", p(stem + ".map")]
    imports = lambda stem: ["--import-cgram", p(stem + ".cgram"), "--import-chr", p(stem + ".chr"), "--import-map", p(stem + ".map")]
    r = cli(raw, p("a.json"), *geom, "--calls", "4", "--candidates", "16", "--max-tiles", "40", *exports("a"))
    assert r.returncode == 0 and "Wrote native data" in r.stdout, r.stdout + r.stderr
    # the imported state itself: byte-identical JSON and exports, without an optimizer call
    r = cli(raw, p("b.json"), *geom, *imports("a"), *exports("b"))
    assert r.returncode == 0 and "Imported native data" in r.stdout and "Wrote native data" in r.stdout, r.stdout + r.stderr
    assert read("b.json") == read("a.json")
    for ext in (".cgram", ".chr", ".map"):
        assert read("b" + ext) == read("a" + ext), ext
    # the continuation: a lower budget on the imported, already reduced state; another layout on the way out
    r = cli(raw, p("c.json"), *geom, *imports("a"), "--max-tiles", "30", "--tilemap", p("c_tm.json"), *exports("c"), "--export-bpp", "4", "--export-char-base", "512")
    assert r.returncode == 0 and "Wrote native data" in r.stdout, r.stdout + r.stderr  # (its own render check passed)
    tm = json.load(open(p("c_tm.json")))
    assert len(tm["characters"]) <= 30 and len(read("c.chr")) == 32 * len(tm["characters"])
    assert json.load(open(p("c.json")))["palette"] == json.load(open(p("a.json")))["palette"]
    # ... and reading that layout back
    r = cli(raw, p("d.json"), *geom, *imports("c"), "--import-bpp", "4", "--import-char-base", "512")
    assert r.returncode == 0 and read("d.json") == read("c.json"), r.stdout + r.stderr
    # the library's refusal: exit 1 with its message, nothing written
    words = np.frombuffer(read("a.map"), "<u2").copy()
    words[3] |= 7 << 10
    words.astype("<u2").tofile(p("bad.map"))
    r = cli(raw, p("e.json"), *geom, "--import-cgram", p("a.cgram"), "--import-chr", p("a.chr"), "--import-map", p("bad.map"))
    assert r.returncode == 1 and "tile 3 " in r.stdout and not os.path.exists(p("e.json")), r.stdout + r.stderr
    # the same identity for a set
    sx = lambda stem: ["--set-export-cgram", p(stem + ".cgram"), "--set-export-chr", p(stem + ".chr"), "--set-export-map", p(stem + ".map")]
    r = cli(raw, p("s0.json"), *geom, "--calls", "4", "--candidates", "16", "--share", raw2 + "=" + p("s1.json"), "--max-set-tiles", "100", *sx("s"))
    assert r.returncode == 0 and "Wrote native data of the set" in r.stdout, r.stdout + r.stderr
    r = cli(raw, p("t0.json"), *geom, "--share", raw2 + "=" + p("t1.json"), "--set-import-cgram", p("s.cgram"), "--set-import-chr", p("s.chr"), "--set-import-map", p("s.map"), *sx("t"))
    assert r.returncode == 0 and "Imported native data of the set" in r.stdout, r.stdout + r.stderr
    assert read("t0.json") == read("s0.json") and read("t1.json") == read("s1.json")
    for ext in (".cgram", ".chr", ".map"):
        assert read("t" + ext) == read("s" + ext), ext
