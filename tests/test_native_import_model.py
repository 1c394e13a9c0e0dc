"""The native import without a GPU: the numpy model of the contract (native_import_model.py) against answers written out by hand,
against native_model's encoding of the CPU oracle's states — parse(encode(x)) == x, and decode(bytes) draws what the oracle
draws from the parsed state — every refusal with the lowest tile, the new symbols' null refusals and the CLI's argument rules."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backdrop_model as B
import character_model as M
import native_import_cases as K
import native_import_model as I
import native_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


# ---- known answers -------------------------------------------------------------------------------------------------------

def hand_parse(cell_bytes, bpp, S):
    """A backdrop picture of 256 x 8, all opaque: tile f (0..3) draws the cell under flip f from row 1, every other tile
    unflipped from row 0.  -> the four tiles' map values as (8, 8) arrays [y, x]."""
    words = np.array([N.map_word(0, 0, 0, 0, 0, 0, 0, bpp)] * 32, np.uint16)
    for f in range(4):
        words[f] = N.map_word(0, 0, 1, 0, 1, f & 1, f >> 1, bpp)  # (the priority bit is set: it is not read)
    got = I.parse(bytes(512), cell_bytes, words, N.layout(bpp), S, 2, True, np.full((8, 256), 255, np.uint8))
    assert len(got) == 4
    pal, b, tp, pm = got
    assert tp.tolist() == [1, 1, 1, 1] + [0] * 28 and not pal.any() and b.tolist() == [0, 0, 0]
    return [pm[:, 8 * f:8 * f + 8].astype(int) for f in range(4)]


def placed(S, **at):
    """An (8, 8) array of S (the backdrop value) with the given values at 'y,x' keys."""
    a = np.full((8, 8), S, int)
    for k, v in at.items():
        y, x = k[1:].split("_")
        a[int(y), int(x)] = v
    return a


def test_2bpp_cell_by_hand_under_each_flip():
    cell = bytes([0x80, 0x01, 0x80, 0x80] + [0] * 12)  # row 0: value 1 at x = 0, value 2 at x = 7; row 1: value 3 at x = 0
    t = hand_parse(cell, 2, 3)
    assert np.array_equal(t[0], placed(3, p0_0=0, p0_7=1, p1_0=2))
    assert np.array_equal(t[1], placed(3, p0_7=0, p0_0=1, p1_7=2))  # hflip: the screen's column x reads the cell's 7 - x
    assert np.array_equal(t[2], placed(3, p7_0=0, p7_7=1, p6_0=2))  # vflip: row y reads 7 - y
    assert np.array_equal(t[3], placed(3, p7_7=0, p7_0=1, p6_7=2))


def test_4bpp_cell_by_hand_under_each_flip():
    cell = np.zeros(32, np.uint8)
    cell[0], cell[1], cell[18], cell[31] = 0x80, 0x01, 0x80, 0x01  # 1 at (x 0, y 0), 2 at (7, 0), 4 at (0, 1), 8 at (7, 7): test_native_model.py
    t = hand_parse(cell.tobytes(), 4, 15)
    assert np.array_equal(t[0], placed(15, p0_0=0, p0_7=1, p1_0=3, p7_7=7))
    assert np.array_equal(t[1], placed(15, p0_7=0, p0_0=1, p1_7=3, p7_0=7))
    assert np.array_equal(t[2], placed(15, p7_0=0, p7_7=1, p6_0=3, p0_7=7))
    assert np.array_equal(t[3], placed(15, p7_7=0, p7_0=1, p6_7=3, p0_0=7))


def test_cgram_rows_bit_15_and_the_words_that_are_not_read():
    cg = np.full(256, 0xFFFF, np.uint16)  # garbage everywhere
    cg[0] = 0x8000 | 3 | 4 << 5 | 5 << 10
    cg[(3 << 4) + 1:(3 << 4) + 4] = [0x8421, 0x0842, 0x7FFF]  # row 0 at palette_base 3, 4bpp
    cg[(4 << 4) + 1:(4 << 4) + 4] = [1, 2 << 5, 3 << 10]
    words = np.array([N.map_word(0, 0, 0, 3, 0, 0, 0)] * 32, np.uint16)
    chr_ = N.encode_cell(np.ones(64, np.uint8), 4).tobytes()
    pal, b, tp, pm = I.parse(cg.astype("<u2").tobytes(), chr_, words, N.layout(4, palette_base=3), 3, 2, True, np.full((8, 256), 255, np.uint8))
    assert pal.tolist() == [[1, 1, 1], [2, 2, 2], [31, 31, 31], [1, 0, 0], [0, 2, 0], [0, 0, 3]] and b.tolist() == [3, 4, 5] and not pm.any()
    one = np.arange(256, dtype=np.uint16)  # 8bpp: one row at word 0, the palette field ignored
    words8 = np.array([N.map_word(0, 0, 0, 0, 0, 0, 0, 8) | 5 << 10] * 32, np.uint16)
    pal, b, tp, pm = I.parse(one.astype("<u2").tobytes(), N.encode_cell(np.full(64, 20, np.uint8), 8).tobytes(), words8, N.layout(8), 20, 1, False, np.full((8, 256), 255, np.uint8))
    assert b is None and not tp.any() and (pm == 19).all()
    assert [int(c[0]) | int(c[1]) << 5 | int(c[2]) << 10 for c in pal] == list(range(1, 21))


# ---- round trip on the oracle's states, and the picture ----------------------------------------------------------------------

def oracle_pieces(o, img, C_, S_, zero_at=None):
    ntile = 32 * (img.shape[0] // 8)
    chars = M.characters(o.palette_map, img, zero_at)
    rep, flip, U, _ = M.classes(chars)
    return chars, rep, flip, o.tile_palettes[:ntile], o.palette_u16.reshape(C_, -1)[:, :S_]


def round_trip(o, img, C_, S_, regular, backdrop, lay, O):
    """parse(encode(x)) == x, and decode(bytes) is the oracle's as_rgba of the parsed state wherever the source is opaque."""
    zero_at = S_ if backdrop is not None else None
    chars, rep, flip, tp, pal16 = oracle_pieces(o, img, C_, S_, zero_at)
    cgram, chr_, words, bpp = N.encode(chars, rep, flip, tp, pal16, backdrop, lay)
    got = I.parse(cgram, chr_, words, lay, S_, C_, backdrop is not None, img[..., 3])
    assert len(got) == 4, got
    pal, b, tps, pm = got
    opaque = img[..., 3] != 0
    assert np.array_equal(pal, np.asarray(regular).reshape(-1, 3))
    assert (b is None) if backdrop is None else np.array_equal(b, backdrop)
    assert np.array_equal(tps, tp)
    assert np.array_equal(pm[opaque], o.palette_map[opaque]) and not pm[~opaque].any()
    # the parsed state on a fresh oracle context draws what the bytes draw
    row = S_ + (backdrop is not None)
    o2 = O.OracleImage(img, C_, row)
    full = np.zeros((C_, row, 3), np.uint8)
    full[:, :S_] = pal.reshape(C_, S_, 3)
    if backdrop is not None:
        full[:, S_] = b
    tp1024 = np.zeros(1024, np.uint8)
    tp1024[:len(tps)] = tps
    o2.tile_palettes = tp1024
    o2.palette = full.reshape(-1, 3)
    o2.palette_map = pm
    want = o2.as_rgba()
    drawn = N.decode(cgram, chr_, words, dict(lay, bpp=bpp), img.shape[0])
    assert opaque.any() and np.array_equal(drawn[opaque][:, :3], want[opaque][:, :3])
    assert np.array_equal(want, o.as_rgba())
    o2.close()
    return words


@pytest.mark.parametrize("lay", [N.layout(), N.layout(4, char_base=100, palette_base=6, priority=1)])
def test_round_trip_plain(O, lay):
    img = B.image(16, 1)
    o = O.OracleImage(img, 2, 3)
    o.initialize_tiles()
    o.recalculate_palettes()
    round_trip(o, img, 2, 3, o.palette, None, lay, O)
    o.close()


def test_round_trip_backdrop(O):
    img = B.image(16, 2)
    m = B.Model(O, img, 2, 3, {})
    assert (m.palette_map == 3).any(), "the input breaks the premise: no pixel takes the backdrop colour"
    for lay in (N.layout(), N.layout(4, palette_base=1)):
        round_trip(m.o, img, 2, 3, m.regular, m.B, lay, O)
    m.o.close()


def test_round_trip_transparent_block(O):
    img = N.transparent_block_image()
    o = O.OracleImage(img, 2, 3)
    o.initialize_tiles()
    o.recalculate_palettes()
    round_trip(o, img, 2, 3, o.palette, None, N.layout(0, char_base=0x200, palette_base=5, priority=1), O)
    o.close()


def test_round_trip_mirrored_with_all_four_flips(O):
    img = N.mirrored_image()
    o = N.mirrored_state(O.OracleImage(img, *N.MIRROR_GEOMETRY))
    words = round_trip(o, img, *N.MIRROR_GEOMETRY, o.palette, None, N.layout(), O)
    assert sorted(set((words >> 14).tolist())) == [0, 1, 2, 3]
    o.close()


def test_foreign_encoding_parses_to_the_same_state(O):
    """Shuffled, duplicated and unused cells, bases, priority bits, another flip for a symmetric cell, garbage in CGRAM."""
    img = N.transparent_block_image()
    o = O.OracleImage(img, 2, 3)
    o.initialize_tiles()
    o.recalculate_palettes()
    chars, rep, flip, tp, pal16 = oracle_pieces(o, img, 2, 3)
    cgram, chr_, words, lay = K.foreign(chars, rep, flip, tp, pal16, None, 2)
    assert ((words >> 14) != flip).any() and (words & 0x2000).any()
    pal, b, tps, pm = I.parse(cgram, chr_, words, lay, 3, 2, False, img[..., 3])
    opaque = img[..., 3] != 0
    assert np.array_equal(pal, o.palette) and np.array_equal(tps, tp) and np.array_equal(pm[opaque], o.palette_map[opaque])
    drawn = N.decode(cgram, chr_, words, lay, 16)
    assert np.array_equal(drawn[opaque][:, :3], o.as_rgba()[opaque][:, :3])
    o.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_the_base_of_the_refusal_cases_is_accepted():
    cgram, chr_, words = K.refusal_bytes()
    alpha = K.refusal_image()[..., 3]
    for backdrop in (False, True):
        got = I.parse(cgram, chr_, words, K.LAYOUT, K.S, K.C, backdrop, alpha)
        assert len(got) == 4
        assert got[2].tolist() == [1 if t == K.CLEAR_TILE else (0 if t == K.HALF_TILE else t % 2) for t in range(64)]


def test_every_refusal_names_the_lowest_tile_and_its_first_reason():
    cgram, cases = K.refusal_cases()
    alpha = K.refusal_image()[..., 3]
    assert {c[3][1] for c in cases} == {I.CHR, I.BELOW, I.PAST, I.PALETTE, I.VALUE, I.OPAQUE_ZERO, I.CLEAR_VALUE}
    for name, words, chr_, plain, backdrop in cases:
        assert I.parse(cgram, chr_, words, K.LAYOUT, K.S, K.C, False, alpha) == plain, name
        got = I.parse(cgram, chr_, words, K.LAYOUT, K.S, K.C, True, alpha)
        assert (len(got) == 4) if backdrop is None else (got == backdrop), name


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------------

def test_null_context_and_null_set_are_argument_errors():
    from snesimage_amd import _ffi
    lib = _ffi.load()
    info, lay = _ffi.NativeInfo(), _ffi.NativeLayout()
    buf = (C.c_uint8 * 512)()
    words = (C.c_uint16 * 32)()
    u8 = lambda a: C.cast(a, _ffi._u8p)
    assert lib.snesimage_import_native(None, C.byref(lay), u8(buf), u8(buf), 512, C.cast(words, _ffi._u16p), C.byref(info)) == -1
    assert b"null" in lib.snesimage_last_error()
    assert lib.snesimage_shared_import_native(None, C.byref(lay), u8(buf), u8(buf), 512, C.cast(words, _ffi._u16p), C.byref(info)) == -1
    assert b"null" in lib.snesimage_last_error()


def test_header_no_longer_lists_a_reader_as_out_of_scope():
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    assert "a reader of native files" not in text and "Native import — NOT a reference method" in text


# ---- the CLI's argument rules ----------------------------------------------------------------------------------------------

TRIO = ["--import-cgram", "c.bin", "--import-chr", "h.bin", "--import-map", "m.bin"]
SET_TRIO = ["--set-import-cgram", "c.bin", "--set-import-chr", "h.bin", "--set-import-map", "m.bin"]


@pytest.mark.parametrize("extra,named", [
    (["--import-cgram", "c.bin"], "--import-chr"),                                     # all three together
    (["--import-chr", "h.bin", "--import-map", "m.bin"], "--import-cgram"),
    (TRIO + ["--resume", "r.json"], "--resume"),
    (TRIO + ["--tile-palettes", "t.bin"], "--tile-palettes"),
    (TRIO + ["--devices", "0,1"], "--devices"),
    (TRIO + ["--share", "a=b"], "--share"),
    (TRIO + ["--backdrop-fixed", "1,2,3"], "--backdrop-fixed"),
    (SET_TRIO, "--share"),                                                             # the set's trio needs --share
    (SET_TRIO[:4] + ["--share", "a=b"], "--set-import-map"),
    (SET_TRIO + ["--share", "a=b", "--devices", "0,1"], "--devices"),
    (SET_TRIO + ["--share", "a=b", "--set-backdrop"], "--set-backdrop"),
    (SET_TRIO + ["--share", "a=b", "--set-backdrop-fixed", "1,2,3"], "--set-backdrop-fixed"),
    (SET_TRIO + ["--share", "a=b", "--resume", "r.json"], "--resume"),
    (TRIO + ["--import-bpp", "3"], "--import-bpp"),
    (TRIO + ["--import-char-base", "1024"], "--import-char-base"),
    (TRIO + ["--import-palette-base", "8"], "--import-palette-base"),
    (["--import-bpp", "4"], "--import-bpp"),                                           # a layout option without the files
    (["--import-char-base", "5", "--export-chr", "x.bin"], "--import-char-base"),      # the export's files do not count
    (["--import-map"], "--import-map"),                                                # no value
])
def test_cli_argument_rules_are_stated_while_parsing(tmp_path, extra, named):
    """Exit code 2 with the option named, before any file or device is touched: neither the source nor the files exist."""
    missing, out = str(tmp_path / "none.png"), str(tmp_path / "out.json")
    extra = [str(tmp_path / a) if a.endswith((".bin", ".json")) else a for a in extra]
    r = cli(missing, out, *extra)
    assert r.returncode == 2, (extra, r.stdout, r.stderr)
    assert named in r.stderr and "unexpected argument" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("which,size", [(0, 511), (1, 16 * 3 + 1), (2, 2 * 64 - 2), (1, 0)])
def test_cli_refuses_a_wrong_sized_file_before_a_device_is_touched(tmp_path, which, size):
    """CGRAM is 512 bytes, MAP two bytes per tile, CHR whole cells: exit 2, and nothing is written."""
    raw = str(tmp_path / "a.rgba")
    K.refusal_image().tofile(raw)
    sizes = [512, 16 * 3, 2 * 64]
    sizes[which] = size
    names = [str(tmp_path / n) for n in ("c.bin", "h.bin", "m.bin")]
    for n, s in zip(names, sizes):
        open(n, "wb").write(bytes(s))
    before = sorted(os.listdir(tmp_path))
    r = cli(raw, str(tmp_path / "out.json"), "-c", "2", "-s", "3", "--import-cgram", names[0], "--import-chr", names[1], "--import-map", names[2])
    assert r.returncode == 2 and os.path.basename(names[which]) in r.stderr, (r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == before


def test_cli_help_lists_the_import_options_and_says_what_a_call_does_to_the_map():
    r = cli("--help")
    assert r.returncode == 0
    for k in ("--import-cgram", "--import-chr", "--import-map", "--set-import-cgram", "--set-import-chr", "--set-import-map", "--import-bpp", "--import-char-base",
              "--import-palette-base"):
        assert k in r.stderr, k
    assert "replaces the imported map" in r.stderr
