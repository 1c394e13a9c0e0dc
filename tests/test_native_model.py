"""The native export without a GPU: the formats of include/snesimage_hip.h ("Native export") as known answers written out by
hand, the numpy model (native_model.py) round-tripping and drawing what the CPU oracle draws, the premise of the mirrored
image, the new symbols' null-context refusals and the CLI's argument rules."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import backdrop_model as B
import character_model as M
import native_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


# ---- known answers -------------------------------------------------------------------------------------------------------

def hand_character():
    c = np.zeros((8, 8), np.uint8)  # c[y, x]
    c[0, 0], c[0, 7], c[1, 0], c[7, 7] = 1, 2, 4, 8
    return c.reshape(64)


def test_4bpp_cell_known_answer():
    cell = N.encode_cell(hand_character(), 4)
    want = np.zeros(32, np.uint8)
    want[0], want[1], want[18], want[31] = 0x80, 0x01, 0x80, 0x01  # plane 0 row 0; plane 1 row 0; plane 2 row 1; plane 3 row 7
    assert cell.tolist() == want.tolist()


def test_2bpp_and_8bpp_cell_known_answers():
    c = hand_character()
    two = N.encode_cell(np.where(c < 4, c, 0), 2)  # the values a 2bpp cell holds: 1 at (0,0), 2 at (7,0)
    want = np.zeros(16, np.uint8)
    want[0], want[1] = 0x80, 0x01
    assert two.tolist() == want.tolist()
    assert two.tolist() == N.encode_cell(c, 4)[:16].tolist()  # the first plane pair of the 4bpp cell
    c8 = np.zeros(64, np.uint8)
    c8[0] = 128
    eight = N.encode_cell(c8, 8)
    want = np.zeros(64, np.uint8)
    want[49] = 0x80  # plane 7 = pair 3, second of the pair, row 0: 16 * 3 + 2 * 0 + 1
    assert eight.tolist() == want.tolist()


def test_map_word_known_answer():
    assert N.map_word(5, 0x100, 3, 2, 1, 1, 0) == 0x7505
    assert N.map_word(5, 0x100, 3, 0, 1, 1, 0, bpp=8) == 0x6105  # no palette field at 8bpp
    assert N.map_word(0, 0, 0, 0, 0, 0, 1) == 0x8000


def test_cgram_rows_and_backdrop_word():
    pal = np.arange(1, 7, dtype=np.uint16).reshape(2, 3) * 0x421
    two = np.frombuffer(N.encode_cgram(pal, None, 2), "<u2")
    assert two[:8].tolist() == [0, 0x421, 0x842, 0xC63, 0, 0x1084, 0x14A5, 0x18C6] and not two[8:].any()  # row p at word 4p
    four = np.frombuffer(N.encode_cgram(pal, None, 4, palette_base=3), "<u2")
    assert four[48:52].tolist() == [0, 0x421, 0x842, 0xC63] and four[64:68].tolist() == [0, 0x1084, 0x14A5, 0x18C6]
    assert not four[:48].any() and not four[52:64].any() and not four[68:].any()
    b = (31, 0, 16)  # 31 | 16 << 10
    bd = np.frombuffer(N.encode_cgram(pal, b, 4, palette_base=1), "<u2")
    assert bd[0] == 0x401F and bd[16] == 0x401F and bd[32] == 0x401F and bd[48] == 0
    one = np.frombuffer(N.encode_cgram(np.arange(1, 21, dtype=np.uint16)[None, :], b, 8), "<u2")
    assert one[0] == 0x401F and one[1:21].tolist() == list(range(1, 21)) and not one[21:].any()


# ---- round trip ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bpp,S,C", [(2, 3, 2), (4, 15, 8), (8, 200, 1)])
def test_decode_gives_back_random_characters_under_all_four_flips(bpp, S, C):
    rng = np.random.default_rng(bpp)
    base = rng.integers(0, S + 1, (16, 64)).astype(np.uint8)
    chars = np.concatenate([M.flip_char(base, f) for f in range(4)])  # tiles 16f .. 16f + 15: flip f of the first sixteen
    rep, flip, U, _ = M.classes(chars)
    assert U == 16 and sorted(set(flip.tolist())) == [0, 1, 2, 3]
    tp = rng.integers(0, C, 64).astype(np.uint8)
    pal = rng.integers(0, 32768, (C, S)).astype(np.uint16)
    lay = N.layout(bpp, char_base=7, palette_base=0 if bpp == 8 else 8 - C, priority=1)
    cgram, chr_, words, got_bpp = N.encode(chars, rep, flip, tp, pal, (3, 4, 5), lay)
    assert got_bpp == bpp and len(chr_) == 16 * 8 * bpp and len(cgram) == 512
    img = N.decode(cgram, chr_, words, lay, 16)
    b16 = 3 | 4 << 5 | 5 << 10
    word = np.where(chars == 0, b16, pal[tp[:, None], np.maximum(chars.astype(np.int64) - 1, 0)])
    want = np.stack([M.untile(N.rgb_of_word(word)[..., ch], 16) for ch in range(3)], axis=-1)
    assert np.array_equal(img[..., :3], want) and (img[..., 3] == 255).all()


# ---- against the oracle ------------------------------------------------------------------------------------------------------

def oracle_pieces(o, img, C, S, zero_at=None):
    """What encode is fed, from an oracle context (the expanded one of a backdrop model with zero_at = S)."""
    ntile = 32 * (img.shape[0] // 8)
    chars = M.characters(o.palette_map, img, zero_at)
    rep, flip, U, _ = M.classes(chars)
    pal = o.palette_u16.reshape(C, -1)[:, :S]
    return chars, rep, flip, o.tile_palettes[:ntile], pal, U


def assert_draws_as(cgram, chr_, words, lay, want):
    got = N.decode(cgram, chr_, words, lay, want.shape[0])
    opaque = want[..., 3] != 0
    assert opaque.any() and np.array_equal(got[opaque][:, :3], want[opaque][:, :3])
    zero = N.rgb_of_word(np.frombuffer(cgram, "<u2")[0])
    assert (got[~opaque][:, :3] == zero).all() and (got[..., 3] == 255).all()


@pytest.mark.parametrize("bpp", [0, 4])
def test_oracle_2x3_draws_as_the_oracle_and_cgram_is_the_jsons_palette(O, bpp):
    img = B.image(16, 1)
    o = O.OracleImage(img, 2, 3)
    o.initialize_tiles()
    o.recalculate_palettes()
    chars, rep, flip, tp, pal, _ = oracle_pieces(o, img, 2, 3)
    cgram, chr_, words, got = N.encode(chars, rep, flip, tp, pal, None, N.layout(bpp))
    assert got == (bpp or 2)
    assert_draws_as(cgram, chr_, words, N.layout(got), o.as_rgba())
    if got == 4:  # CGRAM at 4bpp, base 0: the JSON's palette rows, zero-padded
        rows = json.loads(o.as_json())["palette"]
        cg = np.frombuffer(cgram, "<u2")
        assert cg[:len(rows)].tolist() == rows and not cg[len(rows):].any()
    o.close()


def test_backdrop_model_draws_as_the_oracle_and_holds_b_in_every_rows_first_word(O):
    img = B.image(16, 2)
    m = B.Model(O, img, 2, 3, {})
    chars, rep, flip, tp, pal, _ = oracle_pieces(m.o, img, 2, 3, zero_at=3)
    assert (chars == 0).any(), "the input breaks the premise: no pixel takes the backdrop colour"
    for bpp in (2, 4):
        cgram, chr_, words, _ = N.encode(chars, rep, flip, tp, pal, m.B, N.layout(bpp))
        assert_draws_as(cgram, chr_, words, N.layout(bpp), m.as_rgba())
        cg = np.frombuffer(cgram, "<u2")
        b16 = O.snes_as_u16(m.B)
        assert cg[0] == b16 and cg[1 << bpp] == b16
        if bpp == 4:
            rows = json.loads(m.as_json())["palette"]
            assert cg[:len(rows)].tolist() == rows and not cg[len(rows):].any()
    m.o.close()


def test_transparent_block_draws_as_the_oracle(O):
    img = N.transparent_block_image()
    o = O.OracleImage(img, 2, 3)
    o.initialize_tiles()
    o.recalculate_palettes()
    chars, rep, flip, tp, pal, _ = oracle_pieces(o, img, 2, 3)
    assert not chars[11].any() and (chars[10] == 0).any() and chars[10].any()
    cgram, chr_, words, bpp = N.encode(chars, rep, flip, tp, pal, None, N.layout(0, char_base=0x200, palette_base=5, priority=1))
    assert_draws_as(cgram, chr_, words, N.layout(bpp, char_base=0x200, palette_base=5, priority=1), o.as_rgba())
    o.close()


def test_mirrored_image_premise_holds_on_the_oracle(O):
    """What the GPU test leans on: on the mirrored image in its hand-made state all four values of flip_of occur, and U is
    the class count of the top-left quadrant."""
    img = N.mirrored_image()
    assert img.shape == (16, 256, 4) and np.array_equal(img, img[:, ::-1]) and np.array_equal(img, img[::-1])
    o = N.mirrored_state(O.OracleImage(img, *N.MIRROR_GEOMETRY))
    chars, rep, flip, tp, pal, U = oracle_pieces(o, img, *N.MIRROR_GEOMETRY)
    assert sorted(set(flip.tolist())) == [0, 1, 2, 3]
    assert U == M.classes(chars[:16])[2] and U > 1
    cgram, chr_, words, bpp = N.encode(chars, rep, flip, tp, pal, None, N.layout())
    assert_draws_as(cgram, chr_, words, N.layout(bpp), o.as_rgba())
    o.close()


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------------

def test_null_context_is_an_argument_error_on_every_new_call():
    from snesimage_amd import _ffi
    lib = _ffi.load()
    info, lay = _ffi.NativeInfo(), _ffi.NativeLayout()
    buf = (C.c_uint8 * 512)()
    words = (C.c_uint16 * 32)()
    u8 = lambda a: C.cast(a, _ffi._u8p)
    assert lib.snesimage_export_native(None, C.byref(lay), None, None, 0, None, C.byref(info)) == -1
    assert lib.snesimage_shared_export_native(None, C.byref(lay), None, None, 0, None, C.byref(info)) == -1
    assert lib.snesimage_render_native(None, C.byref(lay), u8(buf), u8(buf), 512, C.cast(words, _ffi._u16p), u8(buf)) == -1
    assert b"null" in lib.snesimage_last_error()
    assert C.sizeof(_ffi.NativeLayout) == 8 and C.sizeof(_ffi.NativeInfo) == 16


# ---- the CLI's argument rules ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,named", [
    (["--set-export-cgram", "x.bin"], "--set-export-cgram"),                                        # a set option without --share
    (["--set-export-map", "x.bin"], "--set-export-map"),
    (["--export-chr", "x.bin", "--share", "a=b"], "--export-chr"),                                  # the trio with --share
    (["--export-map", "x.bin", "--devices", "0,1"], "--export-map"),                                # ... and with --devices
    (["--set-export-chr", "x.bin", "--share", "a=b", "--devices", "0,1"], "--set-export-chr"),
    (["--set-export-chr", "x.bin", "--share", "a=b", "--set-backdrop"], "--set-backdrop"),
    (["--set-export-cgram", "x.bin", "--share", "a=b", "--set-backdrop-fixed", "1,2,3"], "--set-backdrop-fixed"),
    (["--export-chr", "x.bin", "--export-bpp", "3"], "--export-bpp"),
    (["--export-chr", "x.bin", "--export-char-base", "1024"], "--export-char-base"),                # a base out of range
    (["--export-chr", "x.bin", "--export-palette-base", "8"], "--export-palette-base"),
    (["--export-chr", "x.bin", "--export-priority", "2"], "--export-priority"),
    (["--export-chr", "x.bin", "--export-char-base", "-1"], "--export-char-base"),
    (["--export-bpp", "4"], "--export-bpp"),                                                        # a layout option without an export file
    (["--export-priority", "1", "--tilemap", "t.json"], "--export-priority"),
    (["--export-cgram"], "--export-cgram"),                                                         # no value
])
def test_cli_argument_rules_are_stated_while_parsing(tmp_path, extra, named):
    """Exit code 2 with the option named, before any file or device is touched: the source does not exist."""
    missing, out = str(tmp_path / "none.png"), str(tmp_path / "out.json")
    extra = [str(tmp_path / a) if a.endswith((".bin", ".json")) else a for a in extra]
    r = cli(missing, out, *extra)
    assert r.returncode == 2, (extra, r.stdout, r.stderr)
    assert named in r.stderr and "unexpected argument" not in r.stderr, r.stderr  # the rule itself, not an option the parser does not know
    assert os.listdir(tmp_path) == []


def test_cli_help_lists_the_export_options():
    r = cli("--help")
    assert r.returncode == 0
    for k in ("--export-cgram", "--export-chr", "--export-map", "--set-export-cgram", "--set-export-chr", "--set-export-map", "--export-bpp", "--export-char-base",
              "--export-palette-base", "--export-priority"):
        assert k in r.stderr, k
