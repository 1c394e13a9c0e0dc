"""One palette shared by several images (a set: snesimage_shared_*, snesimage_amd.SharedPalette, cli --share).

The model is the unchanged oracle: one OracleImage per member for maps and scores, and the member stack (the members top to
bottom, W x F*H) for the initialisers, which are defined as the reference's own on that picture."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL = 1e-11
SHARED_FUNCS = ["snesimage_shared_create", "snesimage_shared_destroy", "snesimage_shared_initialize_tiles",
                "snesimage_shared_recalculate_palettes", "snesimage_shared_set_palette_rgb5", "snesimage_shared_error",
                "snesimage_shared_score_candidates", "snesimage_shared_step", "snesimage_shared_step_async",
                "snesimage_shared_last_step", "snesimage_shared_reassign_tiles"]


def rel(a, b):
    return abs(a - b) / abs(b)


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)


def write_png(path, rgba):
    """A minimal RGBA8 PNG (filter 0 on every row)."""
    h, w = rgba.shape[:2]
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                     chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


# ---- without a device ------------------------------------------------------------------------------------------------------

def test_shared_symbols_exported_and_declared():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in SHARED_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    out = C.c_void_p()
    assert lib.snesimage_shared_create(None, 2, C.byref(out)) == -1 and not out.value
    empty = (C.c_void_p * 1)(None)
    assert lib.snesimage_shared_create(empty, 0, C.byref(out)) == -1
    assert lib.snesimage_shared_create(empty, 1, C.byref(out)) == -1 and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_shared_create(empty, 1, None) == -1
    assert lib.snesimage_shared_error(None, None) == -1
    lib.snesimage_shared_destroy(None)  # a no-op, as snesimage_destroy(NULL)


def test_cli_share_argument_rules(tmp_path):
    """Malformed --share and the combinations a set does not take are refused while parsing: the sources do not even exist,
    so a refusal after any file or device access would exit 1 instead."""
    missing, out = str(tmp_path / "none.png"), str(tmp_path / "o.json")
    r = cli(missing, out, "--share", "frame1.png")
    assert r.returncode == 2 and "--share" in r.stderr and "SOURCE=TARGET" in r.stderr
    r = cli(missing, out, "--share")
    assert r.returncode == 2 and "--share" in r.stderr
    for extra, name in [(["--resume", missing], "--resume"), (["--devices", "0,1"], "--devices"),
                        (["--tile-palettes", missing], "--tile-palettes"), (["--window", "8"], "--window")]:
        r = cli(missing, out, "--share", "%s=%s" % (missing, out), *extra)
        assert r.returncode == 2, extra
        assert "cannot be used with" in r.stderr and name in r.stderr and "--share" in r.stderr, r.stderr
    r = cli("--help")
    assert r.returncode == 0 and "--share" in r.stderr
    assert not os.path.exists(out)


# ---- on the MI355X ---------------------------------------------------------------------------------------------------------

def frames(F, H, variant=0, seed=0x5EED5000):
    from snesimage_amd.synth import synth_image
    return [synth_image(seed + i, 256, H, variant) for i in range(F)]


def make_set(imgs, sub_count, sub_size, chunk=64, **flags):
    import snesimage_amd as S
    ctxs = [S.OptimizedImage(f, sub_count, sub_size, device=0, **flags) for f in imgs]
    for c in ctxs:
        c.set_chunk(chunk)
    return ctxs, S.SharedPalette(ctxs)


def oracle_members(O, imgs, ctxs, sub_count, sub_size, **flags):
    """One oracle image per member, in the member's state (tile palettes, palette, optimize())."""
    out = []
    for f, c in zip(imgs, ctxs):
        o = O.OracleImage(f, sub_count, sub_size, **flags)
        o.tile_palettes = c.tile_palettes
        o.palette = c.palette
        o.optimize()
        out.append(o)
    return out


def check_members(O, imgs, ctxs, sp, sub_count, sub_size, **flags):
    """Every member holds the set's palette and its own oracle map under it; E is the members' oracle errors summed."""
    pal = ctxs[0].palette
    oms = oracle_members(O, imgs, ctxs, sub_count, sub_size, **flags)
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette, pal)
        assert np.array_equal(c.palette_map, o.palette_map)
    e_o = 0.0
    for o in oms:
        e_o = e_o + o.error()
    assert rel(sp.error(), e_o) < REL
    return oms


@pytest.mark.gpu
@pytest.mark.parametrize("F,H,variant,sub_count,sub_size,flags", [
    (1, 112, 1, 4, 7, {}),
    (2, 112, 0, 4, 7, {}),
    (3, 80, 1, 4, 7, {"perceptual": True}),
    (4, 56, 0, 4, 3, {"nes": True}),
    (2, 112, 1, 1, 7, {}),
    (3, 80, 0, 1, 7, {"perceptual": True}),
    (4, 56, 1, 4, 3, {}),
])
def test_initialisers_equal_the_stacked_oracle(O, F, H, variant, sub_count, sub_size, flags):
    imgs = frames(F, H, variant)
    stacked = O.OracleImage(np.concatenate(imgs, axis=0), sub_count, sub_size, **flags)
    ctxs, sp = make_set(imgs, sub_count, sub_size, **flags)
    per = 32 * (H // 8)  # tiles per member
    for phase in ("initialize_tiles", "recalculate_palettes"):
        getattr(stacked, phase)()
        getattr(sp, phase)()
        tp = stacked.tile_palettes
        for i, c in enumerate(ctxs):
            assert np.array_equal(c.tile_palettes[:per], tp[i * per:(i + 1) * per]), (phase, i)
        assert np.array_equal(ctxs[0].palette, stacked.palette), phase
        check_members(O, imgs, ctxs, sp, sub_count, sub_size, **flags)
    sp.close()
    for c in ctxs:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"perceptual": True}, {"dither": True}])
def test_joint_scores_are_the_summed_oracle_scores(O, flags):
    import snesimage_amd as S
    imgs = frames(3, 80, 1, seed=0x5EED5100)
    ctxs, sp = make_set(imgs, 2, 3, **flags)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    before = [(c.palette, c.palette_map, c.error()) for c in ctxs]
    cand = S.random_candidates(11, 3, 16)
    e_g = sp.score_candidates(1, 2, cand)
    oms = oracle_members(O, imgs, ctxs, 2, 3, **flags)
    e_o = None
    for o in oms:
        e = o.score_candidates(1, 2, cand)
        e_o = e if e_o is None else e_o + e
    assert float(np.max(np.abs(e_g - e_o) / np.abs(e_o))) < REL
    for c, (pal, pmap, err) in zip(ctxs, before):  # the members are unchanged
        assert np.array_equal(c.palette, pal) and np.array_equal(c.palette_map, pmap) and c.error() == err
    # and the set still steps afterwards
    sp.step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)
    sp.close()
    for c in ctxs:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"dither": True}])
def test_trajectory_follows_the_summed_oracle(O, flags):
    """24 calls of the reference's schedule with 16 random candidates: every call's winner and the palette after it equal
    the model's — the members' oracle scores summed, the reference's acceptance rule on the sum."""
    import snesimage_amd as S
    imgs = frames(3, 80, 1, seed=0x5EED5200)
    ctxs, sp = make_set(imgs, 2, 3, **flags)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    oms = oracle_members(O, imgs, ctxs, 2, 3, **flags)
    pal = oms[0].palette
    seed, n_random = 9, 16
    log, _ = sp.run(24, seed=seed, first_step_id=0, n_random=n_random)
    for j, (method, p, idx, ch, _) in enumerate(O.schedule(2, 3, 24)):
        assert method == 0
        cand = O.random_candidates(seed, j, n_random)
        inc = 0.0
        for o in oms:
            inc = inc + o.error()
        E = None
        for o in oms:
            e = o.score_candidates(p, idx, cand)
            E = e if E is None else E + e
        k = int(np.argmin(E))  # the first index of the minimum
        slot = p * 3 + idx
        if E[k] < inc:
            pal[slot] = cand[k]
            for o in oms:
                o.palette = pal
                o.optimize()
        e_g, k_g, rgb_g, _ = log[j]
        assert np.array_equal(rgb_g, pal[slot]), j
        assert (k_g == k) == bool(E[k] < inc), j
        assert rel(e_g, E[k] if E[k] < inc else inc) < REL, j
    assert np.array_equal(ctxs[0].palette, pal)
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette, pal) and np.array_equal(c.palette_map, o.palette_map)
    sp.close()
    for c in ctxs:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,n_calls", [({}, 110), ({"dither": True}, 110), ({"nes": True}, 60)])
def test_set_of_one_steps_as_a_plain_context(flags, n_calls):
    """F = 1: palette, map and error bit-identical to snesimage_step after every call (random, channel, NES methods)."""
    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    img = synth_image(0x5EED5300, 256, 64, 1)
    solo = S.OptimizedImage(img, 2, 3, device=0, **flags)
    solo.set_chunk(64)
    ctxs, sp = make_set([img], 2, 3, **flags)
    solo.initialize_tiles()
    solo.recalculate_palettes()
    sp.initialize_tiles()
    sp.recalculate_palettes()
    assert np.array_equal(solo.palette, ctxs[0].palette) and np.array_equal(solo.tile_palettes, ctxs[0].tile_palettes)
    sched = S.schedule(2, 3, n_calls, nes=bool(flags.get("nes")))
    methods = set()
    for j, (method, p, idx, ch, _) in enumerate(sched):
        methods.add(method)
        e_s, b_s = solo.step(method, p, idx, ch, 5, j, 0)
        e_g, b_g = sp.step(method, p, idx, ch, 5, j, 0)
        assert e_g == e_s and np.array_equal(b_g, b_s), j
        if j % 10 == 9 or j == n_calls - 1:
            assert np.array_equal(ctxs[0].palette, solo.palette), j
            assert np.array_equal(ctxs[0].palette_map, solo.palette_map), j
    assert methods == ({S.METHOD_NES} if flags.get("nes") else {S.METHOD_RANDOM, S.METHOD_CHANNEL})
    assert sp.error() == solo.error()
    sp.close()
    ctxs[0].close()
    solo.close()


@pytest.mark.gpu
def test_set_state_and_lifetime(monkeypatch):
    import snesimage_amd as S
    from snesimage_amd import _ffi
    imgs = frames(2, 64, 0, seed=0x5EED5400)

    def ctx(img, chunk=64, **flags):
        c = S.OptimizedImage(img, 2, 3, device=0, **flags)
        c.set_chunk(chunk)
        return c

    def refused(ctxs, code):
        with pytest.raises(S.SnesImageError) as e:
            S.SharedPalette(ctxs)
        assert e.value.code == code, str(e.value)

    # mismatched size, flags, chunk: SNES_ERR_ARG
    from snesimage_amd.synth import synth_image
    a, b = ctx(imgs[0]), ctx(synth_image(3, 256, 128))
    refused([a, b], -1)
    b.close()
    b = ctx(imgs[1], perceptual=True)
    refused([a, b], -1)
    b.close()
    b = ctx(imgs[1], chunk=128)
    refused([a, b], -1)
    b.close()
    # differing palettes: SNES_ERR_STATE
    b = ctx(imgs[1])
    pal = b.palette
    pal[0] = (pal[0] + 1) % 32
    b.palette = pal
    refused([a, b], -3)
    b.close()
    # a context lent to a batch is refused
    b = ctx(imgs[1])
    L = _ffi.load()
    arr = (C.c_void_p * 1)(b._c)
    h = C.c_void_p()
    assert L.snesimage_batch_create(arr, 1, C.byref(h)) == 0
    refused([a, b], -3)
    L.snesimage_batch_destroy(h)
    # a member changed from outside: the next set call fails
    sp = S.SharedPalette([a, b])
    sp.initialize_tiles()
    sp.step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)
    pal = b.palette
    pal[1] = (pal[1] + 3) % 32
    b.palette = pal
    with pytest.raises(S.SnesImageError) as e:
        sp.step(S.METHOD_RANDOM, 0, 1, 0, 1, 1, 16)
    assert e.value.code == -3
    with pytest.raises(S.SnesImageError) as e:
        S.SharedPalette([a])  # still lent to the set
    assert e.value.code == -3
    sp.close()
    # a destroyed member retires the set
    a.close()
    a = ctx(imgs[0])
    sp = S.SharedPalette([a, ctx(imgs[1])])
    sp.initialize_tiles()
    sp.images[1].close()
    with pytest.raises(S.SnesImageError) as e:
        sp.step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)
    assert e.value.code == -3
    with pytest.raises(S.SnesImageError) as e:
        sp.error()
    assert e.value.code == -3
    sp.close()
    a.step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)  # the surviving member is its own again
    a.close()
    b.close()
    # SNES_SPARSE=0: SNES_ERR_UNSUPPORTED
    monkeypatch.setenv("SNES_SPARSE", "0")
    a, b = ctx(imgs[0]), ctx(imgs[1])
    refused([a, b], -5)
    a.close()
    b.close()


@pytest.mark.gpu
def test_shared_reassign_tiles_equals_the_oracle_per_member(O):
    import snesimage_amd as S
    imgs = frames(2, 112, 1, seed=0x5EED5500)
    ctxs, sp = make_set(imgs, 4, 7)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    sp.run(6, seed=2, n_random=16)
    oms = oracle_members(O, imgs, ctxs, 4, 7)
    moved_o = sum(o.reassign_tiles() for o in oms)
    assert sp.reassign_tiles() == moved_o and moved_o > 0
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.tile_palettes, o.tile_palettes)
        assert np.array_equal(c.palette_map, o.palette_map)
        assert np.array_equal(c.palette, ctxs[0].palette)
    sp.step(S.METHOD_RANDOM, 0, 0, 0, 1, 100, 16)  # the set goes on from the new tile palettes
    sp.close()
    for c in ctxs:
        c.close()


@pytest.mark.gpu
def test_cli_share_end_to_end(tmp_path, O):
    """Two PNG frames, 30 calls: two JSON files with one palette; each equals the oracle's as_json for its frame under
    the palette and tile palettes it holds."""
    imgs = frames(2, 64, 1, seed=0x5EED5600)
    for i, f in enumerate(imgs):
        write_png(tmp_path / ("f%d.png" % i), f)
    r = cli(str(tmp_path / "f0.png"), str(tmp_path / "o0.json"), "--share", "%s=%s" % (tmp_path / "f1.png", tmp_path / "o1.json"),
            "-c", "2", "-s", "3", "--calls", "30", "--candidates", "16", "--reassign-tiles", "2")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Current Error" in r.stdout and "Sharing one palette between 2 images" in r.stdout
    outs = [json.loads((tmp_path / ("o%d.json" % i)).read_text()) for i in range(2)]
    assert outs[0]["palette"] == outs[1]["palette"]
    pal16 = outs[0]["palette"]
    rgb5 = np.array([[v & 31, (v >> 5) & 31, (v >> 10) & 31] for p in range(2) for v in pal16[16 * p + 1:16 * p + 4]], np.uint8)
    for i, f in enumerate(imgs):
        o = O.OracleImage(f, 2, 3)
        tp = np.zeros(1024, np.uint8)
        tp[:len(outs[i]["tile_palettes"])] = outs[i]["tile_palettes"]
        o.tile_palettes = tp
        o.palette = rgb5
        o.optimize()
        assert o.as_json() == (tmp_path / ("o%d.json" % i)).read_text(), i
    r = cli(str(tmp_path / "f0.png"), str(tmp_path / "x.json"), "--share", "%s=%s" % (tmp_path / "nope.png", tmp_path / "y.json"))
    assert r.returncode == 1 and "nope.png" in r.stdout
