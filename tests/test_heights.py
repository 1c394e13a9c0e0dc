"""Heights that are a multiple of 8 without being a power of two (256 x 224, the SNES frame; 256 x 240 with overscan).

ssimulacra2 halves a scale's height rounding up, so from scale 2 on a scale may end in a partial 4-row group or have an
odd number of rows (224: 224/112/56/28/14/7; 240: .../30/15/8; 200: .../50/25/13/7; 40: 40/20/10/5; 24: 24/12/6).
The heights below cover each of those shapes; the oracle admits every multiple of 8 in [8, 256]."""
import ctypes as C
import json
import os
import subprocess
import zlib
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = 1e-11
HEIGHTS = [24, 40, 56, 200, 224, 240, 248]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def image(h, variant=0):
    from snesimage_amd.synth import synth_image
    return synth_image(0x5EED0100 + h, 256, h, variant)


# ---- argument check: no device needed ------------------------------------------------------------------------------
def test_create_admits_every_multiple_of_eight():
    """Every multiple of 8 in [8, 256] passes the argument check (0 with a device, SNES_ERR_HIP without one); other
    heights are still SNES_ERR_ARG."""
    from snesimage_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros((264, 256, 4), np.uint8)
    p = buf.ctypes.data_as(_ffi._u8p)
    gpu = os.path.exists("/dev/kfd")
    for h in (24, 40, 200, 224, 240):
        ctx = C.c_void_p()
        rc = lib.snesimage_create(p, 256, h, 8, 15, 0, 0, C.byref(ctx))
        assert rc == (0 if gpu else -2), (h, rc, lib.snesimage_last_error())
        if rc == 0:
            lib.snesimage_destroy(ctx)
    for h in (0, 4, 100, 228, 264):
        ctx = C.c_void_p()
        assert lib.snesimage_create(p, 256, h, 8, 15, 0, 0, C.byref(ctx)) == -1, h
        assert b"multiple of 8" in lib.snesimage_last_error()


# ---- GPU: against the oracle and against the dense path ----------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


FLAGS = [({}, 4, 7), ({"perceptual": True}, 4, 7), ({"dither": True}, 4, 7), ({"nes": True}, 2, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("flags,count,size", FLAGS, ids=["rgb", "perceptual", "dither", "nes"])
def test_initialisers_maps_and_scores_match_oracle(S, O, h, flags, count, size):
    """k-means initialisers, optimize() and the JSON / RGBA bit-exact; error() and score_candidates within 1e-11."""
    for variant in (0, 1):  # variant 1 has transparent pixels
        img = image(h, variant)
        g, o = S.OptimizedImage(img, count, size, **flags), O.OracleImage(img, count, size, **flags)
        g.initialize_tiles()
        o.initialize_tiles()
        assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette, o.palette)
        assert np.array_equal(g.palette_map, o.palette_map)
        g.recalculate_palettes()
        o.recalculate_palettes()
        assert np.array_equal(g.palette, o.palette) and np.array_equal(g.palette_map, o.palette_map)
        g.optimize()
        assert np.array_equal(g.palette_map, o.palette_map)
        assert rel(g.error(), o.error()) < REL_ERR, (h, variant)
        cand = S.random_candidates(7, h + variant, 24)
        cand[0] = g.palette[1]
        for sp, si in ((0, 1), (count - 1, size - 1)):
            assert rel(g.score_candidates(sp, si, cand), o.score_candidates(sp, si, cand)) < REL_ERR, (h, variant, sp, si)
        assert g.as_json() == o.as_json()
        assert len(json.loads(g.as_json())["tiles"]) == 32 * (h // 8)
        assert np.array_equal(g.as_rgba(), o.as_rgba())
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS + [192])
@pytest.mark.parametrize("flags", [{}, {"perceptual": True}, {"dither": True}], ids=["rgb", "perceptual", "dither"])
def test_sparse_path_equals_dense_path(S, O, h, flags, monkeypatch):
    """The group-sparse path (partial last groups, odd scales) against the dense path bit for bit, a few against the
    oracle, and the slot windows against call-by-call stepping on the dense path."""
    img = image(h, 1 if h in (40, 224) else 0)
    monkeypatch.setenv("SNES_SPARSE", "0")
    dense = S.OptimizedImage(img, 4, 7, **flags)
    monkeypatch.setenv("SNES_SPARSE", "1")
    monkeypatch.setenv("SNES_SPARSE_MIN", "1")
    sparse = S.OptimizedImage(img, 4, 7, **flags)
    dense.initialize_tiles()
    dense.recalculate_palettes()
    sparse.tile_palettes, sparse.palette = dense.tile_palettes, dense.palette
    sparse.optimize()
    pal = dense.palette
    for (sp, si), n in (((1, 2), 150), ((3, 6), 40)):
        cand = S.random_candidates(13, sp * 7 + si + h, n)
        cand[0] = pal[sp * 7 + si]
        cand[1] = pal[sp * 7 + (si + 1) % 7]
        ed, es = dense.score_candidates(sp, si, cand), sparse.score_candidates(sp, si, cand)
        assert np.array_equal(ed, es), (h, sp, si, float(np.max(np.abs(ed - es))))
    o = O.OracleImage(img, 4, 7, **flags)
    o.tile_palettes, o.palette = dense.tile_palettes, dense.palette
    o.optimize()
    assert rel(es[:5], o.score_candidates(3, 6, cand[:5])) < REL_ERR
    sched = S.schedule(4, 7, 60)
    log, _, stats = sparse.run_slots(40, seed=3, first_step_id=20, state=sched[20][1:])
    for j in range(40):
        m, p, i, ch, _ = sched[20 + j]
        e, b = dense.step(m, p, i, ch, 3, 20 + j, 0)
        assert (e, b.tolist()) == (log[j][0], log[j][2].tolist()), (h, j)
    assert np.array_equal(dense.palette, sparse.palette) and np.array_equal(dense.palette_map, sparse.palette_map)
    dense.close()
    sparse.close()


@pytest.mark.gpu
@pytest.mark.parametrize("h", [224, 240])
def test_oracle_trajectory_through_every_loop(S, O, h):
    """100 scheduled calls of the oracle, replayed through the slot windows (adaptive and one call per window) and through
    step(): every call's colour exact and error within 1e-11, palette and palette_map identical after every replay."""
    count, size, calls, nr = 2, 3, 100, 16
    img = image(h, 1)
    o = O.OracleImage(img, count, size)
    o.initialize_tiles()
    o.recalculate_palettes()
    sched = S.schedule(count, size, calls)
    traj = []
    for j, (m, p, i, ch, _) in enumerate(sched):
        traj.append(o.step(m, p, i, ch, 9, j, nr if m == S.METHOD_RANDOM else 0))
    for mode in ("adaptive", "window1", "step"):
        g = S.OptimizedImage(img, count, size)
        g.initialize_tiles()
        g.recalculate_palettes()
        if mode == "step":
            got = [g.step(m, p, i, ch, 9, j, nr if m == S.METHOD_RANDOM else 0) for j, (m, p, i, ch, _) in enumerate(sched)]
        else:
            log, _, stats = g.run_slots(calls, seed=9, first_step_id=0, state=sched[0][1:], window=0 if mode == "adaptive" else 1, n_random=nr)
            assert stats["calls"] == calls
            got = [(e, rgb5) for e, _, rgb5, _ in log]
        for j, ((eg, bg), (eo, bo)) in enumerate(zip(got, traj)):
            assert np.array_equal(bg, bo), (mode, j)
            assert abs(eg - eo) <= REL_ERR * abs(eo), (mode, j, eg, eo)
        assert np.array_equal(g.palette, o.palette) and np.array_equal(g.palette_map, o.palette_map), mode
        assert g.as_json() == o.as_json()
        g.close()


@pytest.mark.gpu
def test_batch_mode_equals_one_image_at_a_time(S):
    from snesimage_amd.throughput import ImageBatch
    ids = [3, 4, 5, 6]
    imgs = [(gid, image(224, gid & 1) if gid != 6 else image(224, 0)[::-1].copy()) for gid in ids]
    batch = ImageBatch(imgs, 4, 7, candidates=24, host_threads=2, batched=True)
    batch.initialize()
    batch.run(5)
    sched = S.schedule(4, 7, 5)
    for pos, (gid, img) in enumerate(imgs):
        solo = S.OptimizedImage(img, 4, 7)
        solo.initialize_tiles()
        solo.recalculate_palettes()
        for j, (m, p, idx, ch, _) in enumerate(sched):
            e, _ = solo.step(m, p, idx, ch, 1 + gid, j, 24 if m == S.METHOD_RANDOM else 0)
        got = batch.images[pos]
        assert np.array_equal(got.palette, solo.palette) and np.array_equal(got.palette_map, solo.palette_map)
        assert batch.errors()[pos] == e
        solo.close()
    batch.close()


@pytest.mark.gpu
def test_split_phase_step_equals_plain_step(S):
    """step_begin / min-reduce / step_commit over two shards == step(), at 224 rows."""
    from hipmem import DeviceArray
    img = image(224, 1)
    ref = S.OptimizedImage(img, 8, 15)
    ref.initialize_tiles()
    ref.recalculate_palettes()
    shards = []
    for _ in range(2):
        s = S.OptimizedImage(img, 8, 15)
        s.tile_palettes, s.palette = ref.tile_palettes, ref.palette
        s.optimize()
        shards.append(s)
    for i, (p, idx) in enumerate([(0, 0), (3, 7), (7, 14)]):
        e_ref, b_ref = ref.step(S.METHOD_RANDOM, p, idx, 0, 4, i, 40)
        bufs = [DeviceArray(40, np.float64, fill=0) for _ in range(2)]
        for r, s in enumerate(shards):
            s.step_begin(S.METHOD_RANDOM, p, idx, 0, 4, i, 40, r, 2, bufs[r].ptr)
            s.sync()
        red = DeviceArray.from_numpy(np.minimum(bufs[0].numpy(), bufs[1].numpy()))
        for s in shards:
            s.step_commit(red.ptr)
            e, b, _ = s.last_step()
            assert e == e_ref and np.array_equal(b, b_ref)
            assert np.array_equal(s.palette, ref.palette) and np.array_equal(s.palette_map, ref.palette_map)
    for s in shards:
        s.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"perceptual": True}], ids=["rgb", "perceptual"])
def test_reassign_tiles_matches_oracle(S, O, flags):
    img = image(224, 1)
    g, o = S.OptimizedImage(img, 4, 7, **flags), O.OracleImage(img, 4, 7, **flags)
    g.initialize_tiles(); o.initialize_tiles()
    g.recalculate_palettes(); o.recalculate_palettes()
    for rnd in range(2):
        mg, mo = g.reassign_tiles(), o.reassign_tiles()
        assert mg == mo
        assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, o.palette_map)
        assert rel(g.error(), o.error()) < REL_ERR
        for i, (p, idx) in enumerate([(0, 0), (3, 6)]):
            eg, bg = g.step(S.METHOD_RANDOM, p, idx, 0, 3, 10 * rnd + i, 24)
            eo, bo = o.step(0, p, idx, 0, 3, 10 * rnd + i, 24)
            assert np.array_equal(bg, bo) and abs(eg - eo) <= REL_ERR * abs(eo)
    assert g.as_json() == o.as_json()
    g.close()


def write_png(path, rgba):
    """A minimal RGBA8 PNG (filter 0 on every row)."""
    h, w = rgba.shape[:2]
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                     chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
def test_cli_256x224_matches_oracle(tmp_path, O):
    """A 256 x 224 raw RGBA file through the CLI: the oracle's JSON after the same calls, byte for byte (28 x 32 tiles, and
    one tile palette per tile: the reference pushes them inside its tile loop, lib.rs:598-616); the same picture as a PNG
    gives the same JSON; --resume from that output starts where it ended."""
    count, size, calls, ncand = 4, 7, 9, 12
    img = image(224, 1)
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    out = tmp_path / "out.json"
    r = cli(str(src), str(out), "-c", str(count), "-s", str(size), "--calls", str(calls), "--candidates", str(ncand), "--seed", "5",
            "--preview", str(tmp_path / "p.png"))
    assert r.returncode == 0, r.stdout + r.stderr
    o = O.OracleImage(img, count, size)
    o.initialize_tiles()
    o.recalculate_palettes()
    for i, (m, p, idx, ch, _) in enumerate(O.schedule(count, size, calls)):
        o.step(m, p, idx, ch, 5, i, ncand if m == 0 else 0)
    text = out.read_text()
    assert text == o.as_json()
    doc = json.loads(text)
    assert len(doc["tiles"]) == 896 and len(doc["tile_palettes"]) == 896
    assert (tmp_path / "p.png").stat().st_size > 0
    png = tmp_path / "in.png"
    write_png(png, img)
    out2 = tmp_path / "out2.json"
    r = cli(str(png), str(out2), "-c", str(count), "-s", str(size), "--calls", str(calls), "--candidates", str(ncand), "--seed", "5")
    assert r.returncode == 0, r.stdout + r.stderr
    assert out2.read_text() == text
    out3 = tmp_path / "out3.json"
    r = cli(str(png), str(out3), "-c", str(count), "-s", str(size), "--calls", "0", "--resume", str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    assert out3.read_text() == text


@pytest.mark.gpu
@pytest.mark.parametrize("h", [200, 224, 240])
@pytest.mark.parametrize("flags", [{}, {"dither": True}], ids=["rgb", "dither"])
def test_group_sparse_storage_is_written_before_it_is_read(S, O, h, flags, monkeypatch):
    """The group-sparse storage starts as NaN bytes (snesimage_debug_poison_alloc) instead of what a fresh allocation
    happens to hold: B's groups that are padding only (224 rows: scale-1 groups 28-31, scale-2 groups 14-15, scale-3
    group 7) are read by every V sweep, so they must be computed, not found.  Scores, steps and slot windows against
    the oracle."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    monkeypatch.setenv("SNES_SPARSE", "1")
    monkeypatch.setenv("SNES_SPARSE_MIN", "1")
    L.snesimage_debug_poison_alloc(1)
    try:
        img = image(h, 1)
        o = O.OracleImage(img, 4, 7, **flags)
        o.initialize_tiles()
        o.recalculate_palettes()
        g = S.OptimizedImage(img, 4, 7, **flags)
        g.tile_palettes, g.palette = o.tile_palettes, o.palette
        g.optimize()
        cand = S.random_candidates(21, h, 100)
        cand[0] = o.palette[1 * 7 + 3]
        eg = g.score_candidates(1, 2, cand)
        assert np.isfinite(eg).all()
        assert rel(eg, o.score_candidates(1, 2, cand)) < REL_ERR, h
        sched = S.schedule(4, 7, 24)
        for j in range(4):
            m, p, i, ch, _ = sched[j]
            eg, bg = g.step(m, p, i, ch, 5, j, 16 if m == S.METHOD_RANDOM else 0)
            eo, bo = o.step(m, p, i, ch, 5, j, 16 if m == S.METHOD_RANDOM else 0)
            assert np.array_equal(bg, bo) and abs(eg - eo) <= REL_ERR * abs(eo), (h, j)
        log, _, _ = g.run_slots(20, seed=5, first_step_id=4, state=sched[4][1:], n_random=16)
        for j in range(20):
            m, p, i, ch, _ = sched[4 + j]
            eo, bo = o.step(m, p, i, ch, 5, 4 + j, 16 if m == S.METHOD_RANDOM else 0)
            assert np.array_equal(log[j][2], bo) and abs(log[j][0] - eo) <= REL_ERR * abs(eo), (h, j)
        assert np.array_equal(g.palette, o.palette) and np.array_equal(g.palette_map, o.palette_map)
        g.close()
    finally:
        L.snesimage_debug_poison_alloc(0)
