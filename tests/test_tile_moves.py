"""Tile moves decided by the objective (snesimage_score_tile_moves, snesimage_tile_step, snesimage_tile_sweep): a tile goes
to another subpalette when error() itself, dithering included, is strictly lower there.  The model is tests/tile_model.py
over the unchanged CPU oracle; maps, tile palettes and JSON are compared exactly, errors within 1e-11 relative, product
against product (window sizes, poisoned storage) bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tile_model import (REL_ERR, assert_log_matches, check_gap, make_pair, model_candidate, model_tile_sweep, run_slots_both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
TILE_FUNCS = ["snesimage_score_tile_moves", "snesimage_tile_step", "snesimage_tile_sweep", "snesimage_shared_tile_sweep"]


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


# ---- without a device ----------------------------------------------------------------------------------------------------

def test_tile_symbols_exported_and_declared():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in TILE_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    assert "snesimage_tile_result" in text
    assert C.sizeof(_ffi.TileResult) == 16
    e = (C.c_double * 1)()
    t, s = (C.c_uint16 * 1)(), (C.c_uint8 * 1)()
    assert lib.snesimage_score_tile_moves(None, t, s, 1, e, None) == -1 and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_tile_step(None, 0, None) == -1
    assert lib.snesimage_tile_sweep(None, 0, 1, 0, None, None) == -1
    assert lib.snesimage_shared_tile_sweep(None, 0, 1, 0, None, None) == -1


def test_cli_tile_moves_argument_rules(tmp_path):
    """Refused while parsing: the source does not exist, so a refusal after any file or device access would exit 1."""
    missing, out = str(tmp_path / "none.png"), str(tmp_path / "o.json")
    r = cli("--help")
    assert r.returncode == 0 and "--tile-moves" in r.stderr and "--reassign-tiles" in r.stderr.split("--tile-moves", 1)[1]
    for extra, name in [(["--devices", "0,1"], "--devices"), (["--reassign-tiles", "1"], "--reassign-tiles")]:
        r = cli(missing, out, "--tile-moves", "1", *extra)
        assert r.returncode == 2, extra
        assert "cannot be used with" in r.stderr and name in r.stderr and "--tile-moves" in r.stderr, r.stderr
    r = cli(missing, out, "--tile-moves")
    assert r.returncode == 2 and "--tile-moves" in r.stderr
    assert not os.path.exists(out)


# ---- on the MI355X -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def image(alpha, h):
    from snesimage_amd.synth import synth_image
    return np.ascontiguousarray((synth_image(0x5EED0001, variant=1) if alpha else synth_image())[:h])


def state_of(g):
    return g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.palette.tobytes(), g.error()


def model_scores(o, pairs, inc):
    """{(tile, sub): (error, map)} for the distinct pairs; a pair naming the tile's subpalette is the state itself."""
    tp, out = o.tile_palettes, {}
    for t, k in sorted(set(pairs)):
        if k == tp[t]:
            out[(t, k)] = (inc, o.palette_map)
        else:
            out[(t, k)] = model_candidate(o, t, k)
            check_gap(out[(t, k)][0], inc)
    return out


def random_pairs(rng, n, ntile, count, pool):
    """n pairs in arbitrary order, with repeats, drawn from `pool` distinct ones (the model evaluates each once)."""
    base = [(int(rng.integers(ntile)), int(rng.integers(count))) for _ in range(pool)]
    return [base[int(i)] for i in rng.integers(len(base), size=n)]


def check_scores(g, o, pairs, want_maps):
    inc = o.error()
    want = model_scores(o, pairs, inc)
    before = state_of(g)
    tiles, subs = [p[0] for p in pairs], [p[1] for p in pairs]
    if want_maps:
        errs, maps = g.score_tile_moves(tiles, subs, want_maps=True)
    else:
        errs, maps = g.score_tile_moves(tiles, subs), None
    cur = g.tile_palettes
    for j, p in enumerate(pairs):
        e, m = want[p]
        assert abs(errs[j] - e) <= REL_ERR * abs(e), (j, p, errs[j], e)
        if maps is not None:
            assert np.array_equal(maps[j], m), (j, p)
        if p[1] == cur[p[0]]:
            assert errs[j] == before[3], (j, p)  # the incumbent, bit for bit
    assert state_of(g) == before  # as if the call had not been made


@pytest.mark.gpu
@pytest.mark.parametrize("flags,count,size,h,alpha,slots", [
    ({}, 4, 7, 64, False, 0),
    ({}, 8, 15, 224, True, 12),
    ({}, 2, 3, 224, False, 0),
    ({"perceptual": True}, 2, 3, 64, True, 12),
    ({"perceptual": True}, 4, 7, 224, False, 0),
    ({"dither": True}, 4, 7, 64, True, 0),
    ({"dither": True}, 4, 1, 64, False, 12),
    ({"dither": True}, 8, 15, 224, False, 12),
    ({"dither": True, "perceptual": True}, 2, 3, 64, False, 12),
    ({"dither": True, "perceptual": True}, 4, 7, 64, True, 0),
    ({"nes": True}, 4, 3, 64, False, 12),
])
def test_score_tile_moves_matches_model(S, O, flags, count, size, h, alpha, slots):
    """Errors and maps_out of explicit (tile, subpalette) pairs — every distance, with and without --dither, geometries from
    4 x 1 to 8 x 15, 64 and 224 rows, straight after the k-means start and after a dozen scheduled calls — and a following
    step that goes as if nothing had happened."""
    img = image(alpha, h)
    g, o = make_pair(S, O, img, count, size, flags, slots=slots)
    ntile = 32 * (h // 8)
    rng = np.random.default_rng(7)
    tp = g.tile_palettes
    pairs = random_pairs(rng, 40, ntile, count, 14) + [(5, int(tp[5])), (ntile - 1, int(tp[ntile - 1]))]
    check_scores(g, o, pairs, want_maps=True)
    check_scores(g, o, pairs[:3], want_maps=False)
    run_slots_both(S, g, o, count, size, slots, 3, bool(flags.get("nes")))
    assert g.as_json() == o.as_json()
    g.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"dither": True}], ids=["rgb", "dither"])
def test_score_tile_moves_list_lengths(S, O, flags, monkeypatch):
    """Lists of 3, 100 and 1,100 pairs: one launch group and several (set_chunk(512): 512 + 512 + 76), and with --dither both
    forms of the Floyd-Steinberg kernel (a quad of lanes per row up to 64 runs per launch here, a lane per row beyond)."""
    monkeypatch.setenv("SNES_DITHER4_MAX", "64")
    count, size, h = 4, 7, 64
    g, o = make_pair(S, O, image(False, h), count, size, flags)
    g.set_chunk(512)
    rng = np.random.default_rng(11)
    for n, pool in ((3, 3), (100, 20), (1100, 30)):
        check_scores(g, o, random_pairs(rng, n, 32 * (h // 8), count, pool), want_maps=(n == 100))
    g.close()
    o.close()


def sweep_from(S, g0, img, count, size, flags, first, n, window):
    """A fresh context in g0's state, swept; -> (log, stats, state)."""
    g = S.OptimizedImage(img, count, size, **flags)
    g.tile_palettes, g.palette = g0.tile_palettes, g0.palette
    g.optimize()
    log, stats = g.tile_sweep(first, n, window)
    out = log, stats, state_of(g), g.as_json()
    g.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flags,count,size,h,alpha,reassign", [
    ({}, 4, 7, 64, False, False),
    ({}, 4, 7, 64, True, False),
    ({"perceptual": True}, 4, 7, 32, False, False),
    ({"dither": True}, 3, 3, 32, False, True),
    ({"dither": True, "perceptual": True}, 3, 3, 32, False, False),
], ids=["rgb", "rgb_alpha", "perceptual", "dither_after_reassign", "dither_perceptual"])
def test_tile_sweep_windows_equal_call_by_call_and_the_model(S, O, flags, count, size, h, alpha, reassign):
    """48 tile calls with window 1, 0, 7 and 64 from identical states: identical logs and states bit for bit, equal to the
    model (accepted tiles and their subpalettes exactly, errors within 1e-11); at least 3 accepted and 20 rejected calls."""
    img = image(alpha, h)
    g0, o = make_pair(S, O, img, count, size, flags)
    if reassign:
        while True:
            mg, mo = g0.reassign_tiles(), o.reassign_tiles()
            assert mg == mo
            if not mg:
                break
    n = 48
    want = model_tile_sweep(o, 0, n, count)
    accepted = sum(ch for _, _, ch in want)
    assert accepted >= 3 and n - accepted >= 20, "the input no longer exercises the windows: %d accepted" % accepted
    ref = None
    for window in (1, 0, 7, 64):
        log, stats, state, js = sweep_from(S, g0, img, count, size, flags, 0, n, window)
        assert_log_matches(log, want)
        assert np.all(np.diff(log["error"]) <= 0.0)
        assert stats["calls"] == n and stats["accepted"] == accepted and stats["voided"] == 0
        assert stats["useful"] == n * (count - 1) and stats["useful"] <= stats["scored"]
        if window == 1:
            assert stats["windows"] == n and stats["scored"] == stats["useful"]
            ref = (log.tobytes(), state, js)
        else:
            assert stats["windows"] < stats["calls"], (window, stats)
            assert (log.tobytes(), state, js) == ref, window
    assert ref[1][0] == o.tile_palettes.tobytes() and ref[1][1] == o.palette_map.tobytes() and ref[2] == o.as_json()
    assert abs(ref[1][3] - o.error()) <= REL_ERR * o.error()
    # tile_step is a sweep of one
    g = S.OptimizedImage(img, count, size, **flags)
    g.tile_palettes, g.palette = g0.tile_palettes, g0.palette
    g.optimize()
    steps = [g.tile_step(t) for t in range(n)]
    assert [(e, s, c) for e, s, c in steps] == [(float(r["error"]), int(r["sub"]), int(r["changed"])) for r in np.frombuffer(ref[0], dtype=S.api.TILE_LOG_DTYPE)]
    assert state_of(g) == ref[1]
    g.close()
    g0.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"dither": True}], ids=["rgb", "dither"])
def test_equal_errors_are_not_taken(S, O, flags):
    """(a) Two identical subpalettes: moving a tile between them changes nothing, e_k == incumbent exactly, never taken.
    (b) Tiles without an opaque pixel (the transparent square of the alpha image: tiles tx, ty in 12..19 at 160 rows)."""
    count, size, h = 4, 7, 160
    img = image(True, h)
    assert not img[96:160, 96:160, 3].any() and img[:96, :, 3].all()
    g, o = make_pair(S, O, img, count, size, flags)
    pal = g.palette
    pal[size:2 * size] = pal[:size]  # subpalette 1 := subpalette 0
    g.palette = pal
    o.palette = pal
    g.optimize()
    o.optimize()
    inc = g.error()
    assert abs(inc - o.error()) <= REL_ERR * inc
    tp = g.tile_palettes
    twins = [t for t in range(32 * (h // 8)) if tp[t] in (0, 1)][:6]
    holes = [ty * 32 + tx for ty in (12, 15, 19) for tx in (12, 19)]
    assert len(twins) == 6
    pairs = [(t, 1 - int(tp[t])) for t in twins] + [(t, k) for t in holes for k in range(count)]
    errs = g.score_tile_moves([p[0] for p in pairs], [p[1] for p in pairs])
    assert (errs == inc).all(), errs - inc
    for t, k in pairs[:3] + pairs[6:9]:
        assert model_candidate(o, t, k)[0] == o.error()  # the oracle agrees: a difference of exactly 0
    # a window does not stop at such tiles: row 12 of tiles, the transparent ones in the middle
    before = state_of(g)
    log, stats = g.tile_sweep(12 * 32 + 8, 16, 64)
    want = model_tile_sweep(o, 12 * 32 + 8, 16, count)
    assert_log_matches(log, want)
    assert not log["changed"][4:12].any() and (log["error"][4:12] == log["error"][3]).all()
    if not log["changed"].any():
        assert stats["windows"] == 1 and state_of(g) == before
    for t in twins:  # the twin subpalette is never preferred
        e, sub, ch = g.tile_step(t)
        assert sub != 1 - int(tp[t])
    g.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"dither": True}], ids=["rgb", "dither"])
def test_interleaving_with_the_other_entry_points_matches_the_oracle(S, O, flags):
    """run_slots 12 calls -> tile_sweep (32 tiles) -> reassign_tiles -> tile_sweep -> run_slots 12 calls; as_json() equal."""
    count, size, h = 4, 7, 64
    img = image(False, h)
    g, o = make_pair(S, O, img, count, size, flags, slots=12)
    for rnd in range(2):
        log, _ = g.tile_sweep(8, 32)
        assert_log_matches(log, model_tile_sweep(o, 8, 32, count))
        assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, o.palette_map)
        assert abs(g.error() - o.error()) <= REL_ERR * o.error()
        if rnd == 0:
            assert g.reassign_tiles() == o.reassign_tiles()
    run_slots_both(S, g, o, count, size, 12, 12)
    assert g.as_json() == o.as_json()
    g.close()
    o.close()


@pytest.mark.gpu
def test_tile_sweep_refused_between_the_phases_of_a_step(S, img256):
    from hipmem import DeviceArray
    img = np.ascontiguousarray(img256[:64])
    g = S.OptimizedImage(img, 4, 7)
    ref = S.OptimizedImage(img, 4, 7)
    for x in (g, ref):
        x.initialize_tiles()
        x.recalculate_palettes()
    e_ref, b_ref = ref.step(S.METHOD_RANDOM, 1, 2, 0, 4, 0, 40)
    buf = DeviceArray(40, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 1, 2, 0, 4, 0, 40, 0, 1, buf.ptr)
    for call in (lambda: g.tile_sweep(0, 4), lambda: g.tile_step(0), lambda: g.score_tile_moves([0], [1])):
        with pytest.raises(S.SnesImageError) as ei:
            call()
        assert ei.value.code == -3
    g.step_commit(buf.ptr)
    e, b, _ = g.last_step()
    assert e == e_ref and np.array_equal(b, b_ref) and np.array_equal(g.palette_map, ref.palette_map)
    log, _ = g.tile_sweep(0, 4)  # and afterwards it is welcome
    log_ref, _ = ref.tile_sweep(0, 4)
    assert log.tobytes() == log_ref.tobytes()
    g.close()
    ref.close()


@pytest.mark.gpu
def test_tile_argument_refusals_and_one_subpalette(S, img256):
    img = np.ascontiguousarray(img256[:64])
    g = S.OptimizedImage(img, 4, 7)
    g.initialize_tiles()
    g.recalculate_palettes()
    for call in (lambda: g.tile_sweep(250, 7), lambda: g.tile_sweep(257, 0), lambda: g.tile_step(256), lambda: g.score_tile_moves([0], [4]),
                 lambda: g.score_tile_moves([256], [0])):
        with pytest.raises(S.SnesImageError) as ei:
            call()
        assert ei.value.code == -1
    before = state_of(g)
    log, stats = g.tile_sweep(250, 6)
    assert len(log) == 6 and stats["calls"] == 6
    g.close()
    one = S.OptimizedImage(img, 1, 7, dither=True)
    one.initialize_tiles()
    one.recalculate_palettes()
    before = state_of(one)
    log, stats = one.tile_sweep()
    assert len(log) == 256 and not log["changed"].any() and (log["error"] == before[3]).all() and (log["sub"] == 0).all()
    assert stats["accepted"] == 0 and stats["scored"] == 0 and state_of(one) == before
    one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("h", [64, 200])
def test_tile_sweep_reads_no_storage_nobody_wrote(S, h):
    """The workspace starts as 0xff bytes (snesimage_debug_poison_alloc): the same log as from plain storage."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    count, size = 4, 7
    img = image(True, h)
    logs = []
    for poison in (0, 1):
        L.snesimage_debug_poison_alloc(poison)
        try:
            for flags in ({}, {"dither": True}):
                g = S.OptimizedImage(img, count, size, **flags)
                g.initialize_tiles()
                g.recalculate_palettes()
                log, _ = g.tile_sweep(0, 40, 8)
                logs.append((poison, log.tobytes(), state_of(g)))
                g.close()
        finally:
            L.snesimage_debug_poison_alloc(0)
    assert logs[0][1:] == logs[2][1:] and logs[1][1:] == logs[3][1:]
    assert np.isfinite(np.frombuffer(logs[2][1], dtype=S.api.TILE_LOG_DTYPE)["error"]).all()


@pytest.mark.gpu
def test_failed_tile_workspace_allocation_leaves_the_context_usable(S, img256):
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = np.ascontiguousarray(img256[:64])
    count, size = 4, 7
    ref = S.OptimizedImage(img, count, size)
    ref.initialize_tiles()
    ref.recalculate_palettes()
    g = S.OptimizedImage(img, count, size)
    g.tile_palettes, g.palette = ref.tile_palettes, ref.palette
    g.optimize()
    g.error()
    before = state_of(g)
    failures = 0
    for nth in (0, 1, 4, 9, 15, 22, 40):
        L.snesimage_debug_fail_alloc(nth)
        try:
            g.tile_sweep(0, 48)
            ok = True
        except S.SnesImageError as e:
            assert e.code == -2
            ok = False
            failures += 1
        finally:
            L.snesimage_debug_fail_alloc(-1)
        if ok:
            break
        assert state_of(g) == before
    assert failures >= 3
    g.tile_palettes, g.palette = ref.tile_palettes, ref.palette
    g.optimize()
    log, _ = g.tile_sweep(0, 48)
    want, _ = ref.tile_sweep(0, 48, 1)
    assert log.tobytes() == want.tobytes() and state_of(g) == state_of(ref)
    g.close()
    ref.close()
