"""Palette blocks (snesimage_set_palette_blocks and the block calls; include/snesimage_hip.h: "Palette blocks"): one
subpalette per block of bw x bh tiles.  The model is tests/block_model.py over the unchanged CPU oracle, the cases are
tests/block_cases.py; tables, palettes, maps and JSON are compared exactly, errors within REL_ERR, product against product
(window sizes, poisoned storage, the tile calls at 1 x 1) bit for bit."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import block_cases as BC
import block_model as BM
from block_model import REL_ERR, check_gap
from tile_model import assert_log_matches, run_slots_both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
BLOCK_FUNCS = ["snesimage_set_palette_blocks", "snesimage_get_palette_blocks", "snesimage_score_block_moves", "snesimage_block_step", "snesimage_block_sweep"]
ARG, STATE, UNSUPPORTED = -1, -3, -5


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


# ---- without a device ----------------------------------------------------------------------------------------------------

def test_block_symbols_exported_and_declared():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in BLOCK_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    e, b, s = (C.c_double * 1)(), (C.c_uint16 * 1)(), (C.c_uint8 * 1)()
    w, h = C.c_uint32(0), C.c_uint32(0)
    assert lib.snesimage_set_palette_blocks(None, 2, 2) == ARG and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_get_palette_blocks(None, C.byref(w), C.byref(h)) == ARG
    assert lib.snesimage_score_block_moves(None, b, s, 1, e, None) == ARG and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_block_step(None, 0, None) == ARG
    assert lib.snesimage_block_sweep(None, 0, 1, 0, None, None) == ARG


def test_cli_palette_blocks_argument_rules(tmp_path):
    """Refused while parsing: the source does not exist, so a refusal after any file or device access would exit 1."""
    missing, out = str(tmp_path / "none.png"), str(tmp_path / "o.json")
    r = cli("--help")
    assert r.returncode == 0 and "--palette-blocks" in r.stderr and "--resume" in r.stderr.split("--palette-blocks", 1)[1].split("--guided", 1)[0]
    three = ["--import-cgram", "a", "--import-chr", "b", "--import-map", "c"]
    for extra, name in [(["--share", "a.png=b.json"], "--share"), (["--devices", "0,1"], "--devices"), (three, "--import-cgram")]:
        r = cli(missing, out, "--palette-blocks", "2x2", *extra)
        assert r.returncode == 2, (extra, r.stderr)
        assert "cannot be used with" in r.stderr and name in r.stderr and "--palette-blocks" in r.stderr, r.stderr
    for bad in ("3x2", "2x", "2x2x2", "16x1", "0x1", "x", "2,2"):
        r = cli(missing, out, "--palette-blocks", bad)
        assert r.returncode == 2 and "invalid value" in r.stderr and "--palette-blocks" in r.stderr, (bad, r.stderr)
    r = cli(missing, out, "--palette-blocks")
    assert r.returncode == 2 and "--palette-blocks" in r.stderr
    assert not os.path.exists(out)


def test_cli_block_height_must_divide_the_rows_of_tiles(tmp_path):
    """Known once the image is read, said before any device is touched (this runs without one): 256 x 24 has three rows of tiles."""
    src, out = tmp_path / "in.rgba", str(tmp_path / "o.json")
    src.write_bytes(BC.image("synth", 24).tobytes())
    r = cli(str(src), out, "-c", "2", "-s", "3", "--palette-blocks", "2x2")
    assert r.returncode == 2 and "invalid value" in r.stderr and "3 rows of tiles" in r.stderr, r.stderr
    assert not os.path.exists(out)


# ---- on the MI355X -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def state_of(g):
    return g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.palette.tobytes(), g.error()


def product(S, img, count, size, bw, bh, flags, init=True):
    g = S.OptimizedImage(img, count, size, **flags)
    g.palette_blocks = (bw, bh)
    if init:
        g.initialize_tiles()
        g.recalculate_palettes()
    return g


def assert_same_state(g, o, count, size, flags):
    assert np.array_equal(g.tile_palettes, o.tile_palettes)
    assert np.array_equal(g.palette, BC.regular(o, count, size, flags))
    assert np.array_equal(g.palette_map, o.palette_map)
    e = o.error()
    print("error: product %r model %r rel %.3e" % (g.error(), e, abs(g.error() - e) / e))
    assert abs(g.error() - e) <= REL_ERR * e


def refused(S, call, code, *words):
    with pytest.raises(S.SnesImageError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def refused_untouched(S, g, call, code, *words):
    """The call is refused and tile_palettes, map, palette, error() and the granularity are bit-equal straight afterwards."""
    before, blocks = state_of(g), g.palette_blocks
    refused(S, call, code, *words)
    assert state_of(g) == before and g.palette_blocks == blocks


def set_blocks(g, v):
    return lambda: setattr(g, "palette_blocks", v)


@pytest.mark.gpu
def test_setter_getter_and_every_refusal_leave_the_state(S):
    """Every refusal of the contract, each followed at once by a comparison of tile_palettes, map, palette and error().  While
    a split-phase step or window is pending the map and the error cannot be read, so the table and the palette are compared
    at once and the whole state after the commit, against a twin context that went through the same phases unprovoked."""
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = BC.image("synth", 48)
    count, size = 4, 3
    g, twin = S.OptimizedImage(img, count, size), S.OptimizedImage(img, count, size)
    assert g.palette_blocks == (1, 1)
    for bad in ((3, 2), (2, 0), (16, 1), (2, 3), (0, 0), (5, 5)):
        refused_untouched(S, g, set_blocks(g, bad), ARG)
    refused_untouched(S, g, set_blocks(g, (2, 4)), ARG, "6 rows")  # 48 rows: bh 4 does not divide 6
    for x in (g, twin):
        x.initialize_tiles()  # per tile
        x.recalculate_palettes()
    mixed = BM.mixed_blocks(g.tile_palettes, 48, 2, 2)
    assert mixed
    refused_untouched(S, g, set_blocks(g, (2, 2)), STATE, "snesimage_initialize_tiles", "block %d " % mixed[0])
    # a pending split-phase step and a pending split-phase window
    buf, tbuf = DeviceArray(40, np.float64, fill=0), DeviceArray(40, np.float64, fill=0)
    for x, b in ((g, buf), (twin, tbuf)):
        x.step_begin(S.METHOD_RANDOM, 1, 2, 0, 4, 0, 40, 0, 1, b.ptr)
    table, pal = g.tile_palettes.tobytes(), g.palette.tobytes()
    refused(S, set_blocks(g, (1, 2)), STATE, "pending")
    assert g.tile_palettes.tobytes() == table and g.palette.tobytes() == pal and g.palette_blocks == (1, 1)
    for x, b in ((g, buf), (twin, tbuf)):
        x.step_commit(b.ptr)
    assert state_of(g) == state_of(twin)
    taken = [x.slots_begin(4, 1, 1, (0, 1, 0, 0))[0] for x in (g, twin)]
    table, pal = g.tile_palettes.tobytes(), g.palette.tobytes()
    refused(S, set_blocks(g, (1, 2)), STATE, "pending")
    assert g.tile_palettes.tobytes() == table and g.palette.tobytes() == pal and g.palette_blocks == (1, 1)
    for x, n in zip((g, twin), taken):
        x.slots_commit(0, n)
    assert state_of(g) == state_of(twin)
    arr = (C.c_void_p * 1)(g._c)
    # a tied table is welcome; the setter changes nothing else
    tied = g.tile_palettes
    for b in range(BM.n_blocks(48, 2, 2)):
        tied[BM.block_tiles(b, 2, 2)] = tied[BM.block_tiles(b, 2, 2)[0]]
    g.tile_palettes = tied
    g.optimize()
    before = state_of(g)
    g.palette_blocks = (2, 2)
    assert g.palette_blocks == (2, 2) and state_of(g) == before
    # on the blocked context
    untied = tied.copy()
    untied[BM.block_tiles(7, 2, 2)[3]] ^= 1
    untied[BM.block_tiles(30, 2, 2)[1]] ^= 1
    refused_untouched(S, g, lambda: setattr(g, "tile_palettes", untied), ARG, "block 7 ")
    refused_untouched(S, g, set_blocks(g, (4, 1)), STATE, "block ")  # tied for 2 x 2 is not tied for 4 x 1
    refused_untouched(S, g, lambda: g.score_tile_moves([0], [1]), UNSUPPORTED, "snesimage_score_block_moves")
    refused_untouched(S, g, lambda: g.tile_step(0), UNSUPPORTED, "snesimage_block_step")
    refused_untouched(S, g, lambda: g.tile_sweep(0, 4), UNSUPPORTED, "snesimage_block_sweep")
    nat = g.export_native()
    refused_untouched(S, g, lambda: g.import_native(nat["cgram"], nat["chr"], nat["map"]), UNSUPPORTED, "snesimage_import_native")
    for fn in (L.snesimage_batch_create, L.snesimage_group_create, L.snesimage_shared_create):
        out = C.c_void_p()
        assert fn(arr, 1, C.byref(out)) == UNSUPPORTED and not out.value
        assert b"snesimage_set_palette_blocks" in L.snesimage_last_error()
        assert state_of(g) == before
    bd = S.OptimizedImage(img, count, size, backdrop=True)
    bd.palette_blocks = (2, 2)
    bd_before = state_of(bd)
    out = C.c_void_p()
    assert L.snesimage_shared_create_backdrop((C.c_void_p * 1)(bd._c), 1, None, C.byref(out)) == UNSUPPORTED and not out.value
    assert b"snesimage_set_palette_blocks" in L.snesimage_last_error() and state_of(bd) == bd_before
    bd.close()
    refused_untouched(S, g, lambda: g.block_sweep(44, 5), ARG)  # 48 blocks
    refused_untouched(S, g, lambda: g.score_block_moves([48], [0]), ARG)
    refused_untouched(S, g, lambda: g.score_block_moves([0], [count]), ARG)
    # entries behind the image's tiles are not judged
    behind = tied.copy()
    behind[32 * 6:] = np.arange(1024 - 32 * 6) % count
    g.tile_palettes = behind
    assert np.array_equal(g.tile_palettes, behind)
    g.tile_palettes = tied
    g.optimize()
    assert state_of(g) == before
    # 1 x 1 switches blocking off
    g.palette_blocks = (1, 1)
    assert state_of(g) == before
    g.tile_step(0)
    g.close()
    twin.close()


@pytest.mark.gpu
def test_setter_is_refused_on_a_context_lent_to_a_batch_a_set_or_a_group(S):
    """SNES_ERR_STATE while lent, the table compared at once and the whole state once the context is its own again."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    g = S.OptimizedImage(BC.image("synth", 16), 2, 3)
    g.initialize_tiles()
    g.recalculate_palettes()
    before = state_of(g)
    arr = (C.c_void_p * 1)(g._c)
    for create, destroy in ((L.snesimage_batch_create, L.snesimage_batch_destroy), (L.snesimage_shared_create, L.snesimage_shared_destroy),
                            (L.snesimage_group_create, L.snesimage_group_destroy)):
        hnd = C.c_void_p()
        assert create(arr, 1, C.byref(hnd)) == 0, L.snesimage_last_error()
        table = g.tile_palettes.tobytes()
        refused(S, set_blocks(g, (1, 2)), STATE, "lent")
        assert g.tile_palettes.tobytes() == table and g.palette_blocks == (1, 1)
        destroy(hnd)
        assert state_of(g) == before
    g.palette_blocks = (1, 1)
    g.close()


@pytest.mark.gpu
def test_blocked_initialiser_counts_blocks_and_one_subpalette_is_unchanged(S, O):
    """cogset's 2 <= k < n counts blocks: 256 x 64 at 8 x 8 has four, so four subpalettes are SNES_ERR_KMEANS (per tile the same
    geometry starts) and the context is untouched.  sub_count == 1 on a blocked context is the unblocked initialiser."""
    img = BC.image("synth", 64)
    g = S.OptimizedImage(img, 4, 3)
    g.palette_blocks = (8, 8)
    refused_untouched(S, g, g.initialize_tiles, -4, "2 <= k < n")
    g.palette_blocks = (1, 1)
    g.initialize_tiles()
    g.close()
    one, plain, o = S.OptimizedImage(img, 1, 7), S.OptimizedImage(img, 1, 7), O.OracleImage(img, 1, 7)
    one.palette_blocks = (8, 8)
    for x in (one, plain, o):
        x.initialize_tiles()
    assert state_of(one) == state_of(plain)
    assert np.array_equal(one.palette, o.palette) and np.array_equal(one.palette_map, o.palette_map) and not one.tile_palettes.any()
    log, stats = one.block_sweep()
    assert len(log) == 4 and not log["changed"].any() and stats["scored"] == 0 and state_of(one) == state_of(plain)
    for x in (one, plain, o):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,h,count,size,bw,bh,flags,kind", BC.CASES, ids=BC.CASE_IDS)
def test_initialize_and_reassign_match_the_model(S, O, name, h, count, size, bw, bh, flags, kind):
    """Table, palette and map exactly, the error within REL_ERR, `moved` equal — after the blocked initialiser, after
    recalculate_palettes and after the blocked reassignment."""
    img = BC.image(kind, h, bw, bh)
    g = product(S, img, count, size, bw, bh, flags, init=False)
    if kind == "holes":  # blocks left out keep what they had
        tp = np.zeros(1024, np.uint8)
        tp[:32 * (h // 8)] = 3
        g.tile_palettes = tp
    g.initialize_tiles()
    if kind != "holes":
        o = BC.model_start(O, img, count, size, bw, bh, flags, recalc=False)
    else:
        o = O.OracleImage(img, count, size)
        o.tile_palettes = tp
        BM.model_initialize_tiles(O, o, img, bw, bh)
        for key in ("transparent", "black"):
            assert (g.tile_palettes[BM.block_tiles(BC.HOLE_BLOCKS[key], bw, bh)] == 3).all()
    assert np.array_equal(g.tile_palettes, o.tile_palettes) and BM.is_tied(g.tile_palettes, h, bw, bh)
    assert np.array_equal(g.palette, BC.regular(o, count, size, flags))
    if not flags.get("backdrop"):  # (the expanded oracle is in the initialiser's state only once the regular entries are final)
        assert_same_state(g, o, count, size, flags)
    g.recalculate_palettes()
    if flags.get("backdrop"):
        o.close()
        o = BC.model_start(O, img, count, size, bw, bh, flags)
    else:
        o.recalculate_palettes()
    assert_same_state(g, o, count, size, flags)
    moved = BM.model_reassign(O, o, img, bw, bh, bool(flags.get("perceptual")))
    assert g.reassign_tiles() == moved and moved % (bw * bh) == 0
    assert_same_state(g, o, count, size, flags)
    assert BM.is_tied(g.tile_palettes, h, bw, bh)
    g.close()
    o.close()


def model_scores(o, pairs, inc, bw, bh):
    """{(block, sub): (error, map)} for the distinct pairs; a pair naming the block's subpalette is the state itself."""
    tp, out = o.tile_palettes, {}
    for b, k in sorted(set(pairs)):
        if k == tp[BM.block_tiles(b, bw, bh)[0]]:
            out[(b, k)] = (inc, o.palette_map)
        else:
            out[(b, k)] = BM.model_block_candidate(o, b, k, bw, bh)
            check_gap(out[(b, k)][0], inc)
    return out


def check_scores(g, o, pairs, bw, bh):
    inc = o.error()
    want = model_scores(o, pairs, inc, bw, bh)
    before = state_of(g)
    errs, maps = g.score_block_moves([p[0] for p in pairs], [p[1] for p in pairs], want_maps=True)
    cur = g.tile_palettes
    for j, p in enumerate(pairs):
        e, m = want[p]
        print("pair %r: product %r model %r rel %.3e" % (p, errs[j], e, abs(errs[j] - e) / e))
        assert abs(errs[j] - e) <= REL_ERR * abs(e), (j, p, errs[j], e)
        assert np.array_equal(maps[j], m), (j, p)
        if p[1] == cur[BM.block_tiles(p[0], bw, bh)[0]]:
            assert errs[j] == before[3], (j, p)  # the incumbent, bit for bit
    assert np.array_equal(g.score_block_moves([p[0] for p in pairs[:3]], [p[1] for p in pairs[:3]]), errs[:3])
    assert state_of(g) == before  # as if the call had not been made


@pytest.mark.gpu
@pytest.mark.parametrize("name,h,count,size,bw,bh,flags,kind", BC.CASES, ids=BC.CASE_IDS)
def test_score_block_moves_matches_the_model(S, O, name, h, count, size, bw, bh, flags, kind):
    """Random pairs with repeats, the first and the last block and pairs naming the current subpalette: straight after the
    start, and after a dozen scheduled calls (thirteen on the backdrop row: its schedule's backdrop slot included; none at
    256 x 224, which takes a handful of pairs only)."""
    img = BC.image(kind, h, bw, bh)
    g = product(S, img, count, size, bw, bh, flags)
    o = BC.model_start(O, img, count, size, bw, bh, flags)
    nb = BM.n_blocks(h, bw, bh)
    rng = np.random.default_rng(11)
    pool = 4 if h == 224 else 8

    def pairs_now():
        tp = g.tile_palettes
        base = [(int(rng.integers(nb)), int(rng.integers(count))) for _ in range(pool)]
        first, last = int(tp[0]), int(tp[BM.block_tiles(nb - 1, bw, bh)[0]])
        return [base[int(i)] for i in rng.integers(len(base), size=2 * pool)] + [(0, first), (nb - 1, last), (0, (first + 1) % count), (nb - 1, (last + 1) % count)]

    check_scores(g, o, pairs_now(), bw, bh)
    table = g.tile_palettes.tobytes()
    if flags.get("backdrop"):  # the backdrop schedule: the twelve regular slots and the backdrop slot, on the expanded oracle
        import backdrop_model as BD
        m = BD.Model(O, img, count, size, BC.oracle_flags(flags), init="none")
        m.o.tile_palettes = o.tile_palettes
        m.set_state(BC.regular(o, count, size, flags), BC.mean_backdrop(O, img, flags))
        o.close()
        o = m.o
        g.run_slots(13, seed=5, first_step_id=0, state=(0, 0, 0, 0), n_random=8)
        for j, (method, p, i, ch, _) in enumerate(BD.model_schedule(O, count, size, 13)):
            m.call(method, p, i, ch, 5, j, 8)
        assert np.array_equal(g.palette, m.regular) and np.array_equal(g.backdrop, m.B) and np.array_equal(g.palette_map, m.palette_map)
    elif h != 224:  # (256 x 224: a handful of pairs only)
        run_slots_both(S, g, o, count, size, 0, 12, bool(flags.get("nes")))
    if h != 224:
        assert g.tile_palettes.tobytes() == table
        check_scores(g, o, pairs_now(), bw, bh)
    g.close()
    o.close()


def sweep_range(h, bw, bh):
    nb = BM.n_blocks(h, bw, bh)
    n = 4 if h == 224 else nb  # every block (at most 48), or the last four of the 112 at 224 rows
    return nb - n, n


def sweep_from(S, g0, img, count, size, bw, bh, flags, first, n, window):
    """A fresh context in g0's state, swept; -> (log bytes, stats, state, JSON)."""
    g = product(S, img, count, size, bw, bh, flags, init=False)
    g.tile_palettes, g.palette = g0.tile_palettes, g0.palette
    if flags.get("backdrop"):
        g.backdrop = g0.backdrop
    g.optimize()
    log, stats = g.block_sweep(first, n, window)
    out = log, stats, state_of(g), g.as_json()
    g.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,h,count,size,bw,bh,flags,kind", BC.CASES, ids=BC.CASE_IDS)
def test_block_sweep_windows_equal_call_by_call_and_the_model(S, O, name, h, count, size, bw, bh, flags, kind):
    """Block calls on every block (256 x 224: the last four) with window 1, 0, 3 and "all" from identical states, and window 0 on poisoned storage: identical logs and
    states bit for bit, equal to the model's call-by-call log (sub and changed exactly, errors within REL_ERR, check_gap on every
    candidate); final table, map and JSON the model's."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = BC.image(kind, h, bw, bh)
    g0 = product(S, img, count, size, bw, bh, flags)
    o = BC.model_start(O, img, count, size, bw, bh, flags)
    first, n = sweep_range(h, bw, bh)
    want = BM.model_block_sweep(o, first, n, count, bw, bh)
    ref = None
    for window in (1, 0, 3, n, "poison"):
        L.snesimage_debug_poison_alloc(1 if window == "poison" else 0)
        try:
            log, stats, state, js = sweep_from(S, g0, img, count, size, bw, bh, flags, first, n, 0 if window == "poison" else window)
        finally:
            L.snesimage_debug_poison_alloc(0)
        for r, w in zip(log, want):
            print("window %r: product %r model %r" % (window, (float(r["error"]), int(r["sub"]), int(r["changed"])), w))
        assert_log_matches(log, want)
        assert stats["calls"] == n and stats["accepted"] == sum(ch for _, _, ch in want) and stats["useful"] == n * (count - 1)
        assert BM.is_tied(np.frombuffer(state[0], np.uint8), h, bw, bh)
        if window == 1:
            assert stats["windows"] == n and stats["scored"] == stats["useful"]
            ref = (log.tobytes(), state, js)
        else:
            assert (log.tobytes(), state, js) == ref, window
    assert ref[1][0] == o.tile_palettes.tobytes() and ref[1][1] == o.palette_map.tobytes()
    assert abs(ref[1][3] - o.error()) <= REL_ERR * o.error()
    if not flags.get("backdrop"):
        assert ref[2] == o.as_json()
    else:
        from backdrop_model import model_json
        assert ref[2] == model_json(O, BC.regular(o, count, size, flags), BC.mean_backdrop(O, img, flags), o.tile_palettes, o.palette_map, img, count, size)
    # block_step is a sweep of one
    g = product(S, img, count, size, bw, bh, flags, init=False)
    g.tile_palettes, g.palette = g0.tile_palettes, g0.palette
    g.optimize()
    steps = [g.block_step(b) for b in range(first, first + n)]
    assert steps == [(float(r["error"]), int(r["sub"]), int(r["changed"])) for r in np.frombuffer(ref[0], dtype=S.api.TILE_LOG_DTYPE)]
    assert state_of(g) == ref[1]
    g.close()
    g0.close()
    o.close()


@pytest.mark.gpu
def test_failed_block_workspace_allocation_leaves_the_context_usable(S):
    from snesimage_amd import _ffi
    L = _ffi.load()
    _, h, count, size, bw, bh, flags, kind = BC.case("48_2x2")
    img = BC.image(kind, h, bw, bh)
    ref = product(S, img, count, size, bw, bh, flags)
    g = product(S, img, count, size, bw, bh, flags, init=False)
    g.tile_palettes, g.palette = ref.tile_palettes, ref.palette
    g.optimize()
    g.error()
    before = state_of(g)
    failures = 0
    for nth in (0, 1, 4, 9, 15, 22, 40):
        L.snesimage_debug_fail_alloc(nth)
        try:
            g.block_sweep(0, 24)
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
    log, _ = g.block_sweep(0, 24)
    want, _ = ref.block_sweep(0, 24, 1)
    assert log.tobytes() == want.tobytes() and state_of(g) == state_of(ref)
    g.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"perceptual": True}, {"dither": True}], ids=["rgb", "perceptual", "dither"])
def test_at_1x1_the_block_calls_are_the_tile_calls(S, flags):
    """block_sweep, block_step and score_block_moves against tile_sweep, tile_step and score_tile_moves: log, table, map and
    error bit for bit."""
    img = BC.image("alpha", 32)
    count, size = 4, 7
    a, b = (S.OptimizedImage(img, count, size, **flags) for _ in range(2))
    for x in (a, b):
        x.initialize_tiles()
        x.recalculate_palettes()
    assert b.palette_blocks == (1, 1)
    rng = np.random.default_rng(3)
    tiles, subs = rng.integers(0, 128, 40), rng.integers(0, count, 40)
    ea, ma = a.score_tile_moves(tiles, subs, want_maps=True)
    eb, mb = b.score_block_moves(tiles, subs, want_maps=True)
    assert ea.tobytes() == eb.tobytes() and np.array_equal(ma, mb)
    for window in (0, 1, 5):
        la, sa = a.tile_sweep(8, 40, window)
        lb, sb = b.block_sweep(8, 40, window)
        assert la.tobytes() == lb.tobytes() and sa == sb and state_of(a) == state_of(b)
    assert [a.tile_step(t) for t in range(60, 70)] == [b.block_step(t) for t in range(60, 70)]
    assert state_of(a) == state_of(b)
    a.close()
    b.close()


@pytest.mark.gpu
def test_the_other_paths_leave_the_table_as_they_found_it(S):
    """On a 2 x 2 context, in order: four scheduled calls through run_slots, a guided sweep, reduce_characters,
    refit_characters, export_native + render_native.  The table is byte-equal before and after; the render equals as_rgba()."""
    _, h, count, size, bw, bh, flags, kind = BC.case("32_2x2_alpha")
    img = BC.image("synth", h)
    g = product(S, img, count, size, bw, bh, flags)
    table = g.tile_palettes.tobytes()
    g.run_slots(4, seed=3)
    assert g.tile_palettes.tobytes() == table
    g.guided_sweep()
    assert g.tile_palettes.tobytes() == table
    u0 = g.characters()[0]
    _, u1 = g.reduce_characters(u0 - 4)
    assert u1 <= u0 - 4 and g.tile_palettes.tobytes() == table
    g.refit_characters()
    assert g.tile_palettes.tobytes() == table
    nat = g.export_native()
    rgba = g.render_native(nat["cgram"], nat["chr"], nat["map"], bpp=nat["bpp"])
    assert g.tile_palettes.tobytes() == table and BM.is_tied(g.tile_palettes, h, bw, bh)
    assert img[..., 3].all() and np.array_equal(rgba[..., :3], g.as_rgba()[..., :3])
    d = json.loads(g.as_tilemap_json())
    assert d is not None and g.palette_blocks == (bw, bh)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["--reassign-tiles", "--tile-moves"])
def test_cli_runs_on_blocks_and_equals_the_library(S, tmp_path, option):
    """--palette-blocks 2x2 with --reassign-tiles 1 and with --tile-moves 1 on a 256 x 32 PNG, one sweep of the palette: the JSON's
    tile_palettes is tied and the JSON equals the same run through api.py; --resume without the flag's table being tied is the
    library's refusal, exit 1."""
    import zlib, struct
    h, count, size, bw, bh = 32, 2, 3, 2, 2
    img = BC.image("synth", h)
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    png = tmp_path / "in.png"
    png.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 256, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    sched = S.schedule(count, size, 4 * count * size)
    n = next(j for j in range(len(sched)) if sched[j][4] != sched[0][4])  # the calls of one sweep of the palette
    out = str(tmp_path / "o.json")
    r = cli(str(png), out, "-c", str(count), "-s", str(size), "--palette-blocks", "2x2", option, "1", "--calls", str(n), "--seed", "2")
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(open(out).read())
    tp = np.zeros(1024, np.uint8)
    tp[:len(d["tile_palettes"])] = d["tile_palettes"]
    assert len(d["tile_palettes"]) == 32 * (h // 8) and BM.is_tied(tp, h, bw, bh)
    g = product(S, img, count, size, bw, bh, {})
    g.run_slots(n, seed=2)
    if option == "--reassign-tiles":
        g.reassign_tiles()
    else:
        g.block_sweep()
    assert g.as_json() == open(out).read()
    g.close()
    # a per-tile result resumed under the flag: the library's refusal of the untied table, exit 1 with its message
    per_tile = str(tmp_path / "t.json")
    r = cli(str(png), per_tile, "-c", "4", "-s", "3", "--calls", "0")
    assert r.returncode == 0, r.stdout + r.stderr
    r = cli(str(png), out, "-c", "4", "-s", "3", "--palette-blocks", "2x2", "--resume", per_tile, "--calls", "0")
    assert r.returncode == 1 and "not constant over block" in r.stderr + r.stdout, r.stdout + r.stderr
