"""Per-tile ordered-dither levels chosen by the objective (include/snesimage_hip.h: snesimage_set_ordered_dither_bank,
snesimage_level_sweep).

The model is tests/level_model.py: one target-side oracle per level, maps composed tile-wise, errors through an oracle over
the original.  Target images, maps, levels and decisions agree bit for bit, errors within the project's 1e-11 relative.  The
inputs are level_model.CASES; tests/test_level_model.py shows on the CPU that the model's sweep over each of them holds the
gap premise, accepts and rejects calls, and moves tiles off the start level."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import level_model as LM
import ordered_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = LM.REL_ERR
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
NAMES = ("snesimage_set_ordered_dither_bank", "snesimage_get_ordered_dither_bank", "snesimage_get_tile_levels", "snesimage_set_tile_levels",
         "snesimage_score_tile_levels", "snesimage_level_step", "snesimage_level_sweep")


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_level_symbols():
    from snesimage_amd import _ffi
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in NAMES:
        assert name + "(" in text and name in bound and getattr(lib, name) is not None
    assert lib.snesimage_set_ordered_dither_bank(None, None, 4, 2, 0) == ERR_ARG
    assert lib.snesimage_level_sweep(None, 0, 1, 0, None, None) == ERR_ARG
    assert lib.snesimage_score_tile_levels(None, None, None, 0, None, None) == ERR_ARG


def test_cli_argument_rules(tmp_path):
    out, lv = str(tmp_path / "o.json"), str(tmp_path / "lv.json")
    od = ["--ordered-dither", "4"]
    for args, word in [(["--tile-dither", "1", "-d"], "--dither"), (["--tile-dither", "1"], "--ordered-dither"),
                       (od + ["--tile-dither", "1", "--share", "synth:2=" + str(tmp_path / "s.json")], "--share"),
                       (od + ["--tile-dither", "1", "--devices", "0"], "--devices"),
                       (od + ["--dither-levels", "4", "--tile-dither", "1", "--devices", "0"], "--devices"),
                       (od + ["--tile-levels-out", lv, "--tile-dither", "1", "--share", "synth:2=" + str(tmp_path / "s.json")], "--share"),
                       (od + ["--tile-levels-in", lv, "--devices", "0"], "--devices"), (["--tile-levels-in", lv, "-d"], "--dither"),
                       (od + ["--dither-levels", "4", "--tile-dither", "1", "--share", "synth:2=" + str(tmp_path / "s.json")], "--share"),
                       (od + ["--tile-levels-out", lv, "--tile-dither", "1", "--devices", "0"], "--devices"),
                       (od + ["--tile-levels-in", lv, "--share", "synth:2=" + str(tmp_path / "s.json")], "--share"),
                       (od + ["--tile-dither", "1", "-d"], "--dither"), (od + ["--tile-levels-in", lv, "-d"], "--dither"),
                       (["--tile-levels-out", lv, "-d"], "--dither"), (["--dither-levels", "4", "-d"], "--dither"),
                       (od + ["--tile-dither", "0"], "--tile-dither"), (od + ["--tile-dither", "x"], "--tile-dither"),
                       (od + ["--tile-dither", "1", "--dither-levels", "1"], "--dither-levels"), (od + ["--tile-dither", "1", "--dither-levels", "9"], "--dither-levels"),
                       (od + ["--dither-levels", "4"], "--tile-dither"), (od + ["--tile-levels-out", lv], "--tile-dither"),
                       (od + ["--tile-dither", "1", "--dither-amplitude", "2"], "--dither-amplitude")]:
        r = run_cli("synth:1", out, *args)
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out) and not os.path.exists(lv)  # said before any file or device is touched
    h = run_cli("--help").stderr
    assert "--tile-dither" in h and "--dither-levels" in h and "--tile-levels-out" in h and "--tile-levels-in" in h and "default: 4: a choice, not a" in h


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

_refs = {}


def reference(O, name):
    """Everything the model says about a case, computed once and left unchanged."""
    if name in _refs:
        return _refs[name]
    h, hole, count, size, flags, backdrop, n, amp, L, seed = LM.CASES[name]
    img, bank, start, m, B = LM.case_setup(O, name)
    r = dict(img=img, bank=bank, start=start, B=B, count=count, size=size, flags=flags, backdrop=backdrop, L=L, ntile=m.ntile, msize=m.S,
             tp=m.tile_palettes, pal=m.palette, T0=m.T, map0=m.palette_map, err0=m.error())
    # mixed levels, and explicit pairs scored from there: 70 pairs (more than a chunk of 64) from 20 distinct ones, current-level pairs among them
    rng = np.random.default_rng(11)
    mixed = np.zeros(1024, np.uint8)
    mixed[:m.ntile] = rng.integers(0, L, m.ntile)
    m.set_levels(mixed)
    r.update(mixed=mixed, T_mixed=m.T, map_mixed=m.palette_map, err_mixed=m.error())
    pool = [(int(rng.integers(m.ntile)), int(rng.integers(L))) for _ in range(18)] + [(5, int(mixed[5])), (m.ntile - 1, int(mixed[m.ntile - 1]))]
    pairs = [pool[int(i)] for i in rng.integers(len(pool), size=68)] + pool[-2:]
    scored = {}
    for t, l in sorted(set(pairs)):
        scored[(t, l)] = (r["err_mixed"], m.palette_map) if l == mixed[t] else m.candidate(t, l)
    r.update(pairs=pairs, scored=scored)
    # the sweep from the start state, and a few optimizer calls on T(level) behind it
    lv0 = np.zeros(1024, np.uint8)
    lv0[:] = start
    m.set_levels(lv0)
    r["sweep"] = m.level_sweep()
    r.update(levels1=m.levels.copy(), T1=m.T, map1=m.palette_map, err1=m.error())
    sm = m.slot_model()
    calls = []
    for j, (method, p, i, ch, _) in enumerate(O.schedule(count, size, 4)):  # (regular slots, also of a backdrop context)
        e, rgb, changed = sm.call(method, [p * m.S + i], ch, 1, j, 8)
        calls.append((e, rgb, changed))
    r.update(calls=calls, pal2=sm.palette, map2=sm.palette_map)
    sm.close()
    m.close()
    _refs[name] = r
    return r


def regular(r, pal):
    """The regular entries of the model's palette: a backdrop context keeps B apart."""
    return pal.reshape(r["count"], r["msize"], 3)[:, :r["size"]].reshape(-1, 3) if r["backdrop"] else pal


def make_ctx(S, r, chunk=None):
    g = S.OptimizedImage(r["img"], r["count"], r["size"], backdrop=r["backdrop"], **r["flags"])
    if chunk:
        g.set_chunk(chunk)
    g.set_ordered_dither_bank(r["bank"], r["start"])
    g.tile_palettes = r["tp"]
    g.palette = regular(r, r["pal"])
    if r["backdrop"]:
        g.backdrop = r["B"]
    g.optimize()
    return g


def state_of(g):
    return g.tile_levels.tobytes(), g.target_rgba().tobytes(), g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.palette.tobytes(), g.error()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_target_image_and_map(S, O, name):
    """T after the bank setter and after set_tile_levels with mixed levels, and optimize() on both, against the model."""
    r = reference(O, name)
    g = make_ctx(S, r)
    assert np.array_equal(g.ordered_dither_bank, r["bank"]) and (g.tile_levels[:r["ntile"]] == r["start"]).all()
    assert np.array_equal(g.target_rgba(), r["T0"]) and np.array_equal(g.palette_map, r["map0"])
    assert rel(g.error(), r["err0"]) < REL_ERR
    g.tile_levels = r["mixed"]
    assert np.array_equal(g.tile_levels[:r["ntile"]], r["mixed"][:r["ntile"]])
    assert np.array_equal(g.target_rgba(), r["T_mixed"])
    assert not np.array_equal(r["T_mixed"], r["T0"])
    g.optimize()
    assert np.array_equal(g.palette_map, r["map_mixed"])
    assert not np.array_equal(r["map_mixed"], r["map0"]), "the levels change no pixel's choice: the comparison shows nothing"
    print("%s: error %r, model %r" % (name, g.error(), r["err_mixed"]))
    assert rel(g.error(), r["err_mixed"]) < REL_ERR
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_score_tile_levels(S, O, name):
    r = reference(O, name)
    g = make_ctx(S, r, chunk=64)  # 70 pairs: two launch groups
    g.tile_levels = r["mixed"]
    g.optimize()
    before = state_of(g)
    tiles, levels = [p[0] for p in r["pairs"]], [p[1] for p in r["pairs"]]
    errs, maps = g.score_tile_levels(tiles, levels, want_maps=True)
    worst = 0.0
    for j, p in enumerate(r["pairs"]):
        e, mp = r["scored"][p]
        worst = max(worst, rel(errs[j], e))
        assert np.array_equal(maps[j], mp), (j, p)
        if p[1] == r["mixed"][p[0]]:
            assert errs[j] == before[5], (j, p)  # the incumbent, bit for bit
    print("%s: max rel err of %d pairs %.3e" % (name, len(tiles), worst))
    assert worst <= REL_ERR
    assert np.array_equal(g.score_tile_levels(tiles[:3], levels[:3]), errs[:3])
    assert state_of(g) == before  # as if the calls had not been made
    g.close()


def swept_ctx(S, r, window):
    """A context at the case's start state whose slot contexts already exist, swept with `window` -> (context, log)."""
    g = make_ctx(S, r)
    g.run_slots(1, seed=9, n_random=8)  # the slot contexts exist before the levels move; the palette is put back below
    g.palette = regular(r, r["pal"])
    if r["backdrop"]:
        g.backdrop = r["B"]
    g.optimize()
    if window == "step":
        return g, np.array([g.level_step(t) for t in range(r["ntile"])], dtype=S.api.TILE_LOG_DTYPE)
    log, stats = g.level_sweep(window=window)
    assert stats["calls"] == r["ntile"] and stats["accepted"] == sum(ch for _, _, ch in r["sweep"])
    assert window != 1 or stats["windows"] == r["ntile"]
    return g, log


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_level_sweep_through_the_windows(S, O, name):
    """A sweep over every tile with window 1, 3 and 0 and level_step tile by tile: everything observable identical bit for bit,
    every decision the model's.  Then optimize() of the same palette without a rebuild of T (it reads the Lab(T) plane the
    commits left), and optimize() after a rebuild from the swept levels: both give the map the sweep left."""
    r = reference(O, name)
    want = r["sweep"]
    print("%s: %d calls, %d accepted, error %.6f -> %.6f" % (name, len(want), sum(ch for _, _, ch in want), r["err0"], r["err1"]))
    seen = []
    for window in (1, 3, 0, "step"):
        g, log = swept_ctx(S, r, window)
        LM.assert_log_matches(log, want)
        assert np.array_equal(g.tile_levels, r["levels1"]) and np.array_equal(g.target_rgba(), r["T1"]) and np.array_equal(g.palette_map, r["map1"])
        e = g.error()
        assert e == float(log[-1]["error"]) and rel(e, r["err1"]) < REL_ERR
        seen.append((log.tobytes(), state_of(g)))
        g.palette = regular(r, r["pal"])  # the map is owed again; T and Lab(T) stay as the commits wrote them
        g.optimize()
        assert np.array_equal(g.palette_map, r["map1"]) and g.error() == e
        if window == 0:  # and from scratch: the setter rebuilds T from the swept levels
            g.tile_levels = g.tile_levels
            g.optimize()
            assert np.array_equal(g.target_rgba(), r["T1"]) and np.array_equal(g.palette_map, r["map1"]) and g.error() == e
        g.close()
    assert all(s == seen[0] for s in seen)


_flows = {}


def check_calls(out, want, where):
    for j, (ce, rgb, changed) in enumerate(want):
        assert np.array_equal(out[j][2], rgb) and out[j][3] == changed, (where, j)
        assert rel(out[j][0], ce) < REL_ERR, (where, j, out[j][0], ce)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.CASES))
@pytest.mark.parametrize("window", [3, 0, 1])
def test_calls_sweep_calls_with_nothing_between(S, O, name, window):
    """What a run does: optimizer calls (they leave the pack, the contested list and the slot contexts' packs valid for their
    slot), a level sweep straight behind them, further calls on the same slot straight behind that, on one context with no setter, no
    error() and no read of the map in between — each of those would rebuild or invalidate something.  Equal to the model's
    calls on T(level) call by call (level_model.flow; its premises: tests/test_level_model.py).  A pack, a contested list or a
    slot context's pack left over from in front of the sweep, or a wrong Lab(T) plane behind a commit, shows in the calls."""
    r = reference(O, name)
    if name not in _flows:
        _flows[name] = LM.flow(O, name)
    f = _flows[name]
    seed = LM.FLOW_SEED[name]
    g = make_ctx(S, r)
    k0 = f["k0"]  # the schedule's first channel call: it and the two behind it share slot (0, 0), the sweep between them
    pre, _, _ = g.run_slots(2, seed=seed)
    one, st, _ = g.run_slots(1, seed=seed, first_step_id=k0, state=(0, 0, 0, 4))
    pre = pre + one
    log, stats = g.level_sweep(window=window)
    post, _, _ = g.run_slots(5, seed=seed, first_step_id=k0 + 1, state=st)
    check_calls(pre, f["pre"], (name, "pre"))
    LM.assert_log_matches(log, f["sweep"])
    assert stats["accepted"] == sum(ch for _, _, ch in f["sweep"])
    check_calls(post, f["post"], (name, "post"))
    assert np.array_equal(g.tile_levels, f["levels"]) and np.array_equal(g.target_rgba(), f["T"])
    assert np.array_equal(g.palette, regular(r, f["palette"])) and np.array_equal(g.palette_map, f["palette_map"])
    g.close()


@pytest.mark.gpu
def test_refusals_and_the_plain_setter_on_a_bank(S, O):
    from snesimage_amd import _ffi
    from snesimage_amd.throughput import ImageBatch
    L = _ffi.load()
    img = LM.image(16, 31)
    bank = LM.ladder(4, 64, 4)
    bp = bank.ctypes.data_as(_ffi._i8p)

    def refused(call, code):
        with pytest.raises(S.SnesImageError) as e:
            call()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    d = S.OptimizedImage(img, 2, 3, dither=True)
    refused(lambda: d.set_ordered_dither_bank(bank), UNSUPPORTED)
    d.set_ordered_dither_bank(None)  # switching "off" there is no error
    d.close()
    g = S.OptimizedImage(img, 2, 3)
    g.set_chunk(64)
    g.initialize_tiles()
    g.recalculate_palettes()
    before = g.error()
    refused(lambda: g.level_sweep(), ERR_STATE)  # no bank
    refused(lambda: g.score_tile_levels([0], [0]), ERR_STATE)
    refused(lambda: setattr(g, "tile_levels", np.zeros(1024, np.uint8)), ERR_STATE)
    assert L.snesimage_set_ordered_dither_bank(g._c, bp, 4, 9, 0) == ERR_ARG  # L = 9
    assert L.snesimage_set_ordered_dither_bank(g._c, bp, 3, 2, 0) == ERR_ARG
    assert L.snesimage_set_ordered_dither_bank(g._c, bp, 4, 4, 4) == ERR_ARG  # the start level is no table of the bank
    assert L.snesimage_set_ordered_dither_bank(g._c, None, 4, 4, 0) == ERR_ARG
    assert g.ordered_dither_bank is None and g.error() == before
    g.set_ordered_dither_bank(bank, 3)
    g.optimize()
    lv = g.tile_levels
    lv[7] = 4
    refused(lambda: setattr(g, "tile_levels", lv), ERR_ARG)  # a level >= L on a tile of the image
    lv[7], lv[500] = 3, 200  # (beyond the image: no tile)
    g.tile_levels = lv
    refused(lambda: g.score_tile_levels([0], [4]), ERR_ARG)
    refused(lambda: g.score_tile_levels([64], [0]), ERR_ARG)
    refused(lambda: g.level_sweep(60, 8), ERR_ARG)
    assert "snesimage_get_ordered_dither_bank" in refused(lambda: g.ordered_dither, ERR_STATE)
    # batches, sets and groups refuse a member with a bank of several tables
    for create in (L.snesimage_batch_create, L.snesimage_shared_create, L.snesimage_group_create):
        h = C.c_void_p()
        assert create((C.c_void_p * 1)(g._c), 1, C.byref(h)) == ERR_ARG and not h.value, create
        assert b"bank" in L.snesimage_last_error()
    msg = refused(lambda: S.SharedPalette([g]), ERR_ARG)
    assert "bank" in msg
    twin = S.OptimizedImage(img, 2, 3)
    assert "bank" in refused(lambda: S.SharedPalette([twin], ordered_dither=bank), ERR_ARG)
    twin.close()
    b = ImageBatch([(0, img), (1, LM.image(16, 32))], 2, 3, batched=True, groups=1, ordered_dither=bank)
    assert "bank" in refused(b.initialize, ERR_ARG)  # where the batch forms
    b.close()
    # a pending split-phase step
    from hipmem import DeviceArray
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    refused(lambda: g.set_ordered_dither_bank(bank), ERR_STATE)
    refused(lambda: setattr(g, "tile_levels", np.zeros(1024, np.uint8)), ERR_STATE)
    refused(lambda: g.level_sweep(), ERR_STATE)
    g.step_commit(buf.ptr)
    # the plain setter replaces the bank by a bank of one; a bank of one is that table
    table = OM.bayer(4, 64)
    g.set_ordered_dither(table)
    g.optimize()
    assert np.array_equal(g.ordered_dither, table) and np.array_equal(g.ordered_dither_bank, table[None]) and not g.tile_levels.any()
    assert np.array_equal(g.target_rgba(), OM.target_image(img, table))
    e_plain, map_plain = g.error(), g.palette_map
    log, stats = g.level_sweep(0, 8)
    assert stats["calls"] == 8 and stats["accepted"] == 0 and all(float(x["error"]) == e_plain and x["sub"] == 0 for x in log)
    g.set_ordered_dither_bank(table[None])
    g.optimize()
    assert np.array_equal(g.ordered_dither, table) and g.error() == e_plain and np.array_equal(g.palette_map, map_plain)
    h = C.c_void_p()
    assert L.snesimage_group_create((C.c_void_p * 1)(g._c), 1, C.byref(h)) == 0, L.snesimage_last_error()  # a bank of one is a table: members may carry it
    refused(lambda: g.set_ordered_dither_bank(bank), ERR_STATE)  # lent
    L.snesimage_group_destroy(h)
    g.set_ordered_dither_bank(None)
    g.optimize()
    assert g.ordered_dither is None and g.ordered_dither_bank is None and np.array_equal(g.target_rgba(), img)
    plain = S.OptimizedImage(img, 2, 3)  # (the split-phase step above moved the palette: a context without a bank in that state)
    plain.tile_palettes, plain.palette = g.tile_palettes, g.palette
    plain.optimize()
    assert g.error() == plain.error() and np.array_equal(g.palette_map, plain.palette_map)
    plain.close()
    g.close()


@pytest.mark.gpu
def test_failed_workspace_allocation_leaves_the_context_usable(S, O):
    from snesimage_amd import _ffi
    L = _ffi.load()
    r = reference(O, "hole-2x3-L4-perceptual")
    ref = make_ctx(S, r)
    g = make_ctx(S, r)
    before = state_of(g)
    failures, log = 0, None
    for nth in (0, 1, 4, 9, 15, 21, 22, 23, 24, 40):
        L.snesimage_debug_fail_alloc(nth)
        try:
            log, _ = g.level_sweep(0, 48)
            ok = True
        except S.SnesImageError as e:
            assert e.code == ERR_HIP
            ok = False
            failures += 1
        finally:
            L.snesimage_debug_fail_alloc(-1)
        if ok:
            break
        assert state_of(g) == before
    assert failures >= 3
    fresh = S.OptimizedImage(r["img"], r["count"], r["size"], **r["flags"])
    L.snesimage_debug_fail_alloc(0)  # the setter's own buffers
    try:
        with pytest.raises(S.SnesImageError):
            fresh.set_ordered_dither_bank(r["bank"], r["start"])
    finally:
        L.snesimage_debug_fail_alloc(-1)
    assert fresh.ordered_dither_bank is None and np.array_equal(fresh.target_rgba(), r["img"])
    fresh.close()
    if log is None:
        log, _ = g.level_sweep(0, 48)
    want, _ = ref.level_sweep(0, 48, 1)
    assert log.tobytes() == want.tobytes() and state_of(g) == state_of(ref)
    g.close()
    ref.close()


def drive(S, g, calls, every, seed=1):
    """The CLI's loop: scheduled calls, a level sweep behind every `every` sweeps of the palette and one behind the last call."""
    st, sweep = (0, 0, 0, 0), 0
    for call in range(calls):
        _, st, _ = g.run_slots(1, seed=seed, first_step_id=call, state=st, window=1)
        if st[3] != sweep:
            if st[3] % every == 0:
                g.error()
                g.level_sweep()
            sweep = st[3]
    g.error()
    g.level_sweep()


@pytest.mark.gpu
def test_cli_ladder_levels_out_and_resume(tmp_path, S):
    """--tile-dither writes the JSON and the levels of the library driven the same way.  --resume with --tile-levels-in writes
    what the library writes when it continues from that state without an interruption: the levels, tile palettes and palette of
    the first run's files, the schedule and the call numbers starting again at 0 as every --resume run starts them (the
    convention of test_ordered_dither's round trip; the CLI has no way to enter the schedule in the middle, so this is not
    compared with one run of 22 calls)."""
    img = OM.with_hole(OM.image(64, 40))
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    a, la, c, lc = (str(tmp_path / f) for f in ("a.json", "a.levels.json", "c.json", "c.levels.json"))
    common = ["-c", "2", "-s", "3", "--ordered-dither", "4", "--dither-amplitude", "48", "--seed", "1", "--tile-dither", "1"]
    r = run_cli(str(src), a, *common, "--dither-levels", "5", "--calls", "14", "--tile-levels-out", la)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Per-tile dither levels: 5 levels, amplitudes 0, 12, 24, 36, 48" in r.stdout and r.stdout.count("Tile dither: 256 calls") == 3
    first = json.loads(open(la).read())
    assert first["n"] == 4 and first["amplitudes"] == [48 * j // 4 for j in range(5)] and len(first["levels"]) == 256
    assert 0 < sum(l != 4 for l in first["levels"]), "no tile left the start level: the comparison shows nothing"
    bank = LM.ladder(4, 48, 5)
    g = S.OptimizedImage(img, 2, 3)
    g.set_ordered_dither_bank(bank, 4)
    g.initialize_tiles()
    g.recalculate_palettes()
    drive(S, g, 14, 1)
    assert g.as_json() == open(a).read() and g.tile_levels[:256].tolist() == first["levels"]
    # eight further calls from the two files == the library continuing from that state
    r = run_cli(str(src), c, *common, "--resume", a, "--tile-levels-in", la, "--calls", "8", "--tile-levels-out", lc)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Per-tile dither levels: 5 levels, amplitudes 0, 12, 24, 36, 48" in r.stdout
    tp, pal = g.tile_palettes, g.palette
    g.close()
    g = S.OptimizedImage(img, 2, 3)
    g.set_ordered_dither_bank(bank, 4)
    lv = np.zeros(1024, np.uint8)
    lv[:256] = first["levels"]
    g.tile_levels = lv
    g.tile_palettes, g.palette = tp, pal
    g.optimize()
    drive(S, g, 8, 1)
    second = json.loads(open(lc).read())
    assert g.as_json() == open(c).read() and g.tile_levels[:256].tolist() == second["levels"] and second["amplitudes"] == first["amplitudes"]
    g.close()
    # a levels file for another pattern size is refused
    r = run_cli(str(src), c, "-c", "2", "-s", "3", "--ordered-dither", "8", "--tile-levels-in", la)
    assert r.returncode != 0 and "--ordered-dither 4" in r.stderr + r.stdout
    # the ladder is the file's: a command line that names another one is refused
    for extra, word in ((["--dither-levels", "4"], "--dither-levels"), (["--dither-amplitude", "32"], "--dither-amplitude")):
        r = run_cli(str(src), c, "-c", "2", "-s", "3", "--ordered-dither", "4", "--tile-levels-in", la, *extra)
        assert r.returncode != 0 and word in r.stderr + r.stdout, (extra, r.stderr)
