"""Per-tile ordered-dither levels of a shared-palette set, tied or per frame (include/snesimage_hip.h:
snesimage_shared_set_ordered_dither_bank, snesimage_shared_level_sweep).

The model is tests/set_level_model.py: one level_model.Model per frame, a tied call decided on the frames' errors summed in
member order.  Target images, maps, levels and decisions agree bit for bit, errors within the project's 1e-11 relative.  The
inputs are set_level_model.CASES; tests/test_set_level_model.py shows on the CPU that a tied sweep over each of them holds the
gap premise on the sum, accepts calls that make one frame worse and rejects calls one frame alone would take."""
import json
import os
import subprocess

import numpy as np
import pytest

import level_model as LM
import ordered_model as OM
import set_level_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = SM.REL_ERR
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
NAMES = ("snesimage_shared_set_ordered_dither_bank", "snesimage_shared_set_tile_levels", "snesimage_shared_score_tile_levels", "snesimage_shared_level_sweep")


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_set_level_symbols():
    from snesimage_amd import _ffi
    from snesimage_amd.shared import SharedPalette
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in NAMES:
        assert name + "(" in text and name in bound and getattr(lib, name) is not None
    assert "TIED LEVEL CALL" in text
    assert lib.snesimage_shared_set_ordered_dither_bank(None, None, 4, 2, 0) == ERR_ARG
    assert lib.snesimage_shared_set_tile_levels(None, 0, None) == ERR_ARG
    assert lib.snesimage_shared_score_tile_levels(None, None, None, 0, None, None) == ERR_ARG
    assert lib.snesimage_shared_level_sweep(None, 0, 1, 0, 1, None, None) == ERR_ARG
    for method in ("set_ordered_dither_bank", "set_tile_levels", "tile_levels", "score_tile_levels", "level_sweep"):
        assert hasattr(SharedPalette, method)


def levels_file(path, frames, tied=True, n=4, amps=(0, 16, 32, 48)):
    path.write_text(json.dumps(dict(n=n, amplitudes=list(amps), tied=tied, frames=frames)))
    return str(path)


def test_cli_argument_rules(tmp_path):
    out, lv, s1 = str(tmp_path / "o.json"), str(tmp_path / "lv.json"), str(tmp_path / "s.json")
    od, share = ["--ordered-dither", "4"], ["--share", "synth:2=" + s1]
    for args, word in [(od + share + ["--set-tile-dither", "1", "-d"], "--dither"), (share + ["--set-tile-dither", "1", "-d"], "--dither"),
                       (od + share + ["--set-tile-dither", "1", "--devices", "0"], "--devices"),
                       (od + share + ["--set-levels", "frame", "--set-tile-dither", "1", "--devices", "0"], "--devices"),
                       (od + share + ["--set-tile-levels-out", lv, "--set-tile-dither", "1", "--devices", "0"], "--devices"),
                       (od + share + ["--set-tile-levels-in", lv, "--devices", "0"], "--devices"), (share + ["--set-tile-levels-in", lv, "-d"], "--dither"),
                       (share + ["--set-tile-levels-out", lv, "-d"], "--dither"), (share + ["--set-levels", "tied", "-d"], "--dither"),
                       (od + ["--set-tile-dither", "1"], "--share"), (od + ["--set-levels", "frame"], "--share"),
                       (od + ["--set-tile-levels-out", lv, "--set-tile-dither", "1"], "--share"), (od + ["--set-tile-levels-in", lv], "--share"),
                       (share + ["--set-tile-dither", "1"], "--ordered-dither"), (share + ["--set-tile-levels-in", lv], "--ordered-dither"),
                       (od + share + ["--set-tile-dither", "0"], "--set-tile-dither"), (od + share + ["--set-tile-dither", "x"], "--set-tile-dither"),
                       (od + share + ["--set-tile-dither", "1", "--set-levels", "both"], "--set-levels"),
                       (od + share + ["--set-levels", "frame"], "--set-tile-dither"), (od + share + ["--set-tile-levels-out", lv], "--set-tile-dither"),
                       (od + share + ["--set-tile-dither", "1", "--dither-levels", "1"], "--dither-levels"), (od + share + ["--set-tile-dither", "1", "--dither-levels", "9"], "--dither-levels"),
                       (od + share + ["--set-tile-dither", "1", "--dither-amplitude", "2"], "--dither-amplitude"),
                       (od + share + ["--set-tile-dither", "1", "--tile-dither", "1"], "--share"),  # the levels of one image stay refused beside --share
                       (od + share + ["--dither-levels", "4"], "--share")]:                          # ... and --dither-levels alone still means them
        r = run_cli("synth:1", out, *args)
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out) and not os.path.exists(lv) and not os.path.exists(s1)  # said before any file or device is touched
    h = run_cli("--help").stderr
    assert all(o in h for o in ("--set-tile-dither", "--set-levels", "--set-tile-levels-out", "--set-tile-levels-in")) and "[default: tied: a choice" in h
    # a levels file that does not fit the command line: refused before any image or device is touched
    two = [[3] * 96, [3] * 96]
    base = ["synth:1", out] + od + share
    for file, extra, word in [(levels_file(tmp_path / "a.json", two), ["--dither-levels", "5"], "--dither-levels"),
                              (levels_file(tmp_path / "b.json", two), ["--dither-amplitude", "32"], "--dither-amplitude"),
                              (levels_file(tmp_path / "c.json", two + [[3] * 96]), [], "3 frames"),
                              (levels_file(tmp_path / "d.json", [[3] * 96, [2] + [3] * 95]), [], "tied"),
                              (levels_file(tmp_path / "e.json", [[3] * 96, [2] + [3] * 95], tied=False), [], "--set-levels frame"),
                              (levels_file(tmp_path / "f.json", two, n=8), [], "--ordered-dither 8"),
                              (levels_file(tmp_path / "g.json", [[4] * 96, [4] * 96]), [], "level out of range")]:
        r = run_cli(*base, "--set-tile-levels-in", file, *extra)
        assert r.returncode != 0 and word in r.stderr + r.stdout, (file, extra, r.stdout + r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

_refs = {}


def reference(O, name):
    """Everything the model says about a case, computed once and left unchanged."""
    if name in _refs:
        return _refs[name]
    F, h, hole, count, size, flags, n, amp, L, seed = SM.CASES[name]
    imgs, bank, start, m, tps, pal = SM.case_setup(O, name)
    nt = m.ntile
    r = dict(F=F, imgs=imgs, bank=bank, start=start, count=count, size=size, flags=flags, L=L, ntile=nt, tps=tps, pal=pal,
             T0=[f.T for f in m.frames], map0=[f.palette_map for f in m.frames], errs0=m.errors())
    # mixed levels, every frame its own but for two tiles, and explicit pairs scored from there: 70 pairs (more than a chunk of 64)
    # from 20 distinct ones, two of them naming the level every frame is on
    rng = np.random.default_rng(11)
    mixed = np.zeros((F, 1024), np.uint8)
    mixed[:, :nt] = rng.integers(0, L, (F, nt))
    mixed[:, 5], mixed[:, nt - 1] = mixed[0, 5], mixed[0, nt - 1]
    for f, lv in zip(m.frames, mixed):
        f.set_levels(lv)
    r.update(mixed=mixed, T_mixed=[f.T for f in m.frames], map_mixed=[f.palette_map for f in m.frames], errs_mixed=m.errors())
    pool = [(int(rng.integers(nt)), int(rng.integers(L))) for _ in range(18)] + [(5, int(mixed[0, 5])), (nt - 1, int(mixed[0, nt - 1]))]
    pairs = [pool[int(i)] for i in rng.integers(len(pool), size=68)] + pool[-2:]
    scored = {}
    for t, l in sorted(set(pairs)):
        es, same = [], []
        for i, f in enumerate(m.frames):
            e, mp = f.candidate(t, l)
            same.append(bool(np.array_equal(mp, f.palette_map)))  # on that level already, or the tile's 64 choices do not change
            es.append(r["errs_mixed"][i] if same[-1] else e)
        scored[(t, l)] = (SM.total(es), es, same)
    r.update(pairs=pairs, scored=scored)
    # the tied sweep from the start state
    lv0 = np.full(1024, start, np.uint8)
    for f in m.frames:
        f.set_levels(lv0)
    r["sweep"] = m.tied_sweep()
    r.update(levels1=m.levels, T1=[f.T for f in m.frames], map1=[f.palette_map for f in m.frames], errs1=m.errors())
    # the per-frame sweep from the start state
    for f in m.frames:
        f.set_levels(lv0)
    r["fsweep"] = m.frame_sweep()
    r.update(levelsF=m.levels, TF=[f.T for f in m.frames], mapF=[f.palette_map for f in m.frames], errsF=m.errors())
    m.close()
    _refs[name] = r
    return r


def make_members(S, r, table=None, **more):
    ctxs = [S.OptimizedImage(img, r["count"], r["size"], **r["flags"], **more) for img in r["imgs"]]
    for c, tp in zip(ctxs, r["tps"]):
        c.set_chunk(64)
        if table is not None:
            c.set_ordered_dither(table)
        c.tile_palettes = tp
        c.palette = r["pal"]
        c.optimize()
    return ctxs


def make_set(S, r, bank=True):
    """The members in the case's start state (set explicitly, before the set forms), the set, and the set's bank."""
    ctxs = make_members(S, r)
    sp = S.SharedPalette(ctxs)
    if bank:
        sp.set_ordered_dither_bank(r["bank"], r["start"])
    return sp, ctxs


def close_all(sp, ctxs):
    sp.close()
    for c in ctxs:
        c.close()


def state_of(sp, ctxs):
    return tuple((c.tile_levels.tobytes(), c.target_rgba().tobytes(), c.tile_palettes.tobytes(), c.palette_map.tobytes(), c.palette.tobytes(), c.error()) for c in ctxs) + (sp.error(),)


def refused(S, call, code):
    with pytest.raises(S.SnesImageError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_bank_setter(S, O, name):
    """After the set's bank setter every member's T, map and error are the model's; a bank of one table is that table."""
    r = reference(O, name)
    sp, ctxs = make_set(S, r)
    assert (sp.tile_levels[:, :r["ntile"]] == r["start"]).all() and sp.tile_levels.shape == (r["F"], 1024)
    for i, c in enumerate(ctxs):
        assert np.array_equal(c.ordered_dither_bank, r["bank"])
        assert np.array_equal(c.target_rgba(), r["T0"][i]) and np.array_equal(c.palette_map, r["map0"][i]), i
        print("%s member %d: error %r, model %r" % (name, i, c.error(), r["errs0"][i]))
        assert rel(c.error(), r["errs0"][i]) < REL_ERR
    assert rel(sp.error(), SM.total(r["errs0"])) < REL_ERR
    # mixed levels through the set, member by member
    for i in range(r["F"]):
        sp.set_tile_levels(i, r["mixed"][i])
    assert np.array_equal(sp.tile_levels[:, :r["ntile"]], r["mixed"][:, :r["ntile"]])
    for i, c in enumerate(ctxs):
        assert np.array_equal(c.target_rgba(), r["T_mixed"][i]) and np.array_equal(c.palette_map, r["map_mixed"][i]), i
        assert rel(c.error(), r["errs_mixed"][i]) < REL_ERR
    assert any(not np.array_equal(a, b) for a, b in zip(r["map_mixed"], r["map0"])), "the levels change no pixel's choice: the comparison shows nothing"
    close_all(sp, ctxs)
    # a bank of one table: the set of SharedPalette(ctxs, ordered_dither=table), bit for bit
    table = r["bank"][r["L"] - 1]
    sp, ctxs = make_set(S, r, bank=False)
    sp.set_ordered_dither_bank(table[None])
    twins = make_members(S, r)
    sq = S.SharedPalette(twins, ordered_dither=table)
    for c, t in zip(ctxs, twins):
        assert np.array_equal(c.ordered_dither, table) and np.array_equal(c.target_rgba(), t.target_rgba())
        assert np.array_equal(c.palette_map, t.palette_map) and c.error() == t.error()
    assert sp.error() == sq.error()
    log, stats = sp.level_sweep(0, 8)
    assert stats["calls"] == 8 and stats["accepted"] == 0 and all(float(x["error"]) == sp.error() and x["sub"] == 0 and not x["changed"] for x in log)
    sp.set_ordered_dither_bank(None)  # and off again: the original
    for c, img in zip(ctxs, r["imgs"]):
        assert c.ordered_dither_bank is None and np.array_equal(c.target_rgba(), img)
    close_all(sp, ctxs)
    close_all(sq, twins)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_score_tile_levels(S, O, name):
    r = reference(O, name)
    sp, ctxs = make_set(S, r)  # chunk 64, 70 pairs: two launch groups
    for i in range(r["F"]):
        sp.set_tile_levels(i, r["mixed"][i])
    before = state_of(sp, ctxs)
    incs = [s[5] for s in before[:-1]]
    tiles, levels = [p[0] for p in r["pairs"]], [p[1] for p in r["pairs"]]
    errs, mem = sp.score_tile_levels(tiles, levels)
    assert mem.shape == (len(tiles), r["F"])
    worst, exact = 0.0, 0
    for j, p in enumerate(r["pairs"]):
        E, es, same = r["scored"][p]
        worst = max([worst, rel(errs[j], E)] + [rel(mem[j, i], es[i]) for i in range(r["F"])])
        for i in range(r["F"]):
            if same[i]:
                assert mem[j, i] == incs[i], (j, p, i)  # the incumbent, bit for bit
                exact += 1
        assert errs[j] == SM.total(mem[j]), (j, p)  # summed in member order
        if all(same):
            assert errs[j] == before[-1], (j, p)
    print("%s: max rel err of %d pairs %.3e, %d member errors the incumbent bit for bit" % (name, len(tiles), worst, exact))
    assert worst <= REL_ERR and exact >= 2 * r["F"]
    e3, _ = sp.score_tile_levels(tiles[:3], levels[:3])
    assert np.array_equal(e3, errs[:3])
    assert state_of(sp, ctxs) == before  # as if the calls had not been made
    close_all(sp, ctxs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_tied_sweep_through_the_windows(S, O, name):
    """A tied sweep over every tile position with window 1, 3 and 0: everything observable identical bit for bit, every
    decision the model's, in every member."""
    r = reference(O, name)
    want = r["sweep"]
    print("%s: %d calls, %d accepted, E %.6f -> %.6f" % (name, len(want), sum(ch for _, _, ch in want), SM.total(r["errs0"]), SM.total(r["errs1"])))
    seen = []
    for window in (1, 3, 0):
        sp, ctxs = make_set(S, r)
        log, stats = sp.level_sweep(window=window)
        SM.assert_log_matches(log, want)
        assert stats["calls"] == r["ntile"] and stats["accepted"] == sum(ch for _, _, ch in want)
        if window == 1:
            assert stats["windows"] == r["ntile"]
        if window == 0:
            assert stats["windows"] < stats["calls"]
        assert np.array_equal(sp.tile_levels, r["levels1"])
        for i, c in enumerate(ctxs):
            assert np.array_equal(c.target_rgba(), r["T1"][i]) and np.array_equal(c.palette_map, r["map1"][i]), (window, i)
            assert rel(c.error(), r["errs1"][i]) < REL_ERR
        E = sp.error()
        assert E == float(log[-1]["error"]) and rel(E, SM.total(r["errs1"])) < REL_ERR
        seen.append((log.tobytes(), state_of(sp, ctxs)))
        sp.palette = r["pal"]  # the maps are owed again; T and Lab(T) stay as the commits wrote them
        for i, c in enumerate(ctxs):
            assert np.array_equal(c.palette_map, r["map1"][i])
        assert sp.error() == E
        close_all(sp, ctxs)
    assert all(s == seen[0] for s in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_per_frame_sweep_then_a_tied_sweep_is_refused(S, O, name):
    r = reference(O, name)
    sp, ctxs = make_set(S, r)
    log, stats = sp.level_sweep(tied=False)
    assert log.shape == (r["F"], r["ntile"]) and stats["calls"] == r["F"] * r["ntile"]
    for i, c in enumerate(ctxs):
        LM.assert_log_matches(log[i], r["fsweep"][i])
        assert np.array_equal(c.tile_levels, r["levelsF"][i]) and np.array_equal(c.target_rgba(), r["TF"][i]) and np.array_equal(c.palette_map, r["mapF"][i]), i
        assert c.error() == float(log[i][-1]["error"]) and rel(c.error(), r["errsF"][i]) < REL_ERR
    assert stats["accepted"] == sum(ch for f in r["fsweep"] for _, _, ch in f)
    assert rel(sp.error(), SM.total(r["errsF"])) < REL_ERR
    differ = np.flatnonzero((r["levelsF"][:, :r["ntile"]] != r["levelsF"][0, :r["ntile"]]).any(0))
    assert differ.size, "every frame chose the same levels: the refusal below shows nothing"
    before = state_of(sp, ctxs)
    assert "differ in level" in refused(S, lambda: sp.level_sweep(), ERR_STATE)
    assert "differ in level" in refused(S, lambda: sp.level_sweep(int(differ[0]), 1, window=1), ERR_STATE)
    assert state_of(sp, ctxs) == before
    close_all(sp, ctxs)


_flows = {}


def stored_error(O, r, ctxs):
    """The model's error of the members' stored maps: a plain oracle over each original holding the member's state."""
    es = []
    for img, c in zip(r["imgs"], ctxs):
        o = O.OracleImage(img, r["count"], r["size"], **r["flags"])
        o.tile_palettes, o.palette, o.palette_map = c.tile_palettes, c.palette, c.palette_map
        es.append(o.error())
        o.close()
    return SM.total(es)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SM.FLOW_SEED))
def test_sweep_then_the_other_set_paths(S, O, name):
    """What a run does.  The set's slot contexts exist before the bank arrives (they borrowed the members' target pointers when
    the target was the original); then a tied sweep and six scheduled calls straight behind it, with nothing set or read in
    between, against the summed model call by call: a slot context still reading the old target, or a pack left over from in
    front of the sweep, shows in the calls.  Then the set's tile sweep, character budget and refit: after each, error() is the
    model's error of the members' stored maps."""
    r = reference(O, name)
    if name not in _flows:
        _flows[name] = SM.flow(O, name)
    f = _flows[name]
    sp, ctxs = make_set(S, r, bank=False)
    sp.run_slots(1, seed=9, n_random=8)
    sp.palette = r["pal"]
    sp.set_ordered_dither_bank(r["bank"], r["start"])
    log, stats = sp.level_sweep()
    calls, _, _ = sp.run_slots(SM.FLOW_CALLS, seed=SM.FLOW_SEED[name], n_random=SM.FLOW_RANDOM)
    SM.assert_log_matches(log, f["sweep"])
    for j, (e, rgb, changed) in enumerate(f["calls"]):
        assert np.array_equal(calls[j][2], rgb) and calls[j][3] == changed, (name, j)
        assert rel(calls[j][0], e) < REL_ERR, (name, j, calls[j][0], e)
    assert np.array_equal(sp.tile_levels, f["levels"]) and np.array_equal(sp.palette, f["palette"])
    for i, c in enumerate(ctxs):
        assert np.array_equal(c.target_rgba(), f["T"][i]) and np.array_equal(c.palette_map, f["maps2"][i]), i
    assert rel(sp.error(), f["E2"]) < REL_ERR and rel(sp.error(), stored_error(O, r, ctxs)) < REL_ERR
    _, ts = sp.tile_sweep()
    print("%s: tile sweep accepted %d" % (name, ts["accepted"]))
    assert rel(sp.error(), stored_error(O, r, ctxs)) < REL_ERR
    U = sp.characters()[0]
    merges, U1 = sp.reduce_characters(U - 3)
    assert U1 < U and len(merges) > 0
    assert rel(sp.error(), stored_error(O, r, ctxs)) < REL_ERR
    sp.refit_characters()
    assert rel(sp.error(), stored_error(O, r, ctxs)) < REL_ERR
    for i, c in enumerate(ctxs):  # T is still T(level): the levels did not move behind the sweep
        assert np.array_equal(c.target_rgba(), f["T"][i])
    close_all(sp, ctxs)
    # after snesimage_shared_destroy the members keep bank and levels, as lone contexts do
    sp, ctxs = make_set(S, r)
    sp.level_sweep(0, 8)
    lv = sp.tile_levels
    sp.close()
    for c, l in zip(ctxs, lv):
        assert np.array_equal(c.ordered_dither_bank, r["bank"]) and np.array_equal(c.tile_levels, l)
        c.level_sweep(0, 4)  # a legal lone context
        c.close()


@pytest.mark.gpu
def test_refusals(S, O):
    from snesimage_amd import _ffi
    L = _ffi.load()
    name = "set2-hole-2x3-L4-perceptual"
    r = reference(O, name)
    bank, nt = r["bank"], r["ntile"]
    bp = np.ascontiguousarray(bank, np.int8).ctypes.data_as(_ffi._i8p)
    # a SNES_DITHER set
    d = make_members(S, r, dither=True)
    sd = S.SharedPalette(d)
    refused(S, lambda: sd.set_ordered_dither_bank(bank), UNSUPPORTED)
    sd.set_ordered_dither_bank(None)  # switching "off" there is no error
    close_all(sd, d)
    sp, ctxs = make_set(S, r, bank=False)
    refused(S, lambda: sp.level_sweep(), ERR_STATE)  # no bank
    refused(S, lambda: sp.score_tile_levels([0], [0]), ERR_STATE)
    refused(S, lambda: sp.set_tile_levels(0, np.zeros(1024, np.uint8)), ERR_STATE)
    before = state_of(sp, ctxs)
    assert L.snesimage_shared_set_ordered_dither_bank(sp._s, bp, 8, 9, 0) == ERR_ARG  # L = 9
    assert L.snesimage_shared_set_ordered_dither_bank(sp._s, bp, 3, 2, 0) == ERR_ARG
    assert L.snesimage_shared_set_ordered_dither_bank(sp._s, bp, 8, 4, 4) == ERR_ARG  # the start level is no table of the bank
    assert L.snesimage_shared_set_ordered_dither_bank(sp._s, None, 8, 4, 0) == ERR_ARG
    assert state_of(sp, ctxs) == before
    # a failed allocation of the bank setter leaves every member as it was (two members, four buffers each)
    for nth in (0, 3, 4, 7):
        L.snesimage_debug_fail_alloc(nth)
        try:
            assert refused(S, lambda: sp.set_ordered_dither_bank(bank, r["start"]), ERR_HIP)
        finally:
            L.snesimage_debug_fail_alloc(-1)
        assert state_of(sp, ctxs) == before and all(c.ordered_dither_bank is None for c in ctxs), nth
    sp.set_ordered_dither_bank(bank, r["start"])
    for i, c in enumerate(ctxs):
        assert np.array_equal(c.target_rgba(), r["T0"][i]) and np.array_equal(c.palette_map, r["map0"][i])
    before = state_of(sp, ctxs)
    lv = np.full(1024, r["start"], np.uint8)
    lv[7] = r["L"]
    refused(S, lambda: sp.set_tile_levels(0, lv), ERR_ARG)  # a level beyond the bank
    refused(S, lambda: sp.score_tile_levels([0], [r["L"]]), ERR_ARG)
    refused(S, lambda: sp.set_tile_levels(r["F"], np.zeros(1024, np.uint8)), ERR_ARG)  # a member beyond F
    refused(S, lambda: sp.score_tile_levels([nt], [0]), ERR_ARG)  # a tile beyond the image
    refused(S, lambda: sp.level_sweep(nt - 4, 8), ERR_ARG)
    refused(S, lambda: sp.level_sweep(nt - 4, 8, tied=False), ERR_ARG)
    # a member's own setters while lent
    refused(S, lambda: setattr(ctxs[0], "tile_levels", np.zeros(1024, np.uint8)), ERR_STATE)
    refused(S, lambda: ctxs[1].set_ordered_dither_bank(bank), ERR_STATE)
    refused(S, lambda: ctxs[1].set_ordered_dither(bank[1]), ERR_STATE)
    assert state_of(sp, ctxs) == before
    # a pending split-phase step of a member (it takes the member out of the set's hands for good: last)
    from hipmem import DeviceArray
    buf = DeviceArray(64, np.float64, fill=0)
    ctxs[0].step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    refused(S, lambda: sp.set_ordered_dither_bank(bank), ERR_STATE)
    refused(S, lambda: sp.set_tile_levels(0, np.zeros(1024, np.uint8)), ERR_STATE)
    refused(S, lambda: sp.level_sweep(), ERR_STATE)
    refused(S, lambda: sp.score_tile_levels([0], [0]), ERR_STATE)
    ctxs[0].step_commit(buf.ptr)
    close_all(sp, ctxs)


def drive(sp, calls, every, tied, seed=1):
    """The CLI's loop on a set: scheduled calls, a level sweep behind every `every` sweeps of the palette and one behind the last call."""
    st, sweep = (0, 0, 0, 0), 0
    for call in range(calls):
        _, st, _ = sp.run_slots(1, seed=seed, first_step_id=call, state=st, window=1)
        if st[3] != sweep:
            if st[3] % every == 0:
                sp.error()
                sp.level_sweep(tied=tied)
            sweep = st[3]
    sp.error()
    sp.level_sweep(tied=tied)


def cli_set(S, imgs, bank, start, levels=None):
    """The set as the CLI builds it: the members created with the full-amplitude table, the set's bank, the stack's initialisers."""
    ctxs = [S.OptimizedImage(img, 2, 3) for img in imgs]
    for c in ctxs:
        c.set_ordered_dither(bank[start])
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    sp.set_ordered_dither_bank(bank, start)
    if levels is not None:
        for i, lv in enumerate(levels):
            sp.set_tile_levels(i, lv)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    return sp, ctxs


@pytest.mark.gpu
def test_cli_set_tile_dither(tmp_path, S):
    """--set-tile-dither writes the JSON per frame and the levels of the library driven the same way, tied and per frame;
    --set-tile-levels-in starts a run from the levels of such a file; without the new options the command writes what the
    commit before this feature wrote (tests/golden/set_levels_cli_frame{0,1}.json: recorded from that commit's CLI on an
    MI355X for these frames and arguments)."""
    imgs = [OM.with_hole(OM.image(24, 40 + i)) for i in range(2)]
    for i, im in enumerate(imgs):
        (tmp_path / ("f%d.rgba" % i)).write_bytes(im.tobytes())

    def args(tag, calls="14"):
        return [str(tmp_path / "f0.rgba"), str(tmp_path / ("%s0.json" % tag)), "--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / ("%s1.json" % tag)),
                "-c", "2", "-s", "3", "--ordered-dither", "4", "--dither-amplitude", "48", "--seed", "1", "--calls", calls]

    def files(tag):
        return [(tmp_path / ("%s%d.json" % (tag, i))).read_text() for i in range(2)]
    bank = LM.ladder(4, 48, 4)
    # without the new options
    rp = run_cli(*args("p"))
    assert rp.returncode == 0, rp.stdout + rp.stderr
    for i in range(2):
        assert (tmp_path / ("p%d.json" % i)).read_bytes() == open(os.path.join(ROOT, "tests", "golden", "set_levels_cli_frame%d.json" % i), "rb").read(), i
    # tied
    la = str(tmp_path / "a.levels.json")
    ra = run_cli(*args("a"), "--dither-levels", "4", "--set-tile-dither", "1", "--set-tile-levels-out", la)
    assert ra.returncode == 0, ra.stdout + ra.stderr
    assert "Per-tile dither levels of the set (tied): 4 levels, amplitudes 0, 16, 32, 48" in ra.stdout and ra.stdout.count("Set tile dither (tied): 96 calls") == 3
    first = json.loads(open(la).read())
    assert first["n"] == 4 and first["amplitudes"] == [0, 16, 32, 48] and first["tied"] is True and len(first["frames"]) == 2 and first["frames"][0] == first["frames"][1]
    assert len(first["frames"][0]) == 96 and sum(l != 3 for l in first["frames"][0]) > 0, "no tile left the start level: the comparison shows nothing"
    sp, ctxs = cli_set(S, imgs, bank, 3)
    drive(sp, 14, 1, True)
    assert [c.as_json() for c in ctxs] == files("a") and sp.tile_levels[:, :96].tolist() == first["frames"]
    assert files("a") != files("p")
    close_all(sp, ctxs)
    # per frame
    lb = str(tmp_path / "b.levels.json")
    rb = run_cli(*args("b"), "--dither-levels", "4", "--set-tile-dither", "1", "--set-levels", "frame", "--set-tile-levels-out", lb)
    assert rb.returncode == 0 and "Set tile dither (per frame): 192 calls" in rb.stdout, rb.stdout + rb.stderr
    second = json.loads(open(lb).read())
    assert second["tied"] is False and second["frames"][0] != second["frames"][1] and second["frames"] != first["frames"]
    sp, ctxs = cli_set(S, imgs, bank, 3)
    drive(sp, 14, 1, False)
    assert [c.as_json() for c in ctxs] == files("b") and sp.tile_levels[:, :96].tolist() == second["frames"]
    close_all(sp, ctxs)
    # a run that starts from the levels of the first: the ladder is the file's
    lc = str(tmp_path / "c.levels.json")
    rc = run_cli(*args("c", "8")[:-4], "--seed", "1", "--calls", "8", "--set-tile-dither", "1", "--set-tile-levels-in", la, "--set-tile-levels-out", lc)
    assert rc.returncode == 0 and "Tile levels of the set from" in rc.stdout, rc.stdout + rc.stderr
    lv = np.zeros((2, 1024), np.uint8)
    lv[:, :96] = first["frames"]
    sp, ctxs = cli_set(S, imgs, bank, 3, lv)
    drive(sp, 8, 1, True)
    third = json.loads(open(lc).read())
    assert [c.as_json() for c in ctxs] == files("c") and sp.tile_levels[:, :96].tolist() == third["frames"] and third["amplitudes"] == first["amplitudes"]
    close_all(sp, ctxs)
    # a file with another tile count is refused
    short = tmp_path / "short.json"
    short.write_text(json.dumps(dict(n=4, amplitudes=[0, 16, 32, 48], tied=True, frames=[[3] * 64, [3] * 64])))
    rs = run_cli(*args("s"), "--set-tile-levels-in", str(short))
    assert rs.returncode != 0 and "one level per 8 x 8 tile" in rs.stdout + rs.stderr and not os.path.exists(tmp_path / "s0.json")
