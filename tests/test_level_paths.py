"""The other single-image paths on a context with a bank of several ordered-dither tables (include/snesimage_hip.h:
snesimage_set_ordered_dither_bank: "takes every existing path as it is"), and the edges of the level paths' own geometry.

A  every kernel that computes T (k_build_target_levels, k_level_remap, k_level_commit) on banks whose offsets reach both ends of
   the clamp, with transparent and partly transparent tiles, with and without `perceptual`;
B  L = 8, a chunk smaller than one call's candidates, a pattern taller than the picture, tiles up to 1023;
C  tile moves, reassignment, explicit scoring, the split-phase step, the character budget, the refit, the tilemap and the CLI on a
   context with L > 1, with nothing between the steps.

The references are tests/level_paths_model.py (the models over the unchanged CPU oracle); tests/test_level_paths_model.py asserts
their premises on the CPU.  Target images, maps, levels, tile palettes, palettes, decisions, character tables and JSON agree bit
for bit, errors within the project's 1e-11 relative."""
import json
import os
import subprocess

import numpy as np
import pytest

import character_model as CM
import level_model as LM
import level_paths_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = P.REL_ERR


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


class Worst:
    """The largest relative error a test saw; every figure is held against the bound as it comes in."""

    def __init__(self, name):
        self.name, self.v = name, 0.0

    def see(self, got, want, where=""):
        d = abs(got - want) / abs(want)
        self.v = max(self.v, d)
        assert d <= REL_ERR, (self.name, where, got, want, d)

    def report(self):
        print("%s: worst relative error %.3e" % (self.name, self.v))


def regular(r, pal):
    """The regular entries of the model's palette: a backdrop context keeps B apart."""
    return pal.reshape(r["count"], r["msize"], 3)[:, :r["size"]].reshape(-1, 3) if r["backdrop"] else pal


def make_ctx(S, r, chunk=None, levels=None):
    g = S.OptimizedImage(r["img"], r["count"], r["size"], backdrop=r["backdrop"], **r["flags"])
    if chunk:
        g.set_chunk(chunk)
    g.set_ordered_dither_bank(r["bank"], r["start"])
    g.tile_palettes = r["tp"]
    g.palette = regular(r, r["pal"])
    if r["backdrop"]:
        g.backdrop = r["B"]
    if levels is not None:
        g.tile_levels = levels
    g.optimize()
    return g


def state_of(g):
    return g.tile_levels.tobytes(), g.target_rgba().tobytes(), g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.palette.tobytes(), g.error()


def check_state(g, r, st, w, where):
    """Levels, T, tile palettes, palette and map bit for bit, the error within the bound."""
    assert np.array_equal(g.tile_levels, st["levels"]), where
    assert np.array_equal(g.target_rgba(), st["T"]), where
    assert np.array_equal(g.tile_palettes, st["tp"]), where
    assert np.array_equal(g.palette, regular(r, st["pal"])), where
    assert np.array_equal(g.palette_map, st["map"]), where
    w.see(g.error(), st["err"], where)


def check_log(log, want, w, where):
    """A tile or level sweep's log against the model's: decisions exact, errors within the bound."""
    assert len(log) == len(want), where
    for j, (x, (e, sub, ch)) in enumerate(zip(log, want)):
        assert int(x["sub"]) == sub and int(x["changed"]) == ch, (where, j, x, (e, sub, ch))
        w.see(float(x["error"]), e, (where, j))


def check_calls(out, want, w, where):
    assert len(out) == len(want), where
    for j, (ce, rgb, changed) in enumerate(want):
        assert np.array_equal(out[j][2], rgb) and out[j][3] == changed, (where, j, out[j], (ce, rgb, changed))
        w.see(out[j][0], ce, (where, j))


def calls_bits(out):
    return [(float(e).hex(), int(k), bytes(rgb), int(ch)) for e, k, rgb, ch in out]


# ---- A: each kernel's T with values that reach the clamp -----------------------------------------------------------------------

CLAMP_IDS = ["n%d-%s" % (n, "perceptual" if p else "rgb") for n, p in sorted(P.CLAMP)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,perceptual", sorted(P.CLAMP), ids=CLAMP_IDS)
def test_clamp_target_image_and_map(S, O, n, perceptual):
    """k_build_target_levels: T behind the bank setter and behind tile_levels := mixed levels, optimize() on both."""
    r = P.clamp_reference(O, n, perceptual)
    w = Worst("target n=%d perceptual=%s" % (n, perceptual))
    g = make_ctx(S, r)
    assert np.array_equal(g.ordered_dither_bank, r["bank"]) and (g.tile_levels[:r["ntile"]] == r["start"]).all()
    assert np.array_equal(g.target_rgba(), r["T0"]) and np.array_equal(g.palette_map, r["map0"])
    w.see(g.error(), r["err0"], "start")
    g.tile_levels = r["mixed"]
    assert np.array_equal(g.tile_levels, r["mixed"]) and np.array_equal(g.target_rgba(), r["T_mixed"])
    assert not np.array_equal(r["T_mixed"], r["T0"]) and not np.array_equal(r["map_mixed"], r["map0"])
    g.optimize()
    assert np.array_equal(g.palette_map, r["map_mixed"])
    w.see(g.error(), r["err_mixed"], "mixed")
    w.report()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,perceptual", sorted(P.CLAMP), ids=CLAMP_IDS)
def test_clamp_score_tile_levels(S, O, n, perceptual):
    """k_level_remap: every level on a tile clamped at 0, a tile clamped at 255, a wholly transparent and a partly transparent
    tile, maps included; the transparent tile gives the incumbent bit for bit whatever its level."""
    r = P.clamp_reference(O, n, perceptual)
    w = Worst("pairs n=%d perceptual=%s" % (n, perceptual))
    g = make_ctx(S, r, levels=r["mixed"])
    before = state_of(g)
    tiles, levels = [p[0] for p in r["pairs"]], [p[1] for p in r["pairs"]]
    errs, maps = g.score_tile_levels(tiles, levels, want_maps=True)
    for j, p in enumerate(r["pairs"]):
        e, mp = r["scored"][p]
        assert np.array_equal(maps[j], mp), (j, p)
        w.see(errs[j], e, (j, p))
        if p[0] == P.WHOLE or p[1] == r["mixed"][p[0]]:
            assert errs[j] == before[5], (j, p)
    assert np.array_equal(g.score_tile_levels(tiles, levels), errs) and state_of(g) == before
    w.report()
    g.close()


def swept_twice(S, r, w):
    g = make_ctx(S, r, levels=r["mixed"])
    for k in (1, 2):
        log, stats = g.level_sweep()
        check_log(log, r["sweep%d" % k], w, "sweep %d" % k)
        assert stats["accepted"] == sum(ch for _, _, ch in r["sweep%d" % k])
        check_state(g, r, r["state%d" % k], w, "behind sweep %d" % k)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("n,perceptual", sorted(P.CLAMP), ids=CLAMP_IDS)
def test_clamp_sweeps_then_a_rebuild_changes_nothing(S, O, n, perceptual):
    """k_level_commit: two sweeps, the second from the levels the first left, T, map and error the model's behind each.  Then the
    setter rebuilds T from the swept levels through the first kernel and optimize() reads it: T, map and error keep their bits,
    so the commits wrote what the builder writes."""
    r = P.clamp_reference(O, n, perceptual)
    w = Worst("sweeps n=%d perceptual=%s" % (n, perceptual))
    g = swept_twice(S, r, w)
    before = state_of(g)
    g.tile_levels = g.tile_levels
    g.optimize()
    assert state_of(g) == before
    w.report()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,perceptual", sorted(P.CLAMP), ids=CLAMP_IDS)
def test_clamp_sweeps_then_the_paths_that_read_what_the_commits_wrote(S, O, n, perceptual):
    """Without a rebuild: a slot's candidates through the dense scorer (with `perceptual` its horizontal pass reads the transposed
    Lab(T)) and through the group-sparse one, optimize() of the same palette (Lab(T) as the commits left it), reassign_tiles(),
    tile moves of swept tiles and one channel call through the slot windows."""
    from hipmem import DeviceArray
    r = P.clamp_reference(O, n, perceptual)
    w = Worst("paths n=%d perceptual=%s" % (n, perceptual))
    g = swept_twice(S, r, w)
    d, (p, i) = r["dense"], r["dense"]["slot"]
    nc = len(d["cand"])
    d_c, d_e, d_m = DeviceArray.from_numpy(d["cand"]), DeviceArray(nc, np.float64, fill=0), DeviceArray((nc, 16, 256), np.uint8, fill=255)
    g.score_candidates_device(p, i, d_c.ptr, nc, d_e.ptr, d_m.ptr)  # maps asked for: the dense path
    g.sync()
    assert np.array_equal(d_m.numpy(), d["maps"])
    for j, (got, want) in enumerate(zip(d_e.numpy(), d["errs"])):
        w.see(got, want, ("dense candidate", j))
    assert np.array_equal(g.score_candidates(p, i, d["cand"]), d_e.numpy())  # the group-sparse path
    e = g.error()
    g.palette = regular(r, r["pal"])  # the map is owed again; T and Lab(T) stay as the commits wrote them
    g.optimize()
    assert np.array_equal(g.palette_map, r["state2"]["map"]) and g.error() == e
    assert g.reassign_tiles() == r["moved"]
    check_state(g, r, r["state3"], w, "reassigned")
    errs, maps = g.score_tile_moves([t for t, _ in r["moves"]], [s for _, s in r["moves"]], want_maps=True)
    for j, (e_m, map_m) in enumerate(r["move_scores"]):
        assert np.array_equal(maps[j], map_m), (j, r["moves"][j])
        w.see(errs[j], e_m, ("move", r["moves"][j]))
    out, _, _ = g.run_slots(1, seed=3, first_step_id=r["k0"], state=r["call_state"])
    check_calls(out, r["call"], w, "channel call")
    check_state(g, r, r["state4"], w, "behind the call")
    w.report()
    g.close()


# ---- B: geometry edges of the level paths ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_eight_levels_and_a_chunk_smaller_than_a_call(S, O):
    """L = 8: seven candidates per call.  Sweeps with a chunk of 64 (window 0, 1, 3), with a chunk of 4 — one call's candidates
    exceed the launch group — and level_step tile by tile: logs and states identical to each other and to the model's.  Twenty
    explicit pairs at a chunk of 4 take several launch groups."""
    r = P.geometry_reference(O, "L8-n4-h16")
    w = Worst("L8")
    seen = []
    for chunk, window in ((64, 0), (64, 1), (64, 3), (4, 0), (4, 2), (64, "step")):
        g = make_ctx(S, r, chunk=chunk)
        if window == "step":
            log = np.array([g.level_step(t) for t in range(r["ntile"])], dtype=S.api.TILE_LOG_DTYPE)
        else:
            log, stats = g.level_sweep(window=window)
            assert stats["calls"] == r["ntile"] and stats["accepted"] == sum(ch for _, _, ch in r["sweep"])
            assert window != 1 or stats["windows"] == r["ntile"]
        check_log(log, r["sweep"], w, (chunk, window))
        check_state(g, r, r["state"], w, (chunk, window))
        seen.append((log.tobytes(), state_of(g)))
        g.close()
    assert all(s == seen[0] for s in seen)
    g = make_ctx(S, r, chunk=4)
    before = state_of(g)
    errs, maps = g.score_tile_levels([p[0] for p in r["pairs"]], [p[1] for p in r["pairs"]], want_maps=True)
    for j, p in enumerate(r["pairs"]):
        e, mp = r["scored"][p]
        assert np.array_equal(maps[j], mp), (j, p)
        w.see(errs[j], e, (j, p))
        if p[1] == r["start"]:
            assert errs[j] == before[5]
    assert state_of(g) == before
    w.report()
    g.close()


@pytest.mark.gpu
def test_pattern_taller_than_the_picture(S, O):
    """n = 16 on h = 8: only the pattern's upper half is ever used."""
    r = P.geometry_reference(O, "n16-h8-L2")
    w = Worst("n16-h8")
    seen = []
    for window in (0, 1):
        g = make_ctx(S, r)
        assert np.array_equal(g.target_rgba(), r["T0"]) and np.array_equal(g.palette_map, r["map0"])
        log, _ = g.level_sweep(window=window)
        check_log(log, r["sweep"], w, window)
        check_state(g, r, r["state"], w, window)
        seen.append((log.tobytes(), state_of(g)))
        g.close()
    assert seen[0] == seen[1]
    g = make_ctx(S, r)
    errs, maps = g.score_tile_levels([p[0] for p in r["pairs"]], [p[1] for p in r["pairs"]], want_maps=True)
    for j, p in enumerate(r["pairs"]):
        assert np.array_equal(maps[j], r["scored"][p][1]), (j, p)
        w.see(errs[j], r["scored"][p][0], (j, p))
    w.report()
    g.close()


@pytest.mark.gpu
def test_full_height_first_and_last_tiles(S, O):
    """h = 256: level calls on tiles 0..7 and 1016..1023 (the level table's last entry, the transposed Lab plane's last
    column), then tile moves of the last eight tiles against T as the commits left it."""
    r = P.full_reference(O)
    w = Worst("full height")
    seen = []
    for window in (0, 1):
        g = make_ctx(S, r)
        assert np.array_equal(g.target_rgba(), r["T0"]) and np.array_equal(g.palette_map, r["map0"])
        logs = []
        for (first, n), want in zip(P.FULL_RANGES, r["sweeps"]):
            log, stats = g.level_sweep(first, n, window=window)
            check_log(log, want, w, (window, first))
            assert stats["calls"] == n
            logs.append(log.tobytes())
        check_state(g, r, r["state"], w, window)
        lv, T = g.tile_levels, g.target_rgba()
        assert lv[1023] != r["start"] and not np.array_equal(T[248:, 248:], r["T0"][248:, 248:])
        untouched = np.ones(1024, bool)
        untouched[:8] = untouched[1016:] = False
        assert (lv[untouched] == r["start"]).all() and np.array_equal(T[8:248], r["T0"][8:248])
        seen.append((logs, state_of(g)))
        if window == 1:
            errs, maps = g.score_tile_moves([t for t, _ in r["moves"]], [s for _, s in r["moves"]], want_maps=True)
            for j, (e_m, map_m) in enumerate(r["move_scores"]):
                assert np.array_equal(maps[j], map_m), r["moves"][j]
                w.see(errs[j], e_m, ("move", r["moves"][j]))
        g.close()
    assert seen[0] == seen[1]
    w.report()


# ---- C: the other paths on a context with L > 1 -----------------------------------------------------------------------------------

def run_flow(S, r, name, window, reads, w):
    """The flow on one context -> (bits of every log, final state).  reads: everything observable is read (and compared) behind
    every stage; otherwise nothing is set or read between the stages."""
    g = make_ctx(S, r)
    seed, logs = P.PATH_SEED[name], {}

    def behind(key):
        if reads:
            check_state(g, r, r["states"][key], w, (name, window, key))

    logs["pre"] = g.run_slots(2, seed=seed)[0]
    behind("pre")
    logs["tiles1"] = g.tile_sweep(window=window)[0]
    behind("tiles1")
    logs["levels1"] = g.level_sweep(window=window)[0]
    behind("levels1")
    logs["tiles2"] = g.tile_sweep(0, 32, window=window)[0]
    behind("tiles2")
    logs["levels2"] = g.level_sweep(window=window)[0]
    behind("levels2")
    logs["post"] = g.run_slots(3, seed=seed, first_step_id=r["k0"], state=r["post_state"])[0]
    for key in ("pre", "post"):
        check_calls(logs[key], r["logs"][key], w, (name, window, key))
    for key in ("tiles1", "levels1", "tiles2", "levels2"):
        check_log(logs[key], r["logs"][key], w, (name, window, key))
    check_state(g, r, r["states"]["post"], w, (name, window, "end"))
    final = state_of(g)
    g.close()
    return [calls_bits(logs[k]) if k in ("pre", "post") else logs[k].tobytes() for k in P.STAGES], final


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_calls_tile_moves_levels_with_nothing_between(S, O, name):
    """Two scheduled calls, a full tile sweep, a full level sweep, a tile sweep over the first tile row, a level sweep, three
    channel calls on one slot — on one context with no setter, no error() and no read between them, for window 0 and 1 of both
    kinds of sweep; then the same with everything read behind every stage.  All runs agree bit for bit, and with the model.  A
    level commit keeps the tile workspace, the incumbent and the map; a tile move keeps T: what either leaves stale shows in the
    next stage."""
    r = P.flow_reference(O, name)
    w = Worst("flow " + name)
    runs = [run_flow(S, r, name, window, reads, w) for window in (0, 1) for reads in (False, True)]
    assert all(x == runs[0] for x in runs)
    w.report()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_reassign_tiles_at_mixed_levels_and_behind_a_sweep(S, O, name):
    r = P.reassign_reference(O, name)
    w = Worst("reassign " + name)
    runs = []
    for reads in (False, True):
        g = make_ctx(S, r, levels=r["mixed"])
        moved1 = g.reassign_tiles()
        if reads:
            check_state(g, r, r["state1"], w, "reassigned")
        log1, _ = g.level_sweep()
        if reads:
            check_state(g, r, r["state2"], w, "swept")
        moved2 = g.reassign_tiles()
        if reads:
            check_state(g, r, r["state3"], w, "reassigned again")
        log2, _ = g.level_sweep()
        assert (moved1, moved2) == (r["moved1"], r["moved2"])
        check_log(log1, r["sweep1"], w, "sweep 1")
        check_log(log2, r["sweep2"], w, "sweep 2")
        check_state(g, r, r["state4"], w, "end")
        runs.append((log1.tobytes(), log2.tobytes(), state_of(g)))
        g.close()
    assert runs[0] == runs[1]
    w.report()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_explicit_scoring_and_split_phase_at_mixed_levels(S, O, name):
    """score_candidates on a regular slot (and on the backdrop slot) at mixed levels: 70 candidates at a chunk of 64, duplicates
    among them, with storage allocated from here on full of NaN bytes.  Then a channel call in two phases, a random call through
    step_async and a level sweep straight behind them."""
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    r = P.scoring_reference(O, name)
    w = Worst("scoring " + name)
    L.snesimage_debug_poison_alloc(1)
    try:
        g = make_ctx(S, r, chunk=64, levels=r["mixed"])
        check_state(g, r, r["state0"], w, "mixed")
        before = state_of(g)
        p, i = r["slot"]
        errs = g.score_candidates(p, i, r["cand"])
        for j, e in enumerate(r["errs"]):
            w.see(errs[j], e, ("candidate", j))
        assert errs[40] == errs[7] and errs[69] == errs[3] and errs[66] == errs[65]
        if r["backdrop"]:
            errs_b = g.score_candidates(r["count"], 0, r["cand_b"])
            for j, e in enumerate(r["errs_b"]):
                w.see(errs_b[j], e, ("backdrop candidate", j))
            assert errs_b[40] == errs_b[7] and errs_b[69] == errs_b[3]
        assert state_of(g) == before
        buf = DeviceArray(32, np.float64, fill=0)
        g.step_begin(S.METHOD_CHANNEL, 0, 1, 0, 4, r["k0"], 32, 0, 1, buf.ptr)
        g.step_commit(buf.ptr)
        e1, b1, _ = g.last_step()
        g.step_async(S.METHOD_RANDOM, 1, 0, 0, 4, 7, 0)
        e2, b2, _ = g.last_step()
        log, _ = g.level_sweep()
        w.see(e1, r["split"][0], "split-phase call")
        w.see(e2, r["step"][0], "asynchronous call")
        assert np.array_equal(b1, r["split"][1]) and np.array_equal(b2, r["step"][1])
        check_log(log, r["sweep"], w, "sweep")
        check_state(g, r, r["state3"], w, "end")
        g.close()
    finally:
        L.snesimage_debug_poison_alloc(0)
    w.report()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_last_stages_behind_a_level_sweep(S, O, name):
    """As the CLI orders them: a level sweep, characters(), the shortlist, its scores, reduce_characters, two refit sweeps, the
    tilemap — no optimize() and no read of the state in between.  The proxy and the fit read the original, not T (the CPU test
    shows that T would give other answers on this case); levels and T are left as the sweep left them."""
    r = P.last_reference(O, name)
    w = Worst("last stages " + name)
    K, zero_at = r["K"], (r["size"] if r["backdrop"] else None)
    g = make_ctx(S, r)
    log, _ = g.level_sweep()
    unique, rep, flip, chars = g.characters()
    tiles, donors, flips, costs = g.merge_shortlist(K)
    errs, maps = g.score_merges(tiles, donors, flips, want_maps=True)
    recs, U1 = g.reduce_characters(r["max_unique"], K)
    refits = [g.refit_characters() for _ in range(2)]
    tilemap = g.as_tilemap_json()
    # everything is compared from here on
    check_log(log, r["sweep"], w, "sweep")
    assert unique == r["U0"] and np.array_equal(rep, r["rep"]) and np.array_equal(flip, r["flip"]) and np.array_equal(chars, r["chars"])
    assert [(int(c), int(t), int(b), int(f)) for c, t, b, f in zip(costs, tiles, donors, flips)] == r["shortlist"]
    for j, (e, mp) in enumerate(r["short_scores"]):
        assert np.array_equal(maps[j], mp), j
        w.see(errs[j], e, ("merge candidate", j))
    assert U1 == r["U1"] and len(recs) == len(r["merges"])
    for j, (x, m) in enumerate(zip(recs, r["merges"])):
        got = tuple(int(x[k]) for k in ("tile", "donor", "flip", "rank", "cost", "unique"))
        assert got == (m["tile"], m["donor"], m["flip"], m["rank"], m["cost"], m["unique"]), (j, got, m)
        w.see(float(x["error"]), m["error"], ("merge", j))
    w.see(float(recs[-1]["error"]), r["err1"], "reduced")
    for k, ((got, acc, U), want) in enumerate(zip(refits, r["refits"])):
        assert (acc, U) == (want["accepted"], want["U"]) and len(got) == len(want["recs"]), k
        for j, (x, m) in enumerate(zip(got, want["recs"])):
            t = tuple(int(x[f]) for f in ("rep", "members", "gain", "changed", "scored"))
            assert t == (m["rep"], m["members"], m["gain"], m["changed"], m["scored"]), (k, j, t, m)
            w.see(float(x["error"]), m["error"], ("refit", k, j))
    assert np.array_equal(g.palette_map, r["refits"][1]["map"])
    w.see(g.error(), r["refits"][1]["err"], "refitted")
    assert tilemap == r["tilemap"] and g.as_tilemap_json() == tilemap
    assert json.loads(g.as_json())["tiles"] == CM.characters(g.palette_map, r["img"], zero_at).tolist()
    st = r["state"]
    assert np.array_equal(g.tile_levels, st["levels"]) and np.array_equal(g.target_rgba(), st["T"])
    assert np.array_equal(g.tile_palettes, st["tp"]) and np.array_equal(g.palette, regular(r, st["pal"]))
    w.report()
    g.close()


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def drive(g, calls, seed, tile_moves, reassign, max_tiles, refits):
    """The CLI's order on the library, error() calls included: scheduled calls; behind every sweep of the palette the
    reassignment or the tile sweep, then a level sweep; behind the last call a level sweep, the character budget (max_tiles(U)
    gives the budget from the count reached) and the refit sweeps.  -> (tiles moved, the budget, merges)."""
    st, sweep, moved = (0, 0, 0, 0), 0, 0

    def level_sweep():
        g.error()
        g.level_sweep()
        g.error()

    for call in range(calls):
        _, st, _ = g.run_slots(1, seed=seed, first_step_id=call, state=st, window=1)
        if st[3] != sweep:
            if reassign:
                moved += g.reassign_tiles()
            if tile_moves:
                moved += g.tile_sweep()[1]["accepted"]
                g.error()
            level_sweep()
            sweep = st[3]
    level_sweep()
    U0 = g.characters()[0]
    g.error()
    budget = max_tiles(U0)
    recs, _ = g.reduce_characters(budget)
    g.error()
    for _ in range(refits):
        g.error()
        _, acc, _ = g.refit_characters()
        g.error()
        if acc == 0:
            break
    return moved, budget, len(recs)


@pytest.mark.gpu
@pytest.mark.parametrize("backdrop", [False, True], ids=["tile-moves", "backdrop-reassign"])
def test_cli_tile_dither_with_tile_moves_budget_refit_and_tilemap(tmp_path, S, backdrop):
    """The CLI with --tile-dither beside --tile-moves (or --backdrop and --reassign-tiles), --max-tiles, --refit-tiles, --tilemap
    and --tile-levels-out writes, byte for byte, what the library writes when driven in the CLI's order."""
    img = LM.with_hole(LM.image(64, 40))
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    bank = LM.ladder(4, 48, 4)
    g = S.OptimizedImage(img, 2, 3, backdrop=backdrop)
    g.set_ordered_dither_bank(bank, 3)
    g.initialize_tiles()
    g.recalculate_palettes()
    tp0 = g.tile_palettes
    moved, budget, merges = drive(g, 15, 1, 0 if backdrop else 1, 1 if backdrop else 0, lambda U: U - 6, 2)
    levels = g.tile_levels[:256].tolist()
    assert moved > 0 and not np.array_equal(g.tile_palettes, tp0), "no tile moved: the comparison shows nothing"
    assert sum(l != 3 for l in levels) > 0, "no tile left the start level: the comparison shows nothing"
    assert merges == 6 and g.characters()[0] == budget
    out, lv, tm = (str(tmp_path / f) for f in ("o.json", "o.levels.json", "o.tilemap.json"))
    flags = ["-c", "2", "-s", "3", "--ordered-dither", "4", "--dither-amplitude", "48", "--seed", "1", "--calls", "15", "--tile-dither", "1", "--dither-levels", "4",
             "--max-tiles", str(budget), "--refit-tiles", "2", "--tilemap", tm, "--tile-levels-out", lv]
    flags += ["--backdrop", "--reassign-tiles", "1"] if backdrop else ["--tile-moves", "1"]
    res = run_cli(str(src), out, *flags)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Tile dither: 256 calls" in res.stdout and "in 6 merges (budget %d)" % budget in res.stdout and "Refit sweep 1" in res.stdout
    assert open(out).read() == g.as_json()
    assert open(tm).read() == g.as_tilemap_json()
    want = json.dumps({"n": 4, "amplitudes": [0, 16, 32, 48], "levels": levels}, separators=(",", ":"))
    assert open(lv).read() == want
    g.close()
