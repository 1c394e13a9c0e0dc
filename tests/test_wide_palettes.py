"""Subpalettes of more than 16 entries and more than 16 subpalettes, up to the 253 colours snesimage_create admits, on every
path, on a real MI355X.  The cases, images, starting states and candidate lists are tests/wide_palette_cases.py;
tests/test_wide_palettes_model.py shows on the CPU what is taken for granted here (which initialisers the reference refuses,
the empty cluster, maps that reach every 64-entry stretch, trajectories that accept and reject, the gap premise).

Integers — maps, palettes, tile palettes, decisions, JSON — are compared bit for bit, errors against the CPU oracle within the
project's 1e-11 relative, product against product bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import wide_palette_cases as W
from test_gpu_parity import REL_ERR, pair, rel, sync_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
ERR_KMEANS = -4


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def context_at(S, O, case, kind, flags_name):
    """A library context and an oracle in the starting state of (case, image, flags)."""
    C, Sz, h = W.CASES[case]
    o = W.oracle_at(O, case, kind, flags_name)
    g = S.OptimizedImage(W.start(O, case, kind, flags_name)["img"], C, Sz, **W.FLAGS[flags_name])
    sync_state(g, o)
    return g, o


def close(a, b):
    return abs(a - b) <= REL_ERR * abs(b)


def set_dither_kernels(monkeypatch, quad, wave):
    """SNES_DITHER4 / SNES_DITHERW are read when a context is created: the quad-of-lanes kernels (k_dither4*) or the
    one-lane ones (k_dither), and for the resumed runs of those the one-wave kernel (k_ditherw) or k_dither again."""
    monkeypatch.setenv("SNES_DITHER4", str(quad))
    monkeypatch.setenv("SNES_DITHERW", str(wave))


# ---- 1. the k-means initialisers --------------------------------------------------------------------------------------------

KMEANS = [(c, "rgb") for c in W.TABLE] + [(c, "perceptual") for c in W.PERCEPTUAL_TABLE] + [("W6", "dither"), ("W8", "dither")]


def assert_outputs_equal(g, o):
    assert g.as_json() == o.as_json()
    assert np.array_equal(g.as_rgba(), o.as_rgba())
    assert np.array_equal(g.palette_u16, o.palette_u16)


@pytest.mark.parametrize("case,flags_name", KMEANS, ids=["%s-%s" % k for k in KMEANS])
def test_kmeans_initialisers_bit_exact(S, O, case, flags_name):
    """initialize_tiles and recalculate_palettes at k up to 253 on three pictures each: the states and everything written
    from them (the JSON keeps 15 colours of a wider subpalette) equal the oracle's; where the reference panics in cogset
    (2 <= k < n; W1h16 with the gradient picture is the case that leaves a cluster empty) the library answers
    SNES_ERR_KMEANS and the context goes on working."""
    C, Sz, h = W.CASES[case]
    went = set()
    for kind in W.KINDS:
        g, o = pair(S, O, W.image(case, kind), C, Sz, **W.FLAGS[flags_name])
        stage = 0
        try:
            o.initialize_tiles()
            stage = 1
            g.initialize_tiles()
            assert np.array_equal(g.tile_palettes, o.tile_palettes), kind
            assert np.array_equal(g.palette, o.palette), kind
            assert np.array_equal(g.palette_map, o.palette_map), kind
            assert_outputs_equal(g, o)
            o.recalculate_palettes()
            stage = 2
            g.recalculate_palettes()
            assert np.array_equal(g.tile_palettes, o.tile_palettes), kind
            assert np.array_equal(g.palette, o.palette), kind
            assert np.array_equal(g.palette_map, o.palette_map), kind
            assert_outputs_equal(g, o)
        except RuntimeError as e:
            assert not isinstance(e, S.SnesImageError), (kind, stage, str(e))  # the oracle's refusal, not the library's
            with pytest.raises(S.SnesImageError) as ei:
                (g.initialize_tiles if stage == 0 else g.recalculate_palettes)()
            assert ei.value.code == ERR_KMEANS, (kind, stage)
        went.add(stage)
        s = W.start(O, case, kind, flags_name)  # usable afterwards, whatever happened: the starting state, remapped and measured
        assert (s["init"], s["recalc"]) == (stage >= 1, stage == 2)
        g.tile_palettes, g.palette = s["tp"], s["pal"]
        o.tile_palettes, o.palette = s["tp"], s["pal"]
        g.optimize()
        o.optimize()
        assert np.array_equal(g.palette_map, o.palette_map), kind
        assert rel(g.error(), o.error()) < REL_ERR
        g.close()
        o.close()
    assert 2 in went or case == "W2"


# ---- 2. optimize(), error() and candidate scoring ---------------------------------------------------------------------------

SCORING = [(c, "rgb", k) for c in W.TABLE for k in W.KINDS] + [(c, "perceptual", "alpha") for c in W.PERCEPTUAL_TABLE]


@pytest.mark.parametrize("case,flags_name,kind", SCORING, ids=["%s-%s-%s" % k for k in SCORING])
def test_optimize_error_and_scoring_paths(S, O, case, flags_name, kind, monkeypatch):
    """From the oracle's state: error() of the stored map, optimize(), and a candidate list (the incumbent, copies of the next
    entry and of the entry 64 places on, a repeated candidate) on the first and last slot and on both sides of entry 64 —
    through the dense path with maps, the group-sparse path (bit for bit the dense errors) and the remap alone in chunks of
    four, which does not divide the list (18 candidates, 10 with CIEDE2000)."""
    from hipmem import DeviceArray
    C, Sz, h = W.CASES[case]
    st = W.start(O, case, kind, flags_name)
    monkeypatch.setenv("SNES_SPARSE", "0")
    dense, o = context_at(S, O, case, kind, flags_name)
    monkeypatch.setenv("SNES_SPARSE", "1")
    monkeypatch.setenv("SNES_SPARSE_MIN", "1")
    sparse, o2 = context_at(S, O, case, kind, flags_name)
    o2.close()
    assert rel(dense.error(), st["err"]) < REL_ERR  # the stored map as it is
    o.optimize()
    for g in (dense, sparse):
        g.optimize()
        assert np.array_equal(g.palette_map, o.palette_map)
        assert rel(g.error(), o.error()) < REL_ERR
    pal, pmap = o.palette, o.palette_map
    n = W.SCORING_N[flags_name]
    for p, i in W.slots(case):
        cand = W.candidate_list(O, st["pal"], case, p, i, n)
        eo, mo = o.score_candidates(p, i, cand, want_maps=True)
        d_c = DeviceArray.from_numpy(cand)
        d_e = DeviceArray(n, np.float64, fill=0)
        d_m = DeviceArray((n, h, 256), np.uint8, fill=0)
        dense.score_candidates_device(p, i, d_c.ptr, n, d_e.ptr, d_m.ptr)
        dense.sync()
        assert np.array_equal(d_m.numpy(), mo), (p, i)
        print("%s %s %s slot (%d, %d): max rel err %.3e" % (case, flags_name, kind, p, i, rel(d_e.numpy(), eo)))
        assert rel(d_e.numpy(), eo) < REL_ERR, (p, i)
        ed, es = dense.score_candidates(p, i, cand), sparse.score_candidates(p, i, cand)
        assert np.array_equal(es, ed), (p, i, float(np.max(np.abs(es - ed))))
        assert rel(es, eo) < REL_ERR, (p, i)
        assert es[0] == sparse.error() and es[n - 1] == es[5]  # the incumbent colour; the repeated candidate
        d_r = DeviceArray((n, h, 256), np.uint8, fill=7)
        sparse.set_chunk(W.REMAP_CHUNK)  # divides neither list length: the last chunk is partial
        sparse.remap_candidates_device(p, i, d_c.ptr, n, d_r.ptr)
        sparse.sync()
        sparse.set_chunk(1024)
        assert np.array_equal(d_r.numpy(), mo), (p, i)
    for g in (dense, sparse):
        assert np.array_equal(g.palette, pal) and np.array_equal(g.palette_map, pmap)  # state untouched
        g.close()
    o.close()


# ---- 3. every dither kernel family at every size class ----------------------------------------------------------------------

DITHER = [(c, "dither", q, w) for c in ("W6", "W7", "W8", "W4", "W1") for q in (0, 1) for w in (0, 1)]
DITHER += [("W6", "dither_perceptual", 1, 1), ("W7", "dither_perceptual", 0, 0), ("W8", "dither_perceptual", 1, 1), ("W4h8", "dither_perceptual", 0, 0),
           ("W1", "dither_perceptual", 1, 1), ("W2", "dither", 1, 1), ("W3", "dither", 1, 1), ("W3", "dither", 0, 1)]


@pytest.mark.parametrize("case,flags_name,quad,wave", DITHER, ids=["%s-%s-quad%d-wave%d" % k for k in DITHER])
def test_dither_kernels_at_every_size_class(S, O, case, flags_name, quad, wave, monkeypatch):
    """--dither at sizes 16 (the <16> instantiations without a backdrop), 17, 84, 126 and 253 (the generic body), 1 and 2, on
    a picture with transparent pixels, with each kernel family, against the oracle (wide_palette_cases.dither_reference, shared
    by the families).  Maps compared bit for bit: optimize() of the whole image, and the candidates dithered from row 0 (maps
    asked for).  The base image and the resumed runs (score_candidates) are compared through their errors, and through the map
    that the calls behind the lists commit — the winner's resumed run: the premise file shows that a call of every case
    accepts."""
    from hipmem import DeviceArray
    C, Sz, h = W.CASES[case]
    assert (case, flags_name) in W.DITHER_CASES
    r = W.dither_reference(O, case, flags_name)
    set_dither_kernels(monkeypatch, quad, wave)
    g, o = context_at(S, O, case, "alpha", flags_name)
    o.close()
    g.optimize()
    assert np.array_equal(g.palette_map, r["pmap"])
    assert rel(g.error(), r["err"]) < REL_ERR
    n = r["n"]
    for p, i, cand, eo, mo in r["lists"]:
        d_c = DeviceArray.from_numpy(cand)
        d_e = DeviceArray(n, np.float64, fill=0)
        d_m = DeviceArray((n, h, 256), np.uint8, fill=0)
        g.score_candidates_device(p, i, d_c.ptr, n, d_e.ptr, d_m.ptr)
        g.sync()
        assert np.array_equal(d_m.numpy(), mo), (p, i)
        assert rel(d_e.numpy(), eo) < REL_ERR, (p, i)
        es = g.score_candidates(p, i, cand)
        print("%s %s quad %d wave %d slot (%d, %d): max rel err %.3e" % (case, flags_name, quad, wave, p, i, rel(es, eo)))
        assert rel(es, eo) < REL_ERR, (p, i)
    for p, i, k, eo, bo, changed, pal, pmap in r["calls"]:
        before = g.palette[p * Sz + i].copy()
        eg, bg = g.step(S.METHOD_RANDOM, p, i, 0, r["seed"], k, n)
        assert np.array_equal(bg, bo) and int(not np.array_equal(bg, before)) == changed and rel(eg, eo) < REL_ERR, (p, i)
        assert np.array_equal(g.palette, pal) and np.array_equal(g.palette_map, pmap), (p, i)
    g.close()


# ---- 4. steps and slot windows, live against the oracle ---------------------------------------------------------------------

WINDOWS = [(c, f, 1, 1) for c in ("W1", "W3", "W6", "W8") for f in ("rgb", "dither")] + [("W2", "dither", 1, 1), ("W2", "rgb", 1, 1)]
WINDOWS += [(c, "dither", 0, w) for c in ("W6", "W8") for w in (0, 1)]  # the slot windows' one-lane and one-wave resumed runs


@pytest.mark.parametrize("case,flags_name,quad,wave", WINDOWS, ids=["%s-%s-quad%d-wave%d" % k for k in WINDOWS])
def test_steps_and_slot_windows_follow_the_oracle(S, O, case, flags_name, quad, wave, monkeypatch):
    """Twelve scheduled calls across the start of the channel sweep (16 random candidates, then 32 per channel call):
    run_slots with the library's window, with a window of 7 and snesimage_step call by call, each against OracleImage.step —
    best colour and changed flag exact, error within 1e-11; final palette, map and JSON equal."""
    C, Sz, h = W.CASES[case]
    t = W.trajectory(O, case, flags_name, with_gaps=False)
    kind, seed, first, sched = t["kind"], t["seed"], t["first"], t["sched"]
    set_dither_kernels(monkeypatch, quad, wave)
    for mode in (0, 7, "step"):
        g, o = context_at(S, O, case, kind, flags_name)
        o.close()
        if mode == "step":
            log = []
            for j in range(first, first + W.N_CALLS):
                m, p, i, ch, _ = sched[j]
                before = g.palette[p * Sz + i].copy()
                e, b = g.step(m, p, i, ch, seed, j, W.N_RANDOM if m == 0 else 0)
                log.append((e, b, int(not np.array_equal(b, before))))
        else:
            out, end, stats = g.run_slots(W.N_CALLS, seed=seed, first_step_id=first, state=sched[first][1:], window=mode, n_random=W.N_RANDOM)
            assert end == sched[first + W.N_CALLS][1:] and stats["calls"] == W.N_CALLS and stats["accepted"] == t["accepted"]
            if case == "W2" and flags_name == "dither":
                assert stats["windows"] == W.N_CALLS  # one-entry subpalettes with --dither: stepped call by call
            else:
                assert stats["windows"] < W.N_CALLS, stats
            log = [(e, b, ch) for e, _, b, ch in out]
        for j, ((e, b, ch), (eo, bo, cho)) in enumerate(zip(log, t["recs"])):
            assert np.array_equal(b, bo) and ch == cho, (mode, j, b, bo, ch, cho)
            assert close(e, eo), (mode, j, e, eo)
        assert np.array_equal(g.palette, t["pal"]) and np.array_equal(g.palette_map, t["pmap"]), mode
        assert g.as_json() == t["json"], mode
        g.close()


# ---- 5. the feature layer, once per feature per wide shape, against its own model -------------------------------------------

def feature_context(S, r, C, Sz, flags=None):
    g = S.OptimizedImage(r["img"], C, Sz, **(flags or {}))
    g.tile_palettes, g.palette = r["tp"], r["pal"]
    g.optimize()
    assert np.array_equal(g.palette_map, r["pmap"])
    return g


def test_tile_moves_across_126_subpalettes(S, O):
    """W3: 40 (tile, subpalette) pairs reaching subpalettes 0, 63, 64 and 125 — the oracle's error and map of every moved
    tile — then one tile call (125 candidates in one launch set), which moves the tile to a subpalette above 64."""
    C, Sz, h = W.CASES["W3"]
    r = W.tile_moves(O, "W3", "rgb", 40)
    assert {0, 63, 64, 125} <= {s for _, s in r["pairs"]}
    g = feature_context(S, r, C, Sz)
    errs, maps = g.score_tile_moves([t for t, _ in r["pairs"]], [s for _, s in r["pairs"]], want_maps=True)
    for j, (e, m) in enumerate(r["scored"]):
        assert np.array_equal(maps[j], m), (j, r["pairs"][j])
        assert close(errs[j], e), (j, errs[j], e)
    e, sub, changed = g.tile_step(r["tile"])
    we, wsub, wch = r["step"]
    assert (sub, changed) == (wsub, wch) and wch == 1 and wsub > 64 and close(e, we)
    assert np.array_equal(g.tile_palettes, r["tp_after"]) and np.array_equal(g.palette_map, r["pmap_after"])
    assert close(g.error(), r["err_after"])
    g.close()


@pytest.mark.parametrize("case", ["W3", "W6"])
@pytest.mark.parametrize("quad", [0, 1])
def test_tile_moves_with_dither(S, O, case, quad, monkeypatch):
    """A moved tile under --dither is the whole picture dithered again (k_dither_tile / k_dither4_tile: the <16>
    instantiation at W6, the generic one at W3)."""
    C, Sz, h = W.CASES[case]
    r = W.tile_moves(O, case, "dither", 8)
    set_dither_kernels(monkeypatch, quad, 1)
    g = feature_context(S, r, C, Sz, dict(dither=True))
    errs, maps = g.score_tile_moves([t for t, _ in r["pairs"]], [s for _, s in r["pairs"]], want_maps=True)
    for j, (e, m) in enumerate(r["scored"]):
        assert np.array_equal(maps[j], m), (j, r["pairs"][j])
        assert close(errs[j], e), (j, errs[j], e)
    g.close()


def test_one_subpalette_has_no_tile_moves(S, O):
    """W1: the only subpalette is the tile's own.  A pair on it scores the incumbent; a tile call has no candidate, keeps the
    tile and reports the error as it stands; a second subpalette is an argument error."""
    C, Sz, h = W.CASES["W1"]
    g, o = context_at(S, O, "W1", "synth", "rgb")
    g.optimize()
    o.optimize()
    before = (g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.error())
    assert close(before[2], o.error())
    assert close(g.score_tile_moves([3], [0])[0], before[2])
    e, sub, changed = g.tile_step(3)
    assert (sub, changed) == (0, 0) and close(e, before[2])
    with pytest.raises(S.SnesImageError) as ei:
        g.score_tile_moves([3], [1])
    assert ei.value.code == -1
    assert (g.tile_palettes.tobytes(), g.palette_map.tobytes(), g.error()) == before
    g.close()
    o.close()


def check_merge_records(recs, want):
    assert len(recs) == len(want)
    for j, (r, w) in enumerate(zip(recs, want)):
        got = tuple(int(r[k]) for k in ("tile", "donor", "flip", "rank", "cost", "unique"))
        assert got == (w["tile"], w["donor"], w["flip"], w["rank"], w["cost"], w["unique"]), (j, got, w)
        assert close(float(r["error"]), w["error"]), (j, float(r["error"]), w["error"])


@pytest.mark.parametrize("case,merges", [("W1", 3), ("W3", 1)])
def test_characters_merges_and_refit(S, O, case, merges):
    """The character budget at 253 entries (k_merge_proxy with its largest table, 64 x 253 words of dynamic LDS: the launch has
    to go through) and at 126 subpalettes: characters, the shortlist of 64, the errors and maps of its first 8, `merges`
    reduction steps and one refit sweep, against character_model and refit_model."""
    C, Sz, h = W.CASES[case]
    r = W.characters(O, case, merges)
    assert r["ncand"] > 64 and len(r["merges"]) == merges
    g = feature_context(S, r, C, Sz)
    u, rep, flip, chars = g.characters()
    assert u == r["U0"] and np.array_equal(rep, r["rep"]) and np.array_equal(flip, r["flip"]) and np.array_equal(chars, r["chars"])
    t, b, f, cost = g.merge_shortlist(64)
    assert list(zip(cost.tolist(), t.tolist(), b.tolist(), f.tolist())) == r["short"]
    errs, maps = g.score_merges(t[:8], b[:8], f[:8], want_maps=True)
    for j, (e, m) in enumerate(r["scored"]):
        assert np.array_equal(maps[j], m), j
        assert close(errs[j], e), (j, errs[j], e)
    assert np.array_equal(g.palette_map, r["pmap"])
    recs, unique = g.reduce_characters(r["U0"] - merges, 4)
    check_merge_records(recs, r["merges"])
    assert unique == r["U"] and np.array_equal(g.palette_map, r["pmap_reduced"])
    want, accepted, U = r["refit"]
    recs, acc, unique = g.refit_characters()
    assert len(recs) == len(want) and (acc, unique) == (accepted, U)
    for j, (x, w) in enumerate(zip(recs, want)):
        got = tuple(int(x[k]) for k in ("rep", "members", "gain", "changed", "scored"))
        assert got == (w["rep"], w["members"], w["gain"], w["changed"], w["scored"]), (j, got, w)
        assert close(float(x["error"]), w["error"]), (j, float(x["error"]), w["error"])
    assert np.array_equal(g.palette_map, r["pmap_refit"])
    g.close()


def test_dither_levels_at_126_entries(S, O):
    """W4 with a ladder of four Bayer tables: the target image, optimize() against it, score_tile_levels on eight tiles and one
    level call, against level_model."""
    C, Sz, h = W.CASES["W4"]
    r = W.levels(O, "W4")
    g = S.OptimizedImage(r["img"], C, Sz)
    g.set_ordered_dither_bank(r["bank"], r["start"])
    g.tile_palettes, g.palette = r["tp"], r["pal"]
    g.optimize()
    assert np.array_equal(g.target_rgba(), r["T0"]) and np.array_equal(g.palette_map, r["map0"])
    assert close(g.error(), r["err0"])
    errs, maps = g.score_tile_levels([t for t, _ in r["pairs"]], [l for _, l in r["pairs"]], want_maps=True)
    for j, (e, m) in enumerate(r["scored"]):
        assert np.array_equal(maps[j], m), (j, r["pairs"][j])
        assert close(errs[j], e), (j, errs[j], e)
    e, level, changed = g.level_step(r["tile"])
    we, wl, wch = r["step"]
    assert (level, changed) == (wl, wch) and close(e, we)
    assert np.array_equal(g.tile_levels[:W.ntile("W4")], r["levels"][:W.ntile("W4")]) and np.array_equal(g.palette_map, r["map1"])
    g.close()


@pytest.mark.parametrize("case,proxy", [("W1", "redmean"), ("W3", "redmean"), ("W8", "cielab")])
def test_guided_calls(S, O, case, proxy):
    """All 32,768 costs and the shortlist of the first and the last slot (the floor runs over up to 252 other entries), and
    one guided call, against guided_model (redmean) and guided_lab_model (CIEDE2000 in Q16, on a posterised picture)."""
    C, Sz, h = W.CASES[case]
    r = W.guided(O, case, proxy)
    g = feature_context(S, r, C, Sz, r["flags"])
    g.guided_proxy = proxy
    assert close(g.error(), r["err"])
    for (p, i), cost, (rgb5, c) in zip(r["slots"], r["costs"], r["cands"]):
        got = g.guided_costs(p, i)
        bad = np.flatnonzero(got != cost)
        assert bad.size == 0, "%s slot (%d, %d): %d of 32768 costs differ, first at u = %d" % (case, p, i, bad.size, bad[0])
        got_rgb5, got_c = g.guided_candidates(p, i, 8)
        assert np.array_equal(got_rgb5, rgb5) and np.array_equal(got_c, c), (p, i)
    assert np.array_equal(g.palette, r["pal"]) and np.array_equal(g.palette_map, r["pmap"])
    w = r["call"]
    e, best = g.guided_step(0, 0, 8)
    e2, rgb5, best_k = g.last_step()
    assert best_k == w["best_k"] and w["changed"] == 1 and e2 == e and np.array_equal(rgb5, best)
    assert np.array_equal(best, w["rgb5"]) and close(e, w["error"])
    assert np.array_equal(g.palette, w["palette"]) and np.array_equal(g.palette_map, w["pmap"])
    g.close()


def test_shared_palette_set_at_84_entries(S, O):
    """Two frames at W8: E, the joint errors of a candidate list, a rejected and an accepted random call and one guided call
    against the summed oracles (set_guided_model)."""
    C, Sz, h = W.CASES["W8"]
    r = W.shared_set(O, "W8")
    ctxs = [S.OptimizedImage(f, C, Sz) for f in r["imgs"]]
    for c, tp in zip(ctxs, r["tiles"]):
        c.tile_palettes, c.palette = tp, r["pal"]
        c.optimize()
    sp = S.SharedPalette(ctxs)
    assert close(sp.error(), r["err"])
    for c, m in zip(ctxs, r["pmaps"]):
        assert np.array_equal(c.palette_map, m)
    p, i = r["slot"]
    assert rel(sp.score_candidates(p, i, r["cand"]), r["errs"]) < REL_ERR
    for w in r["steps"]:  # a rejected random call, then an accepted one
        e, best = sp.step(S.METHOD_RANDOM, w["slot"][0], w["slot"][1], 0, w["seed"], w["step_id"], W.N_RANDOM)
        assert sp.last_step()[3] == int(w["best_k"] >= 0) and np.array_equal(best, w["rgb5"]) and close(e, w["error"]), w["step_id"]
        assert w["best_k"] < 0 or sp.last_step()[1] == w["best_k"]
        assert np.array_equal(sp.palette, w["pal"])
        for c, m in zip(ctxs, w["pmaps"]):
            assert np.array_equal(c.palette_map, m), w["step_id"]
    w = r["guided"]
    rgb5, cost = sp.guided_candidates(0, 0, W.SET_K)
    assert np.array_equal(rgb5, w["cand"]) and np.array_equal(cost, w["costs"])
    e, best = sp.guided_step(0, 0, W.SET_K)
    assert sp.last_step()[3] == w["changed"] == 1 and sp.last_step()[1] == w["best_k"] and np.array_equal(best, w["rgb5"]) and close(e, w["error"])
    assert np.array_equal(sp.palette, w["palette"])
    for c, m in zip(ctxs, w["pmaps"]):
        assert np.array_equal(c.palette_map, m)
    sp.close()
    for c in ctxs:
        c.close()


BATCHES = [(c, f, q, w) for c in ("W7", "W6") for f, q, w in (("rgb", 1, 1), ("dither", 1, 1), ("dither", 0, 1), ("dither", 0, 0))]


@pytest.mark.parametrize("case,flags_name,quad,wave", BATCHES, ids=["%s-%s-quad%d-wave%d" % k for k in BATCHES])
def test_image_batch_equals_solo_contexts(S, case, flags_name, quad, wave, monkeypatch):
    """Two images in one library batch (the kb_* kernels: the generic body at W7, the <16> instantiations at W6, with --dither
    every family of the resumed runs): six scheduled calls, then four more, against snesimage_step on contexts of their own, bit for bit."""
    from snesimage_amd.throughput import ImageBatch
    C, Sz, h = W.CASES[case]
    flags = W.FLAGS[flags_name]
    set_dither_kernels(monkeypatch, quad, wave)
    imgs = list(enumerate(W.batch_images(case)))
    batch = ImageBatch(imgs, C, Sz, candidates=16, batched=True, groups=1, **flags)
    batch.initialize()
    solo = [S.OptimizedImage(im, C, Sz, **flags) for _, im in imgs]
    for z in solo:
        z.initialize_tiles()
        z.recalculate_palettes()
    pal = [z.palette for z in solo]
    sched, done = S.schedule(C, Sz, W.BATCH_CALLS[0] + W.BATCH_CALLS[1]), 0
    for n in W.BATCH_CALLS:  # six calls, compared; four more behind them, so that every case has an accepted call
        batch.run(n)
        for k in range(done, done + n):
            m, p, i, ch, _ = sched[k]
            for (gid, _), z in zip(imgs, solo):
                z.step(m, p, i, ch, 1 + gid, k, 16 if m == 0 else 0)
        done += n
        for z, b in zip(solo, batch.images):
            assert z.last_step()[0] == b.last_step()[0] and np.array_equal(z.last_step()[1], b.last_step()[1]), done
            assert np.array_equal(z.palette, b.palette) and np.array_equal(z.palette_map, b.palette_map), done
            assert z.error() == b.error(), done
    assert any(not np.array_equal(z.palette, q) for z, q in zip(solo, pal))  # a call was accepted
    for z in solo:
        z.close()
    batch.close()


# ---- 6. the command-line driver ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,extra,flags_name", [("W1", [], "rgb"), ("W6", ["--dither"], "dither")])
def test_cli_json_equals_the_librarys(S, tmp_path, case, extra, flags_name):
    """A raw 256 x h source through init, clustering and six optimizer calls of 12 candidates: the JSON the driver writes is
    the library's own for the same calls, byte for byte."""
    C, Sz, h = W.CASES[case]
    img = W.image(case, "synth")
    src, out = tmp_path / "in.rgba", tmp_path / "out.json"
    src.write_bytes(img.tobytes())
    r = subprocess.run([CLI, str(src), str(out), "-c", str(C), "-s", str(Sz), "--calls", "6", "--candidates", "12", "--seed", "5", *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    g = S.OptimizedImage(img, C, Sz, **W.FLAGS[flags_name])
    g.initialize_tiles()
    g.recalculate_palettes()
    for k, (m, p, i, ch, _) in enumerate(S.schedule(C, Sz, 6)):
        g.step(m, p, i, ch, 5, k, 12 if m == 0 else 0)
    assert out.read_text() == g.as_json()
    g.close()
