"""What tests/test_wide_palettes.py takes for granted about its inputs (tests/wide_palette_cases.py), shown on the CPU with
the oracle alone, so that no GPU test can pass vacuously."""
import json
import os
import subprocess

import numpy as np
import pytest

import wide_palette_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")


def test_the_table_is_inside_what_the_library_admits_and_outside_what_was_tested():
    for case, (C, S, h) in W.CASES.items():
        assert 1 <= C <= 253 and 1 <= S <= 253 and C * S <= 253 and h % 8 == 0, case
        assert C > 16 or S > 15, case
    assert W.CASES["W2"][2] * 32 // 8 > 253  # tile k-means needs k < n tiles
    assert {W.CASES[c][1] for c in ("W6", "W7", "W8", "W4", "W1")} == {16, 17, 84, 126, 253}  # the size classes of the dither kernels


@pytest.mark.parametrize("case", list(W.CASES))
def test_images_have_what_their_kind_promises(case):
    h = W.CASES[case][2]
    for kind in W.KINDS:
        assert W.image(case, kind).shape == (h, 256, 4)
    a = W.image(case, "alpha")[..., 3]
    assert (a == 0).any() and (a == 255).any()
    assert ((a == 0).any(axis=1) & (a != 0).any(axis=1)).any(), "no row holds transparent pixels beside opaque ones"
    assert not np.array_equal(W.image(case, "alpha"), W.image(case, "synth"))
    few = W.image(case, "few")
    assert len(np.unique(few.reshape(-1, 4), axis=0)) <= 3


def test_synth_variant_1_has_no_transparent_pixel_at_these_heights():
    """Why `alpha` does not come from synth_image: its transparent square starts at row 96."""
    from snesimage_amd.synth import synth_image
    for h in sorted({c[2] for c in W.CASES.values()}):
        assert np.array_equal(synth_image(W.SEED + h, 256, h, 1), synth_image(W.SEED + h, 256, h, 0))


def test_recalculate_palettes_refuses_one_entry_subpalettes(O):
    """cogset's precondition 2 <= k < n with k = 1: W2 starts from initialize_tiles alone."""
    C, S, h = W.CASES["W2"]
    o = O.OracleImage(W.image("W2", "synth"), C, S)
    o.initialize_tiles()
    assert len(np.unique(o.tile_palettes[:W.ntile("W2")])) == 253
    with pytest.raises(RuntimeError):
        o.recalculate_palettes()
    o.close()
    for fl in ("rgb", "dither"):
        s = W.start(O, "W2", "synth", fl)
        assert s["init"] and not s["recalc"]


def test_the_initialisers_go_through_or_refuse_as_the_gpu_tests_expect(O):
    """Both outcomes occur: the k-means test compares states where the reference gets through and error codes where it
    panics; the scoring tests start from hand_state where even initialize_tiles refuses."""
    seen = set()
    for case in W.TABLE:
        for kind in W.KINDS:
            s = W.start(O, case, kind, "rgb")
            seen.add((s["init"], s["recalc"]))
            if kind == "synth":
                assert s["init"] and (s["recalc"] or case == "W2"), case
    assert seen == {(True, True), (True, False), (False, False)}


def test_a_kmeans_case_ends_with_an_empty_cluster(O):
    """253 centres on 4,096 pixels: one cluster is left without a point, its centre is NaN and the entry black, unused."""
    s = W.start(O, "W1h16", "synth", "rgb")
    black = np.flatnonzero((s["pal"] == 0).all(axis=1))
    assert s["recalc"] and black.size == 1
    assert not (s["pmap"] == black[0]).any() and s["img"][..., :3].reshape(-1, 3).sum(axis=1).min() > 0  # no pixel is black: the entry is no centre of anything


def oracle_json(O, case, kind):
    o = W.oracle_at(O, case, kind, "rgb")
    text = o.as_json()
    o.close()
    return text


def test_json_keeps_fifteen_colours_of_a_wider_subpalette(O):
    for case in ("W1", "W6", "W8"):
        C, S, h = W.CASES[case]
        doc = json.loads(oracle_json(O, case, "synth"))
        assert len(doc["palette"]) == 16 * C and len(doc["tiles"]) == W.ntile(case)
        assert max(max(t) for t in doc["tiles"]) == S  # the tiles still hold every index, 1-based


@pytest.mark.parametrize("case", ["W1", "W1h16", "W4", "W4h8", "W8"])
def test_the_starting_maps_reach_every_64_entry_stretch(O, case):
    C, S, h = W.CASES[case]
    for fl in ("rgb", "perceptual") if case in ("W1", "W4h8", "W8") else ("rgb",):
        for kind in ("synth", "alpha"):
            pm = W.start(O, case, kind, fl)["pmap"]
            for lo in range(0, S, 64):
                assert ((pm >= lo) & (pm < min(lo + 64, S))).any(), (case, fl, kind, lo)
    if S == 253:
        assert W.start(O, case, "synth", "rgb")["pmap"].max() == 252


@pytest.mark.parametrize("case", list(W.CASES))
def test_slots_and_candidate_lists(O, case):
    C, S, h = W.CASES[case]
    sl = W.slots(case)
    assert sl[0] == (0, 0) and (C - 1, S - 1) in sl and len(set(sl)) == len(sl)
    if S > 64:
        assert {i for _, i in sl} >= {63, 64}
    pal = W.start(O, case, "synth", "rgb")["pal"]
    for p, i in sl:
        for n in (8, 16, 24):
            cand = W.candidate_list(O, pal, case, p, i, n)
            assert cand.shape == (n, 3) and cand.max() <= 32  # (a k-means centre >= 252 rounds to component 32)
            assert np.array_equal(cand[0], pal[p * S + i]) and np.array_equal(cand[1], pal[p * S + (i + 1) % S])
            assert np.array_equal(cand[n - 1], cand[5])
            if S > 64:
                assert np.array_equal(cand[2], pal[p * S + (i + 64) % S])
    for n in W.SCORING_N.values():  # the remap alone in chunks of REMAP_CHUNK ends on a partial chunk
        assert 8 <= n <= 24 and n % W.REMAP_CHUNK != 0 and n > W.REMAP_CHUNK


@pytest.mark.parametrize("flags_name", ["rgb", "dither"])
@pytest.mark.parametrize("case", list(W.TRAJECTORIES))
def test_short_trajectories_accept_reject_and_hold_the_gap_premise(O, case, flags_name):
    """Twelve scheduled calls around the start of the channel sweep: random and channel calls, accepted and rejected ones, and
    no two errors the acceptance compares closer than MIN_GAP without being equal — so no compared call is skipped."""
    t = W.trajectory(O, case, flags_name)
    assert len(t["recs"]) == W.N_CALLS
    assert t["methods"].count(0) == 6 and t["methods"].count(1) == 6
    assert 0 < t["accepted"] < W.N_CALLS, t["accepted"]
    assert t["min_gap"] > W.MIN_GAP, t["min_gap"]
    errs = [r[0] for r in t["recs"]]
    assert all(b <= a for a, b in zip(errs, errs[1:]))
    assert [r[2] for r in t["recs"]].count(1) == t["accepted"]


@pytest.mark.parametrize("case,flags_name", W.DITHER_CASES, ids=["%s-%s" % k for k in W.DITHER_CASES])
def test_dither_calls_accept_and_hold_the_gap_premise(O, case, flags_name):
    """The calls behind the scored lists of the --dither test: no two errors the acceptance compares are closer than MIN_GAP
    without being equal, and at least one call per case accepts, so that the committed map compared there is a winner's
    resumed run and not the map that was there before."""
    r = W.dither_reference(O, case, flags_name)
    lab = "perceptual" in flags_name
    assert len(r["lists"]) == (2 if lab else len(W.slots(case))) and len(r["calls"]) == (1 if lab else 2)
    assert r["min_gap"] > W.MIN_GAP, r["min_gap"]
    assert any(c[5] for c in r["calls"])
    accepted = [c for c in r["calls"] if c[5]]
    assert W.CASES[case][1] == 1 or not np.array_equal(accepted[-1][7], r["pmap"])  # (one-entry subpalettes: the map is all zeros)
    for p, i, cand, eo, mo in r["lists"]:
        assert eo[0] == r["err"] and np.array_equal(mo[0], r["pmap"])  # the incumbent colour
    assert W.CASES[case][1] == 1 or len({m.tobytes() for _, _, _, _, mo in r["lists"] for m in mo}) > 2  # the candidates' maps differ (a slot no pixel takes changes nothing)


def test_the_feature_models_run_wide_and_decide(O):
    """Each feature's model at its wide shape: the references exist (the models assert the gap premise at every decision they
    compare) and the decisions are not all alike."""
    r = W.tile_moves(O, "W3", "rgb", 40)
    assert {0, 63, 64, 125} <= {s for _, s in r["pairs"]} and r["step"][2] == 1 and r["step"][1] > 64
    assert len({e for e, _ in r["scored"]}) > 30
    for case in ("W3", "W6"):
        d = W.tile_moves(O, case, "dither", 8)
        assert len({e for e, _ in d["scored"]}) > 4
    c = W.characters(O, "W1", 3)
    assert c["U0"] == 32 and c["ncand"] > 64 and len(c["merges"]) == 3 and any(m["rank"] > 0 for m in c["merges"])
    assert c["refit"][1] >= 1 and all(w["scored"] for w in c["refit"][0])
    c = W.characters(O, "W3", 1)
    assert c["U0"] == 128 and len(c["merges"]) == 1 and len(c["refit"][0]) == 1
    lv = W.levels(O, "W4")
    assert lv["step"][2] == 1 and lv["min_gap"] > W.MIN_GAP and not np.array_equal(lv["T0"], lv["img"])
    for case, proxy in (("W1", "redmean"), ("W3", "redmean"), ("W8", "cielab")):
        g = W.guided(O, case, proxy)
        assert g["call"]["changed"] == 1 and g["min_gap"] > W.MIN_GAP
        assert all(cost.any() for cost in g["costs"])
    assert len(np.unique(W.guided(O, "W8", "cielab")["img"][..., :3].reshape(-1, 3), axis=0)) <= 16
    s = W.shared_set(O, "W8")
    assert [x["best_k"] >= 0 for x in s["steps"]] == [False, True]  # a rejected random call, then an accepted one: a commit on the set
    assert s["guided"]["changed"] == 1 and s["min_gap"] > W.MIN_GAP


@pytest.mark.parametrize("case", ["W6", "W7"])
def test_batch_images_pass_the_initialisers(O, case):
    C, S, h = W.CASES[case]
    for img in W.batch_images(case):
        o = O.OracleImage(img, C, S)
        o.initialize_tiles()
        o.recalculate_palettes()
        o.close()
    assert (W.batch_images(case)[1][..., 3] == 0).any()
    for fl in ("rgb", "dither"):  # the batch test's calls (16 random candidates, image i seeded 1 + i) accept at least once
        accepted = 0
        for gid, img in enumerate(W.batch_images(case)):
            o = O.OracleImage(img, C, S, **W.FLAGS[fl])
            o.initialize_tiles()
            o.recalculate_palettes()
            for k, (m, p, i, ch, _) in enumerate(O.schedule(C, S, sum(W.BATCH_CALLS))):
                before = o.palette[p * S + i].copy()
                o.step(m, p, i, ch, 1 + gid, k, 16)
                accepted += int(not np.array_equal(o.palette[p * S + i], before))
            o.close()
        assert accepted >= 1, (case, fl)


def test_cli_resume_rejects_a_17_entry_subpalette(tmp_path):
    """as_json keeps 15 colours per subpalette: --resume with -s 17 has nothing to read the other two from."""
    (tmp_path / "prev.json").write_text(json.dumps({"palette": [0] * 16 * 14, "tile_palettes": [0] * 1024, "tiles": []}))
    r = subprocess.run([CLI, "synth:1", str(tmp_path / "o.json"), "-c", "14", "-s", "17", "--resume", str(tmp_path / "prev.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--resume needs --subpalette-size <= 15" in r.stdout
    assert not (tmp_path / "o.json").exists()
