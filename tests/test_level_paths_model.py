"""The premises of tests/test_level_paths.py, on the CPU: every reference of tests/level_paths_model.py is built here as the GPU
tests build it (the models assert the gap premise at every comparison on the way) and asked for what makes the comparison
worth something — accepts and rejects in every stage, the clamp reached at both ends inside accepted tiles, a tile move that a
level call then answers, merges and refits accepted, and a proxy and a fit that would come out differently against T."""
import time

import numpy as np
import pytest

import character_model as CM
import level_model as LM
import level_paths_model as P


def accepted(log):
    return sum(x[2] for x in log)


def test_unclamped_sums_agree_with_the_target_image_where_nothing_clamps():
    img, bank = P.clamp_image(), P.clamp_bank(16)
    lv = P.mixed_levels(64, 3, 4)
    u = P.unclamped(img, bank, lv)
    T = LM.target_image(img, bank, lv)
    assert np.array_equal(np.clip(u, 0, 255), T[..., :3]) and (u < 0).any() and (u > 255).any()
    assert np.array_equal(T[..., 3], img[..., 3])


@pytest.mark.parametrize("n,perceptual", sorted(P.CLAMP))
def test_clamp_cases_hold_the_premises(O, n, perceptual):
    t0 = time.time()
    r = P.clamp_reference(O, n, perceptual)
    bank = r["bank"]
    assert bank.shape == (3, n, n) and not bank[0].any() and (bank[1] != bank[2]).sum() == 1
    assert {-128, 127, 0} <= set(bank[1].ravel().tolist())
    a1, a2 = accepted(r["sweep1"]), accepted(r["sweep2"])
    print("n=%d perceptual=%s: sweeps accept %d and %d of %d, smallest non-zero gap %.2e, reference in %.1f s" % (n, perceptual, a1, a2, len(r["sweep1"]), r["min_gap"], time.time() - t0))
    assert 0 < a1 < len(r["sweep1"]) and a2 < len(r["sweep2"]) and r["min_gap"] > P.MIN_GAP
    assert r["state2"]["err"] <= r["state1"]["err"] < r["err_mixed"]
    # the clamp at both ends, on opaque pixels, inside tiles whose level call accepted a table other than the all-zero one
    lv, u, opaque = r["state2"]["levels"], r["unclamped"], r["img"][..., 3] != 0
    low = high = 0
    for t in r["swept"]:
        if lv[t] == 0:
            continue
        y, x = 8 * (t // 32), 8 * (t % 32)
        low += int(((u[y:y + 8, x:x + 8] < 0).any(axis=2) & opaque[y:y + 8, x:x + 8]).sum())
        high += int(((u[y:y + 8, x:x + 8] > 255).any(axis=2) & opaque[y:y + 8, x:x + 8]).sum())
    assert low > 0 and high > 0
    assert not np.array_equal(np.clip(u, 0, 255), u) and np.array_equal(np.clip(u, 0, 255), r["state2"]["T"][..., :3])
    # the transparent tile: every level is the incumbent; the clamped tiles: levels tell apart
    for l in range(3):
        assert r["scored"][(P.WHOLE, l)][0] == r["err_mixed"]
    assert len({r["scored"][(r["clamped"][0], l)][0] for l in range(3)}) > 1
    assert len({r["scored"][(r["partly"], l)][0] for l in range(3)}) > 1
    assert len(set(r["dense"]["errs"].tolist())) > 12 and r["dense"]["errs"][5] == r["state2"]["err"]
    assert r["moved"] > 0 and len(r["moves"]) >= 4
    assert any(e != r["state3"]["err"] for e, _ in r["move_scores"])


@pytest.mark.parametrize("name", sorted(P.GEOMETRY))
def test_geometry_cases_hold_the_premises(O, name):
    t0 = time.time()
    r = P.geometry_reference(O, name)
    a = accepted(r["sweep"])
    print("%s: %d of %d accepted, smallest non-zero gap %.2e, reference in %.1f s" % (name, a, len(r["sweep"]), r["min_gap"], time.time() - t0))
    assert 0 < a < len(r["sweep"]) and r["min_gap"] > P.MIN_GAP
    assert len({lv for _, lv, ch in r["sweep"] if ch}) >= min(3, r["L"] - 1)  # several levels of the bank are taken
    others = [e for p, (e, _) in r["scored"].items() if p[1] != r["start"]]
    assert len(set(others)) > len(others) // 2 and len(others) >= 6
    if name == "L8-n4-h16":
        assert np.array_equal(r["bank"], LM.ladder(4, 56, 8))


def test_full_height_case_holds_the_premises(O):
    t0 = time.time()
    r = P.full_reference(O)
    first, last = r["sweeps"]
    print("full height: %d and %d of 8 accepted, smallest non-zero gap %.2e, reference in %.1f s" % (accepted(first), accepted(last), r["min_gap"], time.time() - t0))
    assert len(first) == len(last) == 8 and r["ntile"] == 1024
    assert 0 < accepted(first) < 8 and 0 < accepted(last) < 8 and r["min_gap"] > P.MIN_GAP
    assert last[7][2] == 1 and r["state"]["levels"][1023] != r["start"], "tile 1023 keeps its level"
    assert len({e for e, _ in r["move_scores"]}) == 8


@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_flow_holds_the_premises(O, name):
    t0 = time.time()
    r = P.flow_reference(O, name)
    logs = r["logs"]
    print("%s: accepted per stage %s, smallest non-zero gap %.2e, reference in %.1f s" % (name, {k: accepted(logs[k]) for k in P.STAGES}, r["min_gap"], time.time() - t0))
    assert r["min_gap"] > P.MIN_GAP
    for k in P.STAGES:
        assert accepted(logs[k]) > 0, k
    for k in ("tiles1", "levels1", "tiles2", "levels2"):
        assert accepted(logs[k]) < len(logs[k]), k
    moved = [t for t, x in enumerate(logs["tiles2"]) if x[2]]
    assert any(logs["levels2"][t][2] for t in moved), "no level call answers a tile move"
    assert len(logs["tiles2"]) == 32 and len(logs["tiles1"]) == len(logs["levels1"]) == r["ntile"]


@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_reassignment_holds_the_premises(O, name):
    t0 = time.time()
    r = P.reassign_reference(O, name)
    print("%s: moved %d and %d, sweeps accept %d and %d, reference in %.1f s" % (name, r["moved1"], r["moved2"], accepted(r["sweep1"]), accepted(r["sweep2"]), time.time() - t0))
    assert r["moved1"] > 0 and r["moved2"] > 0 and r["min_gap"] > P.MIN_GAP
    assert 0 < accepted(r["sweep1"]) < r["ntile"] and 0 < accepted(r["sweep2"]) < r["ntile"]
    assert not np.array_equal(r["state1"]["tp"], r["tp"]) and not np.array_equal(r["state3"]["tp"], r["state1"]["tp"])


@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_explicit_scoring_holds_the_premises(O, name):
    t0 = time.time()
    r = P.scoring_reference(O, name)
    print("%s: %d distinct errors of 70, split-phase call %s, step %s, sweep accepts %d, reference in %.1f s" % (
        name, len(set(r["errs"].tolist())), r["split"][2], r["step"][2], accepted(r["sweep"]), time.time() - t0))
    assert len(r["cand"]) == 70 and len(set(r["errs"].tolist())) > 8
    assert r["errs"][40] == r["errs"][7] and r["errs"][69] == r["errs"][3] and r["errs"][32] == r["state0"]["err"]
    if r["backdrop"]:
        assert len(set(r["errs_b"].tolist())) > 8 and r["errs_b"][32] == r["state0"]["err"]
        assert (r["state0"]["map"] == r["size"]).any(), "no pixel shows the backdrop"
    assert r["split"][2] == 1, "the split-phase call leaves the palette as it was"
    assert 0 < accepted(r["sweep"]) < r["ntile"] and r["min_gap"] > P.MIN_GAP


@pytest.mark.parametrize("name", sorted(P.PATHS))
def test_last_stages_hold_the_premises(O, name):
    t0 = time.time()
    r = P.last_reference(O, name)
    merges, K = P.BUDGET[name]
    print("%s: %d characters, winners' ranks %s, refit sweeps accept %s, reference in %.1f s" % (
        name, r["U0"], [x["rank"] for x in r["merges"]], [x["accepted"] for x in r["refits"]], time.time() - t0))
    assert 0 < accepted(r["sweep"]) < r["ntile"] and r["min_gap"] > P.MIN_GAP
    assert len(r["merges"]) == merges and r["U1"] == r["U0"] - merges
    CM.assert_trajectory_decides(r["merges"])
    assert r["refits"][0]["accepted"] >= 1 and r["refits"][0]["err"] < r["err1"]
    assert not np.array_equal(r["state"]["T"], r["img"])
    # the proxy and the fit read the original: against T both would answer differently, so the comparison tells the two apart
    assert r["shortlist_T"] != r["shortlist"]
    assert r["fits_T"] != r["fits"]
