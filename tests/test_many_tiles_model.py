"""What tests/test_many_tiles.py takes for granted about its inputs (tests/many_tiles_cases.py), shown on the CPU with the models
and the oracle alone, so that no GPU test can pass vacuously: every input reaches the tile counts, strides, waves and list
lengths it is there for, and every decision the models compare on it is decided (check_gap)."""
import numpy as np
import pytest

import character_model as M
import many_tiles_cases as T
import refit_model as R


def test_the_table_crosses_every_limit_and_stays_below_the_cap():
    counts = {T.ntile(c) for c in T.CASES}
    assert counts == {288, 544, 1024}  # the smallest heights above 256 and above 512 tiles, and the cap
    assert all(T.CASES[c][0] % 8 == 0 and T.CASES[c][0] <= 256 for c in T.CASES)
    assert {T.CASES[c][0] & (T.CASES[c][0] - 1) != 0 for c in ("T288", "T544")} == {True}  # no powers of two: pyramids 72/36/18/9 and 136/68/34/17/9
    for case, (src, dst, y, x) in T.NEAR_COPY.items():
        assert src < 512 <= dst < T.ntile(case) or src < 256 <= dst < T.ntile(case) == 288


@pytest.mark.parametrize("case", list(T.NEAR_COPY))
def test_the_near_copy_is_a_character_of_its_own(O, case):
    src, dst, y, x = T.NEAR_COPY[case]
    img = T.image(case)
    assert not np.array_equal(T.tile_px(img, src), T.tile_px(img, dst))
    assert sorted(map(tuple, T.tile_px(img, src).reshape(64, 4))) == sorted(map(tuple, T.tile_px(img, dst).reshape(64, 4)))
    cl = T.classes(O, case)
    assert cl["size"][src] == 1 and cl["size"][dst] == 1 and not cl["pinned"].any()
    top = T.shortlist(O, case)["top"]
    assert any((t, b) == (dst, src) for _, t, b, _ in top) and any((t, b) == (src, dst) for _, t, b, _ in top)


def test_288_tiles_shortlist_and_trajectory_premises(O):
    top = T.shortlist(O, "T288")["top"]
    assert T.shortlist(O, "T288")["ncand"] > 64
    assert any(t >= 256 for _, t, _, _ in top) and any(b >= 256 for _, _, b, _ in top)
    ref = T.trajectory(O, "T288", 3, 16)  # (guarded: every decision's gap is 0 or above MIN_GAP)
    assert len(ref["recs"]) == 3 and ref["U"] == ref["U0"] - 3
    M.assert_trajectory_decides(ref["recs"])
    assert any(r["tile"] >= 256 or r["donor"] >= 256 for r in ref["recs"])  # a merge is committed across the stride


@pytest.mark.parametrize("case", ["T544", "T544b"])
def test_544_tiles_shortlist_premises(O, case):
    top = T.shortlist(O, case)["top"]
    assert any(t >= 512 for _, t, _, _ in top) and any(b >= 512 for _, _, b, _ in top)
    assert any(256 <= t < 512 for _, t, _, _ in top) and any(256 <= b < 512 for _, _, b, _ in top)
    assert {f for _, _, _, f in top} == {0, 1, 2, 3}
    pairs = T.SCORED_PAIRS[case]
    assert any(t >= 512 and b < 32 for t, b, _ in pairs) and any(t < 32 and b >= 512 for t, b, _ in pairs)
    ref = T.scored_pairs(O, case)
    errs = [e for e, _ in ref["scored"]]
    assert len(set(errs) | {ref["inc"]}) == len(pairs) + 1  # every pair changes the error, each its own way
    for e in errs:
        M.check_gap(e, ref["inc"])
    if case == "T544b":  # the backdrop value occurs in the map: zero_at matters
        km = T.kmeans_state(O, case)
        assert (km["pmap"] == T.CASES[case][2]).any()


def test_1024_tiles_planted_map_premises(O):
    cl = T.classes(O, "T1024")
    reps = np.flatnonzero(cl["rep"] == np.arange(1024))
    assert cl["U"] == len(reps) >= 8 and (reps >= 64 * 3).any() and reps.max() == 1023
    assert {int(r) // 256 for r in reps} == {0, 1, 2, 3}
    assert cl["size"].max() > 1000  # everything else is one class
    s = T.shortlist(O, "T1024")
    top = s["top"]
    assert 64 < s["ncand"] < 1000  # a few hundred candidates: the model stays quick at the cap
    assert {t // 256 for _, t, _, _ in top} == {0, 1, 2, 3} == {b // 256 for _, _, b, _ in top}
    assert any(t == 1023 for _, t, _, _ in top) and any(b == 1023 for _, _, b, _ in top)
    ref = T.trajectory(O, "T1024", 1, 16)
    assert len(ref["recs"]) == 1 and ref["recs"][0]["rank"] > 0  # the objective overrules the proxy


def test_544_tiles_planted_classes_premises(O):
    planted = T.planted_classes(O)
    assert len(planted) == T.N_CLASSES and all(2 <= len(m) <= 5 for m in planted)
    assert len({t for m in planted for t in m}) == sum(len(m) for m in planted)
    ref = T.refit(O, "R544")
    by_rep = {c["rep"]: c for c in ref["snap"]}
    tp = T.kmeans_state(O, "R544")["tp"]
    flips, both = set(), 0
    for i, mem in enumerate(planted):
        c = by_rep[mem[0]]
        assert c["members"].tolist() == sorted(mem)
        assert mem[0] < 256 and any(256 <= t < 512 for t in mem) and any(t >= 512 for t in mem)
        flips |= {int(f) for f in c["flips"]}
        both += len(set(tp[c["members"]].tolist())) == 2
    assert flips == {0, 1, 2, 3} and both >= 1
    assert any(int(f) != 0 for c in ref["snap"] for t, f in zip(c["members"], c["flips"]) if t >= 512)
    assert sum(not np.array_equal(by_rep[m[0]]["fitted"], by_rep[m[0]]["cur"]) for m in planted) >= 3
    recs, accepted, U = ref["sweep"]  # (guarded)
    assert accepted >= 1 and any(r["scored"] and not r["changed"] for r in recs) and any(not r["scored"] for r in recs)
    assert ref["err"] < ref["inc"]


def test_1024_tiles_one_class_premises(O):
    ref = T.refit(O, "R1024")
    (cls,) = ref["snap"]
    assert cls["rep"] == 0 and len(cls["members"]) == 1024 and not cls["flips"].any()
    assert cls["gain"] > 0 and not np.array_equal(cls["fitted"], cls["cur"])
    o, bud = T.oracle_at(O, "R1024")
    fitted, gain, cost = R.fit_class(bud.orig, bud.pal8, bud.tp, np.arange(1024), np.zeros(1024, np.int64), M.tiles_of(o.palette_map)[0])
    o.close()
    assert np.array_equal(fitted, cls["fitted"]) and gain == cls["gain"]
    assert int(cost.max()) >= 1 << 32  # the sums over 1,024 members need more than 32 bits
    assert ref["sweep"][1:] == (1, 1) and ref["err"] < ref["inc"]
    # with one pinned member the class is not eligible
    cl = T.classes(O, "R1024p")
    assert cl["U"] == 1 and np.flatnonzero(cl["pinned"]).tolist() == [1023] and not cl["chars"][:, 0].any() and cl["chars"][:, 1:].all()
    assert T.refit(O, "R1024p")["snap"] == [] and T.refit(O, "R1024p")["sweep"] == ([], 0, 1)


@pytest.mark.parametrize("case", ["E544", "E544w", "R544", "T1024", "E1024"])
def test_export_inputs_have_characters_on_both_sides_of_tile_512(O, case):
    cl = T.classes(O, case)
    n = T.ntile(case)
    late = int((np.flatnonzero(cl["rep"] == np.arange(n)) >= 512).sum())
    assert late >= 1
    if case in ("E544", "R544", "T1024"):
        assert (cl["rep"][512:] < 512).any()
    if case == "R544":
        assert (cl["flip"][512:] != 0).any()
    if case == "E1024":
        assert late > 256
    if case == "E544w":
        assert 0x100 + cl["U"] <= 1024
    assert cl["U"] <= 1024  # char_base = 0 always fits: a picture has no more characters than tiles


def test_refill_frames_premises(O):
    imgs, ntile, tps, pal = T.set_inputs(O, "refill")
    assert len(imgs) == 3 and ntile == 224 and imgs[0].shape == (56, 256, 4)
    res = {g % 256 for g in T.REFILL_SINGULAR}
    assert len(res) == 2 and len(T.REFILL_SINGULAR) == 6  # two residues: two threads of ks_merge_proxy own all the singular donors
    ref = T.set_shortlist(O, "refill")
    assert np.flatnonzero(ref["size"] == 1).tolist() == sorted(T.REFILL_SINGULAR) and ref["ncand"] > 64
    per_thread = {}
    for _, gt, gb, f in ref["top"]:
        per_thread[(gt, gb % 256)] = per_thread.get((gt, gb % 256), 0) + 1
    assert max(per_thread.values()) >= 5  # more keys of one recipient with one thread than the four it keeps
    assert max(per_thread.values()) >= 9  # ... and more than a second fill holds


def test_past_1024_frames_premises(O):
    imgs, ntile, tps, pal = T.set_inputs(O, "past1024")
    assert len(imgs) * ntile == 1152
    s = T.set_shortlist(O, "past1024")
    assert s["ncand"] > 64 and any(gt > 1023 for _, gt, _, _ in s["top"]) and any(gb > 1023 for _, _, gb, _ in s["top"])
    (gt0, gb0, _), (gt1, gb1, _) = T.SET_PAIRS
    assert gt0 > 1023 and gb0 < ntile and gt1 < ntile and gb1 > 1023
    ref = T.set_step(O, "past1024", 16)  # (guarded)
    for (gt, _, _), (e, _) in zip(T.SET_PAIRS, ref["scored"]):
        assert e != ref["incs"][gt // ntile]
    rec = ref["rec"]
    assert rec["unique"] == s["U"] - 1
    assert max(rec["member"] * ntile + rec["tile"], rec["donor_member"] * ntile + rec["donor"]) > 1023 and rec["member"] != rec["donor_member"]
    snap = ref["snap"]
    assert max(len(c["tiles"]) for c in snap) > 256
    assert any(c["touched"] == [0, 1, 2] for c in snap)
    assert any((c["tiles"] % ntile > 255).any() for c in snap)
    differs = [c for c in snap if not np.array_equal(c["fitted"], c["cur"])]
    assert differs and any(len(c["touched"]) >= 2 and c["tiles"].max() > 1023 for c in differs)
    recs, accepted, U = ref["sweep"]
    assert sum(r["scored"] for r in recs) >= 1
