"""The character budget, the refit of shared characters and the native export above 256, 512 and 1,024 tiles, single image and
set: the tile-indexed kernels of kernels_char.hpp, kernels_char_set.hpp and kernels_export.hpp past their strides of 256, their
third wave and the cross-wave prefixes ("Tile counts").  The inputs are tests/many_tiles_cases.py; what they have
to reach is asserted here as well as on the CPU (tests/test_many_tiles_model.py), so an input that stops reaching its path
fails.  Everything integer is compared exactly, errors within 1e-11 relative, product against product on raw bytes; every
decision the models compare carries check_gap (1e-9)."""
import json

import numpy as np
import pytest

import character_model as M
import many_tiles_cases as T
import native_model as N
import set_refit_model as SR
import test_characters as TC
import test_character_refit as TR
import test_native_export as TE
import test_set_characters as TS
import test_set_refit as TSR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def product_at(S, O, case):
    """The product in the case's starting state: its own k-means start, which is the oracle's, and the planted map."""
    h, count, size, backdrop = T.CASES[case]
    km = T.kmeans_state(O, case)
    g = S.OptimizedImage(km["img"], count, size, backdrop=backdrop)
    g.initialize_tiles()
    g.recalculate_palettes()
    assert np.array_equal(g.tile_palettes, km["tp"]) and np.array_equal(g.palette_map, km["pmap"])
    pm = T.planted_map(O, case)
    if pm is not None:
        g.palette_map = pm
    return g


def zero_at(case):
    return T.CASES[case][2] if T.CASES[case][3] else None


def short_tuples(g, K):
    t, b, f, cost = g.merge_shortlist(K)
    return list(zip(cost.tolist(), t.tolist(), b.tolist(), f.tolist()))


def check_merge_records(recs, want):
    assert len(recs) == len(want)
    for j, (r, w) in enumerate(zip(recs, want)):
        got = tuple(int(r[k]) for k in ("tile", "donor", "flip", "rank", "cost", "unique"))
        assert got == (w["tile"], w["donor"], w["flip"], w["rank"], w["cost"], w["unique"]), (j, got, w)
        assert abs(float(r["error"]) - w["error"]) <= M.REL_ERR * w["error"], (j, float(r["error"]), w["error"])


# ---- 1: above 256 tiles ------------------------------------------------------------------------------------------------------

def test_shortlist_and_trajectory_above_256_tiles(S, O):
    """256 x 72: K = 1, 16 and 64 are the model's; three merges with K = 16 follow Budget.step record for record, and the state
    afterwards is the oracle's.  The top 64 hold a recipient and a donor at or above tile 256 (k_merge_proxy's second donor
    per thread, key fields above 255)."""
    case = "T288"
    g = product_at(S, O, case)
    top = T.shortlist(O, case)["top"]
    assert any(t >= 256 for _, t, _, _ in top) and any(b >= 256 for _, _, b, _ in top), "the input breaks the premise"
    before = TC.state_of(g)
    for K in (1, 16, 64):
        assert short_tuples(g, K) == top[:K], K
    assert TC.state_of(g) == before
    ref = T.trajectory(O, case, 3, 16)
    M.assert_trajectory_decides(ref["recs"])
    assert g.characters()[0] == ref["U0"]
    recs, unique = g.reduce_characters(ref["U0"] - 3, 16)
    assert unique == ref["U"] == ref["U0"] - 3
    check_merge_records(recs, ref["recs"])
    assert np.array_equal(g.palette_map, ref["pmap"])
    assert g.error() == float(recs[-1]["error"]) and abs(g.error() - ref["err"]) <= M.REL_ERR * ref["err"]
    assert TC.check_characters(g, T.image(case))[0] == unique
    assert np.array_equal(g.as_rgba(), ref["rgba"])
    g.close()


# ---- 2: above 512 tiles ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["T544", "T544b"], ids=["4x7", "4x7_backdrop"])
def test_shortlist_and_scored_merges_above_512_tiles(S, O, case):
    """256 x 136: the shortlist of 64 with recipients and donors at or above tile 512 under all four flips, and score_merges on
    pairs (t >= 512, b < 32) and (t < 32, b >= 512) against the oracle with the candidate's map set by hand."""
    g = product_at(S, O, case)
    top = T.shortlist(O, case)["top"]
    assert any(t >= 512 for _, t, _, _ in top) and any(b >= 512 for _, _, b, _ in top) and {f for _, _, _, f in top} == {0, 1, 2, 3}, "the input breaks the premise"
    before = TC.state_of(g)
    assert short_tuples(g, 64) == top
    ref = T.scored_pairs(O, case)
    pairs = T.SCORED_PAIRS[case]
    assert any(t >= 512 and b < 32 for t, b, _ in pairs) and any(t < 32 and b >= 512 for t, b, _ in pairs)
    inc = g.error()
    assert abs(inc - ref["inc"]) <= M.REL_ERR * ref["inc"]
    errs, maps = g.score_merges([c[0] for c in pairs], [c[1] for c in pairs], [c[2] for c in pairs], want_maps=True)
    for j, (e, m) in enumerate(ref["scored"]):
        assert np.array_equal(maps[j], m), (j, pairs[j])
        assert abs(errs[j] - e) <= M.REL_ERR * e, (j, pairs[j], errs[j], e)
    assert len(set(errs.tolist()) | {inc}) == len(pairs) + 1
    assert TC.state_of(g) == before
    g.close()


# ---- 3: the cap ----------------------------------------------------------------------------------------------------------------

def test_characters_shortlist_and_a_merge_at_1024_tiles(S, O):
    """256 x 256 on the planted map: a few hundred candidates among 1,024 tiles.  Class representatives sit behind the third
    wave of k_char_count and k_merge_topk; recipient 1,023 and donor 1,023 are in the top 64, and so are a recipient and a donor
    of every block of 256 tiles."""
    case = "T1024"
    g = product_at(S, O, case)
    img = T.image(case)
    cl = T.classes(O, case)
    U, rep, flip, chars = TC.check_characters(g, img)
    assert U == cl["U"] and np.array_equal(rep, cl["rep"]) and np.array_equal(flip, cl["flip"])
    assert (np.flatnonzero(rep == np.arange(1024)) >= 64 * 3).any(), "the input breaks the premise: no representative behind the third wave"
    top = T.shortlist(O, case)["top"]
    assert {t // 256 for _, t, _, _ in top} == {0, 1, 2, 3} == {b // 256 for _, _, b, _ in top}, "the input breaks the premise"
    assert any(t == 1023 for _, t, _, _ in top) and any(b == 1023 for _, _, b, _ in top), "the input breaks the premise"
    assert short_tuples(g, 64) == top
    ref = T.trajectory(O, case, 1, 16)
    recs, unique = g.reduce_characters(U - 1, 16)
    assert unique == ref["U"] == U - 1
    check_merge_records(recs, ref["recs"])
    assert np.array_equal(g.palette_map, ref["pmap"]) and g.error() == float(recs[-1]["error"])
    assert abs(g.error() - ref["err"]) <= M.REL_ERR * ref["err"]
    g.close()


# ---- 4: refit fits across the strides ------------------------------------------------------------------------------------------

def test_refit_of_classes_that_span_the_strides(S, O):
    """256 x 136 with six planted classes {r < 256, 256 <= m < 512, 512 <= m'} under all flips and in both subpalettes: fits,
    gains and members are Refit.snapshot(), score_refits is Refit.score, and one sweep at window 0 and at window 1 gives the
    model's records bit-identically."""
    case = "R544"
    ref = T.refit(O, case)
    snap = ref["snap"]
    spanning = [c for c in snap if c["members"].min() < 256 and ((c["members"] >= 256) & (c["members"] < 512)).any() and c["members"].max() >= 512 and len(c["members"]) <= 5]
    tp = T.kmeans_state(O, case)["tp"]
    assert len(spanning) == T.N_CLASSES and {int(f) for c in spanning for f in c["flips"]} == {0, 1, 2, 3}, "the input breaks the premise"
    assert any(len(set(tp[c["members"]].tolist())) == 2 for c in spanning), "the input breaks the premise: no class in both subpalettes"
    assert sum(not np.array_equal(c["fitted"], c["cur"]) for c in spanning) >= 3 and ref["sweep"][1] >= 1, "the input breaks the premise"
    ctxs = [product_at(S, O, case) for _ in range(2)]
    g = ctxs[0]
    before = TC.state_of(g)
    reps, members, gains, fits = g.character_fits()
    assert reps.tolist() == [c["rep"] for c in snap] and members.tolist() == [len(c["members"]) for c in snap]
    assert gains.tolist() == [c["gain"] for c in snap]
    assert np.array_equal(fits, np.array([c["fitted"] for c in snap], np.uint8))
    inc = g.error()
    assert abs(inc - ref["inc"]) <= M.REL_ERR * ref["inc"]
    errs, maps = g.score_refits([c["rep"] for c in snap], want_maps=True)
    for j, (c, (e, m)) in enumerate(zip(snap, ref["scored"])):
        assert np.array_equal(maps[j], m), (j, c["rep"])
        assert abs(errs[j] - e) <= M.REL_ERR * e, (j, c["rep"], errs[j], e)
        if np.array_equal(c["fitted"], c["cur"]):
            assert errs[j] == inc
    assert TC.state_of(g) == before
    want, accepted, U = ref["sweep"]
    got = []
    for window, x in zip((0, 1), ctxs):
        recs, acc, unique = x.refit_characters(window)
        TR.check_records(recs, want)
        assert (acc, unique) == (accepted, U)
        assert np.array_equal(x.palette_map, ref["pmap"]) and x.error() == float(recs[-1]["error"])
        assert abs(x.error() - ref["err"]) <= M.REL_ERR * ref["err"]
        got.append((recs.tobytes(), x.palette_map.tobytes(), x.error()))
    assert got[0] == got[1]
    assert np.array_equal(g.as_rgba(), ref["rgba"])
    for x in ctxs:
        x.close()


# ---- 5: the largest class ------------------------------------------------------------------------------------------------------

def test_refit_of_one_class_of_1024_tiles(S, O):
    """256 x 256, every tile the same 64 map values: k_refit_fit's member list is full.  The fit and its gain are fit_class over
    all 1,024 tiles; the sweep's error and the committed map are the oracle's."""
    case = "R1024"
    ref = T.refit(O, case)
    (cls,) = ref["snap"]
    assert len(cls["members"]) == 1024 and cls["gain"] > 0 and ref["sweep"][1] == 1, "the input breaks the premise"
    g = product_at(S, O, case)
    reps, members, gains, fits = g.character_fits()
    assert reps.tolist() == [0] and members.tolist() == [1024] and gains.tolist() == [cls["gain"]]
    assert np.array_equal(fits[0], cls["fitted"].astype(np.uint8))
    errs, maps = g.score_refits([0], want_maps=True)
    e, m = ref["scored"][0]
    assert np.array_equal(maps[0], m) and abs(errs[0] - e) <= M.REL_ERR * e
    recs, acc, unique = g.refit_characters()
    TR.check_records(recs, ref["sweep"][0])
    assert (acc, unique) == ref["sweep"][1:] == (1, 1)
    assert np.array_equal(g.palette_map, ref["pmap"]) and abs(g.error() - ref["err"]) <= M.REL_ERR * ref["err"]
    g.close()


def test_a_class_of_1024_tiles_with_one_pinned_is_left_alone(S, O):
    """The same on a backdrop context whose tile 1,023 has a transparent pixel where every other tile shows the backdrop: one
    class of 1,024 with a pinned member in the last place of the list.  Not eligible: no fit, no call, the state bit for bit."""
    case = "R1024p"
    cl = T.classes(O, case)
    assert cl["U"] == 1 and np.flatnonzero(cl["pinned"]).tolist() == [1023] and T.refit(O, case)["snap"] == [], "the input breaks the premise"
    g = product_at(S, O, case)
    U, rep, flip, chars = TC.check_characters(g, T.image(case), zero_at(case))
    assert U == 1 and not rep.any()
    before = TC.state_of(g)
    assert len(g.character_fits()[0]) == 0
    recs, acc, unique = g.refit_characters()
    assert len(recs) == 0 and acc == 0 and unique == 1 and TC.state_of(g) == before
    with pytest.raises(S.SnesImageError) as ei:
        g.score_refits([0])
    assert ei.value.code == TR.ERR_ARG
    g.close()


# ---- 6: export above 512 tiles -------------------------------------------------------------------------------------------------

def check_export_and_words(g, img, zero, first=512, **lay):
    """check_export, and the MAP words of the tiles from `first` on against positions counted in numpy from the stored map."""
    ex, _ = TE.check_export(g, **lay)
    rep, flip, U, _ = M.classes(M.characters(g.palette_map, img, zero))
    reps = np.flatnonzero(rep == np.arange(len(rep)))
    pos = np.searchsorted(reps, rep)
    assert ex["unique"] == U == len(reps)
    words = ex["map"].astype(np.int64)
    assert np.array_equal((words & 1023)[first:], (lay.get("char_base", 0) + pos)[first:])
    assert np.array_equal((words >> 14)[first:], flip[first:])
    return ex, rep, flip


@pytest.mark.parametrize("case,lay", [("E544", {}), ("E544w", dict(char_base=0x100)), ("R544", {}), ("T1024", {}), ("E1024", dict(char_base=0))],
                         ids=["2x3_h136", "8x15_h136", "planted_classes_h136", "planted_h256", "2x3_h256"])
def test_export_above_512_tiles(S, O, case, lay):
    """k_export_pos past its first wave (tile 512) and k_export_chr / k_export_map over more than 512 tiles: CGRAM, CHR and MAP
    are the model's encoding, the tiles from 512 on name the position counted in numpy, the render is as_rgba() bit for bit."""
    g = product_at(S, O, case)
    img = T.image(case)
    ex, rep, flip = check_export_and_words(g, img, zero_at(case), **lay)
    n = len(rep)
    late = int((np.flatnonzero(rep == np.arange(n)) >= 512).sum())
    assert late >= 1, "the input breaks the premise: no representative from tile 512 on"
    if case in ("E544", "R544", "T1024"):
        assert (rep[512:] < 512).any(), "the input breaks the premise: no tile from 512 on is drawn from a character below it"
    if case == "R544":
        assert (flip[512:] != 0).any(), "the input breaks the premise: no flipped tile from 512 on"
    if case == "E1024":
        assert late > 256, "the input breaks the premise: few representatives from tile 512 on"
    if case == "E544w":
        assert ex["bpp"] == 4 and int((ex["map"] & 1023).max()) == 0x100 + ex["unique"] - 1
    assert len(ex["chr"]) == ex["unique"] * 8 * ex["bpp"] and ex["map"].shape == (n,)
    g.close()


# ---- 7: the CLI at the SNES frame ------------------------------------------------------------------------------------------------

def test_cli_reduces_refits_and_exports_a_256x224_picture(tmp_path):
    import backdrop_model as B
    h = 224
    raw = str(tmp_path / "src.rgba")
    B.image(h, 7).tofile(raw)
    p = lambda n: str(tmp_path / n)  # noqa: E731
    common = ["-c", "8", "-s", "15", "--calls", "12", "--candidates", "8"]
    r = TC.cli(raw, p("plain.json"), *common)
    assert r.returncode == 0, r.stdout + r.stderr
    U0 = M.count_unique(json.load(open(p("plain.json")))["tiles"])
    assert U0 > 512 + 3
    r = TC.cli(raw, p("out.json"), *common, "--max-tiles", str(U0 - 3), "--merge-shortlist", "4", "--refit-tiles", "1", "--tilemap", p("tm.json"),
               "--export-cgram", p("out.cgram"), "--export-chr", p("out.chr"), "--export-map", p("out.map"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Characters: %d -> %d in 3 merges" % (U0, U0 - 3) in r.stdout and "Refit sweep 1" in r.stdout and "Wrote native data" in r.stdout, r.stdout
    js, tm = json.load(open(p("out.json"))), json.load(open(p("tm.json")))
    assert len(js["tiles"]) == 896 and M.unflip_tilemap(tm) == js["tiles"] and len(tm["characters"]) <= U0 - 3
    pal = np.array(js["palette"], np.uint16).reshape(8, 16)[:, 1:16]
    chars, rep, flip, tps = TE.pieces_of_json(js, tm, 1)
    assert chars.tolist() == js["tiles"]
    cgram, chr_, words, bpp = N.encode(chars, rep, flip, tps, pal, None, N.layout())
    assert bpp == 4 and open(p("out.cgram"), "rb").read() == cgram and open(p("out.chr"), "rb").read() == chr_
    assert open(p("out.map"), "rb").read() == words.astype("<u2").tobytes()


# ---- 8: the set shortlist's refill -----------------------------------------------------------------------------------------------

def test_set_shortlist_refills_a_threads_keys(S, O):
    """Three frames of 56 rows (G = 672): more than four of one recipient's cheapest keys belong to donors congruent mod 256, one
    thread of ks_merge_proxy, which keeps four and goes through its donors again."""
    imgs, ntile, tps, pal = T.set_inputs(O, "refill")
    ref = T.set_shortlist(O, "refill")
    per_thread = {}
    for _, gt, gb, f in ref["top"]:
        per_thread[(gt, gb % 256)] = per_thread.get((gt, gb % 256), 0) + 1
    assert max(per_thread.values()) >= 5 and ref["ncand"] > 64, "the input breaks the premise: no thread has to refill"
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, *T.SET_GEOMETRY, start="oracle")
    assert np.array_equal(sp.palette, pal)
    before = TS.state_of(sp, ctxs)
    for K in (64, 16):
        assert TS.short_tuples(sp, K, ntile) == ref["top"][:K], K
    assert sp.characters()[0] == ref["U"]
    assert TS.state_of(sp, ctxs) == before
    TS.close_all(sp, ctxs, oms)


# ---- 9, 10: scored, committed, refitted and exported past 1,024 global tiles -----------------------------------------------------

def past_1024_set(S, O):
    imgs, ntile, tps, pal = T.set_inputs(O, "past1024")
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, *T.SET_GEOMETRY, start="explicit", seed=T.PAST_1024_SEED)
    assert np.array_equal(sp.palette, pal) and all(np.array_equal(c.tile_palettes, tp) for c, tp in zip(ctxs, tps))
    for o in oms:
        o.close()
    return imgs, ntile, ctxs, sp


def reduce_once(sp, ctxs, ref, U):
    recs, unique = sp.reduce_characters(U - 1, 16)
    assert len(recs) == 1 and unique == U - 1 == ref["rec"]["unique"]
    TS.assert_record(recs[0], ref["rec"])
    for c, m in zip(ctxs, ref["pmaps"]):
        assert np.array_equal(c.palette_map, m)
    assert sp.error() == recs[0]["error"]


def test_set_merges_scored_and_committed_past_1024_global_tiles(S, O):
    """frames_past_1024() (G = 1,152): score_merges with the recipient past global tile 1,023 and the donor in member 0, and the
    reverse, against SetBudget.score; one reduction step, its record and the members' maps against SetBudget.step."""
    imgs, ntile, ctxs, sp = past_1024_set(S, O)
    ref = T.set_step(O, "past1024", 16)
    (gt0, gb0, _), (gt1, gb1, _) = T.SET_PAIRS
    assert gt0 > 1023 and gb0 < ntile and gt1 < ntile and gb1 > 1023
    before = TS.state_of(sp, ctxs)
    for c, e in zip(ctxs, ref["incs"]):
        assert abs(c.error() - e) <= M.REL_ERR * e
    cols = [[gt // ntile for gt, _, _ in T.SET_PAIRS], [gt % ntile for gt, _, _ in T.SET_PAIRS], [gb // ntile for _, gb, _ in T.SET_PAIRS], [gb % ntile for _, gb, _ in T.SET_PAIRS],
            [f for _, _, f in T.SET_PAIRS]]
    errs, maps = sp.score_merges(*cols, want_maps=True)
    for j, (e, m) in enumerate(ref["scored"]):
        assert np.array_equal(maps[j], m), j
        assert abs(errs[j] - e) <= M.REL_ERR * e, (j, errs[j], e)
        assert errs[j] != before[0][T.SET_PAIRS[j][0] // ntile][3]
    assert TS.state_of(sp, ctxs) == before
    reduce_once(sp, ctxs, ref, T.set_shortlist(O, "past1024")["U"])
    TS.close_all(sp, ctxs)


def test_set_refit_and_export_past_1024_global_tiles(S, O):
    """Behind that step: character_fits is SetRefit.snapshot() — a class of more than 256 tiles, classes in all three frames,
    members at tiles above 255 —, score_refits on the two largest classes and on the merged one, one sweep, and export_native
    with one CHR and a map per member against the model's encoding."""
    imgs, ntile, ctxs, sp = past_1024_set(S, O)
    ref = T.set_step(O, "past1024", 16)
    snap = ref["snap"]
    assert max(len(c["tiles"]) for c in snap) > 256 and any(c["touched"] == [0, 1, 2] for c in snap), "the input breaks the premise"
    assert any((c["tiles"] % ntile > 255).any() for c in snap) and any(not np.array_equal(c["fitted"], c["cur"]) for c in snap), "the input breaks the premise"
    reduce_once(sp, ctxs, ref, T.set_shortlist(O, "past1024")["U"])
    before = TS.state_of(sp, ctxs)
    TSR.check_fits(sp, snap)
    order = sorted(range(len(snap)), key=lambda i: -len(snap[i]["tiles"]))[:2] + [i for i, c in enumerate(snap) if not np.array_equal(c["fitted"], c["cur"])]
    incs, E = [c.error() for c in ctxs], sp.error()
    errs, mem, maps = sp.score_refits([snap[i]["rep"] for i in order], maps=True)
    for j, i in enumerate(order):
        E1, es, ms = ref["refits"][i]
        differs = not np.array_equal(snap[i]["fitted"], snap[i]["cur"])
        for m in range(len(ctxs)):
            assert np.array_equal(maps[j, m], ms[m]), (j, m)
            if differs and m in snap[i]["touched"]:
                assert abs(mem[j, m] - es[m]) <= SR.REL_ERR * es[m], (j, m, mem[j, m], es[m])
            else:
                assert mem[j, m] == incs[m], (j, m)
        if differs:
            assert abs(errs[j] - E1) <= SR.REL_ERR * E1 and errs[j] == SR.joint(mem[j].tolist()) and errs[j] != E
        else:
            assert errs[j] == E
    assert TS.state_of(sp, ctxs) == before
    # the export reads the reduced maps: one CHR for the set, a map per member
    u, rep, flip, chars = sp.characters()
    assert u == ref["U"] and np.array_equal(chars, ref["chars"]) and np.array_equal(rep, ref["rep"]) and np.array_equal(flip, ref["flip"])
    tps = np.concatenate([c.tile_palettes[:ntile] for c in ctxs])
    for lay in ({}, dict(char_base=1024 - u, palette_base=3, priority=1)):
        ex = sp.export_native(**lay)
        cgram, chr_, words, bpp = N.encode(ref["chars"], ref["rep"], ref["flip"], tps, ctxs[0].palette_u16.reshape(*T.SET_GEOMETRY), None, N.layout(**lay))
        assert ex["bpp"] == bpp == 4 and ex["unique"] == u
        assert ex["cgram"] == cgram and ex["chr"] == chr_ and ex["map"].shape == (3, ntile) and np.array_equal(ex["map"].reshape(-1), words)
    for m, c in enumerate(ctxs):
        TE.assert_renders_as(c, dict(ex, map=ex["map"][m]), c.as_rgba(), lay)
    assert TS.state_of(sp, ctxs) == before
    want, accepted, U = ref["sweep"]
    recs, acc, unique, stats = sp.refit_characters()
    TSR.check_records(recs, want)
    assert (acc, unique) == (accepted, U) and int(recs["scored"].sum()) >= 1
    for c, m in zip(ctxs, ref["pmaps_refit"]):
        assert np.array_equal(c.palette_map, m)
    TS.close_all(sp, ctxs)
