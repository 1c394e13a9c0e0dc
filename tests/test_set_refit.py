"""The refit of shared characters across the members of a shared-palette set (snesimage_shared_character_fits, _score_refits,
_refit_characters, --refit-set-tiles): behind a joint reduction every character shared by tiles of whichever members is refitted
to all of them, and the joint error decides whether the refit stays.  The model is tests/set_refit_model.py over the unchanged
CPU oracle (its premises: tests/test_set_refit_model.py): everything integer is compared exactly, errors within 1e-11 relative,
product against product bit for bit."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import backdrop_model as B
import character_model as M
import set_character_model as SM
import set_refit_model as SR
import test_set_characters as TS

pytestmark = pytest.mark.gpu

ROOT = TS.ROOT
REFIT_FUNCS = ["snesimage_shared_character_fits", "snesimage_shared_score_refits", "snesimage_shared_refit_characters"]
ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -5
REC_INTS = ("rep", "members", "touched", "gain", "changed", "scored")


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def reduced_pair(S, O, state):
    """The product and the model in the state behind the joint reduction of `state`: the product reduces on its own and must
    arrive at the model's maps."""
    imgs, count, size, flags, K, merges, oms, sb = SR.reduced_state(O, state)
    ctxs, sp, start_oms, start_sb = TS.make_set(S, O, imgs, count, size, flags)
    U0 = start_sb.state()[3]
    for o in start_oms:
        o.close()
    recs, U = sp.reduce_characters(U0 - merges, K)
    assert len(recs) == merges and U == sb.state()[3]
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette_map, o.palette_map)
    return ctxs, sp, oms, sb


def check_records(recs, want):
    assert len(recs) == len(want)
    for j, (r, w) in enumerate(zip(recs, want)):
        got = tuple(int(r[k]) for k in REC_INTS)
        assert got == tuple(w[k] for k in REC_INTS), (j, got, w)
        assert abs(float(r["error"]) - w["error"]) <= SR.REL_ERR * w["error"], (j, float(r["error"]), w["error"])


def check_fits(sp, snap):
    reps, members, gains, fits = sp.character_fits()
    assert reps.tolist() == [c["rep"] for c in snap]
    assert members.tolist() == [len(c["tiles"]) for c in snap]
    assert gains.tolist() == [c["gain"] for c in snap]
    assert np.array_equal(fits, np.array([c["fitted"] for c in snap], np.uint8).reshape(-1, 64))


def refused(S, call, code):
    with pytest.raises(S.SnesImageError) as e:
        call()
    assert e.value.code == code, str(e.value)


# ---- 1: symbols ------------------------------------------------------------------------------------------------------------

def test_set_refit_symbols_exported_declared_and_bound(S):
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    lib = _ffi.load()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    for name in REFIT_FUNCS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    assert "snesimage_shared_refit_result" in text
    assert C.sizeof(_ffi.SharedRefitResult) == 24 and S.shared.SHARED_REFIT_LOG_DTYPE.itemsize == 24
    assert S.shared.SHARED_REFIT_LOG_DTYPE.names == ("error", "gain", "rep", "members", "touched", "changed", "scored")
    n = C.c_uint32(0)
    assert lib.snesimage_shared_character_fits(None, None, None, None, None, C.byref(n)) == ERR_ARG and b"null set" in lib.snesimage_last_error()
    assert lib.snesimage_shared_score_refits(None, None, 0, None, None, None) == ERR_ARG
    assert lib.snesimage_shared_refit_characters(None, 0, None, 0, None, None, None, None) == ERR_ARG


# ---- 2: the fits -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", list(SR.STATES))
def test_character_fits_are_the_models(S, O, state):
    """Behind the joint reduction: reps, members, gains and fits exact (with dithering too: the fit reads the originals); the
    state unchanged."""
    ctxs, sp, oms, sb = reduced_pair(S, O, state)
    snap = SR.SetRefit(sb).snapshot()
    assert len(snap) >= 5 and any(len(c["touched"]) >= 2 for c in snap) and any(not np.array_equal(c["fitted"], c["cur"]) for c in snap)
    before = TS.state_of(sp, ctxs)
    check_fits(sp, snap)
    assert TS.state_of(sp, ctxs) == before
    TS.close_all(sp, ctxs, oms)


def test_character_fits_of_two_identical_frames(S, O):
    """A fresh set of two identical frames in the model's start: every class spans both members, and every fit is the character
    itself (what is best for a tile is best for its twin)."""
    imgs = [B.image(16, 30), B.image(16, 30).copy()]
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, 2, 3)
    snap = SR.SetRefit(sb).snapshot()
    assert len(snap) == sb.state()[3] and all(c["touched"] == [0, 1] for c in snap)
    check_fits(sp, snap)
    TS.close_all(sp, ctxs, oms)


# ---- 3: score_refits against the oracle --------------------------------------------------------------------------------------

@pytest.mark.parametrize("state,poison", [("rgb_32", False), ("dither_6", True)], ids=["rgb", "dither_poisoned"])
def test_score_refits_matches_the_oracle(S, O, state, poison):
    """Every eligible class, repeated until n is above one launch group (64), against the oracles with the candidates' maps set
    by hand: E', the members' errors — an untouched member's is its incumbent bit for bit — and every member's map; a class
    whose fit equals its character returns E bit for bit.  Set and members are as if the call had not been made."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    L.snesimage_debug_poison_alloc(1 if poison else 0)
    try:
        ctxs, sp, oms, sb = reduced_pair(S, O, state)
        rf = SR.SetRefit(sb)
        snap = rf.snapshot()
        F = len(ctxs)
        incs = [c.error() for c in ctxs]
        E = sp.error()
        for c, o in zip(ctxs, oms):
            assert abs(c.error() - o.error()) <= SR.REL_ERR * o.error()
        before = TS.state_of(sp, ctxs)
        order = (list(range(len(snap))) * (70 // len(snap) + 1))[:70] + [0]
        want = [rf.score(c) for c in snap]
        errs, mem, maps = sp.score_refits([snap[i]["rep"] for i in order], maps=True)
        assert len(errs) == 71 and mem.shape == (71, F) and maps.shape[:2] == (71, F)
        untouched = same = 0
        for j, i in enumerate(order):
            E1, es, ms = want[i]
            differs = not np.array_equal(snap[i]["fitted"], snap[i]["cur"])
            for m in range(F):
                assert np.array_equal(maps[j, m], ms[m]), (j, m, snap[i]["rep"])
                if m in snap[i]["touched"] and differs:
                    assert abs(mem[j, m] - es[m]) <= SR.REL_ERR * es[m], (j, m, mem[j, m], es[m])
                else:
                    assert mem[j, m] == incs[m], (j, m)
                    untouched += 1
            if differs:
                assert abs(errs[j] - E1) <= SR.REL_ERR * E1, (j, snap[i]["rep"], errs[j], E1)
                assert errs[j] == SR.joint(mem[j].tolist())
            else:
                assert errs[j] == E
                same += 1
        assert untouched > 0 and (same > 0 or state != "rgb_32")
        assert errs[-1] == errs[0] and errs[len(snap)] == errs[0] and len(set(errs.tolist())) > 2
        assert TS.state_of(sp, ctxs) == before
        assert np.array_equal(sp.score_refits([snap[i]["rep"] for i in order[:3]])[0], errs[:3])
        TS.close_all(sp, ctxs, oms)
    finally:
        L.snesimage_debug_poison_alloc(0)


# ---- 4: the sweep ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", list(SR.STATES))
def test_refit_sweep_follows_the_models_trajectory(S, O, state):
    """Two sweeps: records, every member's map, the incumbents, shared_error and U.  What the states decide — accepted calls
    that span members, rejected and skipped calls, a member's own error rising while E falls — is asserted on the model by
    tests/test_set_refit_model.py."""
    ctxs, sp, oms, sb = reduced_pair(S, O, state)
    rf = SR.SetRefit(sb)
    tps, pal = [c.tile_palettes.tobytes() for c in ctxs], sp.palette.tobytes()
    U_before = sb.state()[3]
    for sweep in range(2):
        E_before = sp.error()
        before = TS.state_of(sp, ctxs)
        want, accepted, U = rf.sweep()
        recs, acc, unique, stats = sp.refit_characters()
        check_records(recs, want)
        assert (acc, unique) == (accepted, U) and U <= U_before and sp.characters()[0] == U
        assert stats["calls"] == len(recs) and stats["accepted"] == acc and stats["useful"] == int(recs["scored"].sum()) <= stats["scored"]
        for c, o in zip(ctxs, oms):
            assert np.array_equal(c.palette_map, o.palette_map)
            assert abs(c.error() - o.error()) <= SR.REL_ERR * o.error()
        assert [c.tile_palettes.tobytes() for c in ctxs] == tps and sp.palette.tobytes() == pal
        assert sp.error() == float(recs[-1]["error"]) and sp.error() == SR.joint([c.error() for c in ctxs])
        assert (sp.error() < E_before) == (acc > 0)
        if sweep == 0:
            assert acc >= 1
        if acc == 0:
            assert TS.state_of(sp, ctxs) == before
    TS.close_all(sp, ctxs, oms)


# ---- 5: windows ------------------------------------------------------------------------------------------------------------

def test_refit_windows_are_bit_identical(S, O):
    """The state behind 26 merges (17 scored calls, 2 of them rejected) with window = 1, 2, 5 and 0 on four sets, two sweeps each:
    records, maps, members' errors and E bit for bit.  The epochs have no getter: every set still takes a call (it is
    intact), and that call goes the same on all four."""
    sets = []
    for window in (1, 2, 5, 0):
        ctxs, sp, oms, sb = reduced_pair(S, O, "dither_26")
        for o in oms:
            o.close()
        sets.append((window, sp, ctxs))
    for sweep in range(2):
        got = []
        for window, sp, ctxs in sets:
            recs, acc, unique, stats = sp.refit_characters(window)
            scored = int(recs["scored"].sum())
            assert stats["useful"] == scored <= stats["scored"] and stats["calls"] == len(recs) and stats["accepted"] == acc
            if window == 1:
                assert stats["windows"] == scored == stats["scored"]
            got.append((recs.tobytes(), acc, unique, [c.palette_map.tobytes() for c in ctxs], [c.error() for c in ctxs], sp.error()))
        assert got[0] == got[1] == got[2] == got[3]
        assert sweep > 0 or got[0][1] >= 2
    steps = [sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16) for _, sp, _ in sets]
    assert all(e == steps[0][0] and np.array_equal(b, steps[0][1]) for e, b in steps)
    states = [TS.state_of(sp, ctxs) for _, sp, ctxs in sets]
    assert all(s == states[0] for s in states)
    for _, sp, ctxs in sets:
        TS.close_all(sp, ctxs)


# ---- 6: nothing to do ------------------------------------------------------------------------------------------------------

def test_refit_with_nothing_to_do(S, O):
    # (a) two different frames straight from the start: no character is shared, 0 calls, the state identical
    imgs = [B.image(16, 30), B.image(16, 31)]
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, 1, 15)
    assert SR.SetRefit(sb).snapshot() == [] and sp.characters()[0] == 128
    before = TS.state_of(sp, ctxs)
    recs, acc, unique, stats = sp.refit_characters()
    assert len(recs) == 0 and acc == 0 and unique == 128 and len(sp.character_fits()[0]) == 0 and stats["windows"] == 0
    assert TS.state_of(sp, ctxs) == before
    TS.close_all(sp, ctxs, oms)
    # (b) two identical frames: every class is eligible and every call is skipped
    imgs = [B.image(16, 30), B.image(16, 30).copy()]
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, 2, 3)
    snap = SR.SetRefit(sb).snapshot()
    assert len(snap) > 0 and all(np.array_equal(c["fitted"], c["cur"]) for c in snap)
    before = TS.state_of(sp, ctxs)
    for window in (0, 1):
        recs, acc, unique, stats = sp.refit_characters(window)
        assert len(recs) == len(snap) and acc == 0 and unique == sb.state()[3] and stats["windows"] == 0 and stats["scored"] == 0
        assert not recs["scored"].any() and not recs["changed"].any() and (recs["error"] == before[1]).all()
        assert recs["rep"].tolist() == [c["rep"] for c in snap] and recs["touched"].tolist() == [2] * len(snap)
        assert TS.state_of(sp, ctxs) == before
    e_g, b_g = sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)  # the set is intact, and holds no merged maps
    TS.close_all(sp, ctxs, oms)
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, 2, 3)
    e_t, b_t = sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)
    assert e_g == e_t and np.array_equal(b_g, b_t)
    TS.close_all(sp, ctxs, oms)
    # (c) a fully transparent tile in each member: one class whose tiles are pinned, one of them in ANOTHER member: not eligible
    imgs = [B.image(16, 30).copy(), B.image(16, 30).copy()]
    TS.tile_px(imgs[0], 9)[..., 3] = 0
    TS.tile_px(imgs[1], 40)[..., 3] = 0
    ctxs, sp, oms, sb = TS.make_set(S, O, imgs, 2, 3)
    U, rep, flip, chars = sp.characters()
    assert rep[64 + 40] == 9 and rep[9] == 9
    snap = SR.SetRefit(sb).snapshot()
    check_fits(sp, snap)
    assert 9 not in [c["rep"] for c in snap] and len(snap) > 0
    refused(S, lambda: sp.score_refits([9]), ERR_ARG)
    before = TS.state_of(sp, ctxs)
    recs, acc, unique, stats = sp.refit_characters()
    assert 9 not in recs["rep"].tolist() and acc == 0 and TS.state_of(sp, ctxs) == before
    TS.close_all(sp, ctxs, oms)


# ---- 7: the state afterwards -------------------------------------------------------------------------------------------------

def test_the_state_after_a_refit(S, O):
    """The outputs read the refitted maps; a following step re-optimizes first and goes as on a set that never refitted."""
    ctxs, sp, oms, sb = reduced_pair(S, O, "rgb_32")
    rf = SR.SetRefit(sb)
    want, accepted, U = rf.sweep()
    recs, acc, unique, _ = sp.refit_characters()
    assert acc == accepted >= 1
    for c, o in zip(ctxs, oms):
        assert json.loads(c.as_json())["tiles"] == json.loads(o.as_json())["tiles"] and np.array_equal(c.as_rgba(), o.as_rgba())
    tiles = [json.loads(c.as_json())["tiles"] for c in ctxs]
    assert M.count_unique([t for m in tiles for t in m]) == unique == U
    tm = json.loads(sp.as_tilemap_json())
    assert SM.unflip_set_tilemap(tm) == tiles and len(tm["characters"]) == U
    assert sp.as_tilemap_json() == sb.tilemap_json()
    refused(S, lambda: ctxs[0].refit_characters(), ERR_STATE)  # a member stays lent to the set
    E = sp.error()
    imgs, count, size, flags, K, _ = SM.trajectory_inputs("rgb_2x3")
    twin_ctxs, twin, twin_oms, _ = TS.make_set(S, O, imgs, count, size, flags)
    cand = S.random_candidates(5, 0, 4)  # remapped from the palette: the twin's E_k, and the refitted maps stay
    assert np.array_equal(sp.score_candidates(0, 1, cand), twin.score_candidates(0, 1, cand)) and sp.error() == E
    e_g, b_g = sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)
    e_t, b_t = twin.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 16)
    assert e_g == e_t and np.array_equal(b_g, b_t)
    assert TS.state_of(sp, ctxs) == TS.state_of(twin, twin_ctxs)
    TS.close_all(twin, twin_ctxs, twin_oms)
    TS.close_all(sp, ctxs, oms)


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------

def test_refit_refusals_and_a_failed_workspace_allocation(S, O):
    from snesimage_amd import _ffi
    L = _ffi.load()
    ctxs, sp, oms, sb = reduced_pair(S, O, "dither_6")
    rf = SR.SetRefit(sb)
    snap = rf.snapshot()
    chars, rep, flip, U, size = sb.state()
    elig = [c["rep"] for c in snap]
    alone = next(g for g in range(sb.G) if size[g] == 1)
    follower = next(g for g in range(sb.G) if rep[g] != g and rep[g] in elig)
    before = TS.state_of(sp, ctxs)
    many = (elig * (70 // len(elig) + 1))[:70]  # above the 16 candidates the members' workspaces hold after the reduction: they grow
    # SNES_ERR_HIP: the set's refit arrays on first use (their first and fourth allocation); then, those in place (six), a
    # member's scoring workspace as it grows (its first and seventeenth allocation): set and members usable and unchanged
    for n, call in ((0, sp.refit_characters), (3, sp.character_fits), (6, lambda: sp.score_refits(many)), (16, lambda: sp.score_refits(many))):
        L.snesimage_debug_fail_alloc(n)
        try:
            refused(S, call, ERR_HIP)
        finally:
            L.snesimage_debug_fail_alloc(-1)
        assert TS.state_of(sp, ctxs) == before
        assert sp.characters()[0] == U
    # SNES_ERR_ARG: a rep beyond G, a tile that is no representative, the representative of a class of one, null pointers
    for reps in ([sb.G], [elig[0], 8191], [follower], [alone], [elig[0], follower]):
        refused(S, lambda: sp.score_refits(reps), ERR_ARG)
    assert len(sp.score_refits([])[0]) == 0
    one = (C.c_uint16 * 1)(elig[0])
    err = (C.c_double * 1)()
    assert L.snesimage_shared_score_refits(sp._s, None, 1, err, None, None) == ERR_ARG
    assert L.snesimage_shared_score_refits(sp._s, one, 1, None, None, None) == ERR_ARG
    assert TS.state_of(sp, ctxs) == before
    want, accepted, Uw = rf.sweep()
    recs, acc, unique, _ = sp.refit_characters()
    check_records(recs, want)
    assert (acc, unique) == (accepted, Uw)
    for c, o in zip(ctxs, oms):
        assert np.array_equal(c.palette_map, o.palette_map)
    # SNES_ERR_STATE: a destroyed member retires the set, said before any member is looked at
    ctxs[1].close()
    for call in (sp.character_fits, lambda: sp.score_refits([elig[0]]), lambda: sp.score_refits([]), sp.refit_characters):
        refused(S, call, ERR_STATE)
    sp.close()
    for c in (ctxs[0], ctxs[2]):
        c.close()
    for o in oms:
        o.close()


def test_more_than_8192_global_tiles_are_refused_by_the_refit(S):
    """Nine members of 256 x 256: G = 9,216.  Every new entry point answers SNES_ERR_UNSUPPORTED."""
    from snesimage_amd.synth import synth_image
    img = synth_image(0x5EED5A00, 256, 256, 0)
    ctxs = [S.OptimizedImage(img, 1, 3, device=0) for _ in range(9)]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    for call in (sp.character_fits, lambda: sp.score_refits([0]), sp.refit_characters):
        refused(S, call, ERR_UNSUPPORTED)
    TS.close_all(sp, ctxs)


# ---- 9: the headless driver --------------------------------------------------------------------------------------------------

def test_cli_refit_set_tiles(S, tmp_path):
    from snesimage_amd.synth import synth_image
    imgs = [synth_image(0x5EED5B00 + i, 256, 32, 0) for i in range(2)]
    for i, f in enumerate(imgs):
        (tmp_path / ("f%d.rgba" % i)).write_bytes(f.tobytes())

    def args(tag):
        return [str(tmp_path / "f0.rgba"), str(tmp_path / ("%s0.json" % tag)), "--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / ("%s1.json" % tag)),
                "-c", "2", "-s", "3", "--calls", "12", "--candidates", "8"]
    r0 = TS.cli(*args("p"))
    assert r0.returncode == 0, r0.stdout + r0.stderr
    plain = [json.loads((tmp_path / ("p%d.json" % i)).read_text()) for i in range(2)]
    N = M.count_unique([t for p in plain for t in p["tiles"]]) - 24
    tm_file = tmp_path / "set.tilemap.json"
    r = TS.cli(*args("o"), "--max-set-tiles", str(N), "--merge-shortlist", "4", "--refit-set-tiles", "2", "--set-tilemap", str(tm_file))
    assert r.returncode == 0, r.stdout + r.stderr
    outs = [json.loads((tmp_path / ("o%d.json" % i)).read_text()) for i in range(2)]
    tm = json.loads(tm_file.read_text())
    assert SM.unflip_set_tilemap(tm) == [o["tiles"] for o in outs] and len(tm["characters"]) <= N
    assert [o["palette"] for o in outs] == [p["palette"] for p in plain] and [o["tile_palettes"] for o in outs] == [p["tile_palettes"] for p in plain]
    sweeps = re.findall(r"Refit sweep of the set (\d+): (\d+) calls, (\d+) accepted, (\d+) skipped; error (\S+) -> (\S+); (\d+) characters", r.stdout)
    assert 1 <= len(sweeps) <= 2 and [int(s[0]) for s in sweeps] == list(range(1, len(sweeps) + 1)), r.stdout
    merged = float(re.search(r"Error: \S+ -> (\S+)", r.stdout).group(1))
    assert float(sweeps[0][4]) == merged and int(sweeps[0][2]) >= 1, r.stdout
    for j, s in enumerate(sweeps):
        assert float(s[5]) <= float(s[4]) and int(s[6]) <= N and int(s[2]) + int(s[3]) <= int(s[1])
        assert (float(s[5]) < float(s[4])) == (int(s[2]) > 0)
        if j:
            assert float(s[4]) == float(sweeps[j - 1][5])
    assert r.stdout.index("Refit sweep of the set 1") > r.stdout.index("Characters of the set:") and r.stdout.index("Refit sweep of the set 1") < r.stdout.index("Writing output")
    # the library on the CLI's own state: palette and tile palettes of the plain run, then the reduction and the sweeps
    ctxs = [S.OptimizedImage(f, 2, 3, device=0) for f in imgs]
    for c, p in zip(ctxs, plain):
        tp = np.zeros(1024, np.uint8)
        tp[:len(p["tile_palettes"])] = p["tile_palettes"]
        c.tile_palettes = tp
    words = np.array(plain[0]["palette"], np.int64).reshape(2, 16)[:, 1:4].reshape(-1)  # a row of 16 words per subpalette, slot 0 unused
    pal = np.stack([words & 31, (words >> 5) & 31, (words >> 10) & 31], axis=1).astype(np.uint8)
    for c in ctxs:
        c.palette = pal
    sp = S.SharedPalette(ctxs)
    assert [json.loads(c.as_json())["tiles"] for c in ctxs] == [p["tiles"] for p in plain]
    sp.reduce_characters(N, 4)
    for _ in range(len(sweeps)):
        sp.refit_characters()
    assert [json.loads(c.as_json())["tiles"] for c in ctxs] == [o["tiles"] for o in outs]
    assert sp.error() == float(sweeps[-1][5])
    TS.close_all(sp, ctxs)
    # without --max-set-tiles it runs behind the last optimizer call
    r = TS.cli(*args("q"), "--refit-set-tiles", "1")
    assert r.returncode == 0 and "Refit sweep of the set 1" in r.stdout and "Characters of the set:" not in r.stdout, r.stdout + r.stderr
    # wrong combinations and values: exit code 2, nothing written
    share = ["--share", "%s=%s" % (tmp_path / "f1.rgba", tmp_path / "x1.json")]
    out = tmp_path / "x0.json"
    for extra in (["--refit-set-tiles", "2"], share + ["--refit-set-tiles", "2", "--devices", "0,1"], share + ["--refit-set-tiles", "0"], share + ["--refit-set-tiles", "17"],
                  share + ["--refit-set-tiles", "x"], share + ["--refit-set-tiles", "2x"], share + ["--refit-set-tiles", "-1"], share + ["--refit-set-tiles"],
                  share + ["--refit-set-tiles", "2", "--refit-tiles", "1"], share + ["--refit-set-tiles", "2", "--max-tiles", "10"],
                  share + ["--refit-set-tiles", "2", "--tilemap", str(tmp_path / "x.tm")]):
        rr = TS.cli(str(tmp_path / "f0.rgba"), str(out), *extra, "-c", "2", "-s", "3")
        assert rr.returncode == 2, (extra, rr.stdout, rr.stderr)
        assert not out.exists() and not (tmp_path / "x1.json").exists() and not (tmp_path / "x.tm").exists()
    assert "--refit-set-tiles" in TS.cli("--help").stderr
