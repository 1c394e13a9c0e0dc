"""The backdrop colour of a shared-palette set (snesimage_shared_create_backdrop, SharedPalette(..., backdrop=...), cli
--set-backdrop; DESIGN 5c'').

The model (tests/set_backdrop_model.py) is one backdrop_model.Model per member over the unchanged CPU oracle: the expanded
context (C, S + 1) whose column S holds the set's B; joint errors are the members' summed in member order.  Errors agree
within the project's 1e-11 relative; palettes, B, maps, JSON and scheduler states bit for bit.  The premises of the
trajectories (the gap between compared errors; a backdrop call that accepts and one that rejects) are proved on the CPU by
tests/test_set_backdrop_model.py.  256 x 32, (C, S) = (2, 3), 16 random candidates unless noted."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import backdrop_model as M
import set_backdrop_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL = 1e-11
ERR_ARG, ERR_STATE, UNSUPPORTED = -1, -3, -5
NEW_SYMBOLS = ["snesimage_shared_create_backdrop", "snesimage_shared_get_backdrop_rgb5", "snesimage_shared_set_backdrop_rgb5"]


def rel(a, b):
    return abs(a - b) / abs(b)


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_set_backdrop_symbols():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    out = C.c_void_p()
    assert lib.snesimage_shared_create_backdrop(None, 2, None, C.byref(out)) == ERR_ARG and not out.value
    empty = (C.c_void_p * 1)(None)
    assert lib.snesimage_shared_create_backdrop(empty, 1, None, C.byref(out)) == ERR_ARG and b"null context" in lib.snesimage_last_error()
    assert lib.snesimage_shared_get_backdrop_rgb5(None, None) == ERR_ARG and lib.snesimage_shared_set_backdrop_rgb5(None, None) == ERR_ARG


def test_cli_set_backdrop_argument_rules(tmp_path):
    """Everything is said while parsing: the sources do not exist, so a refusal behind a file or device access would exit 1."""
    missing, out, other = str(tmp_path / "none.png"), str(tmp_path / "o.json"), str(tmp_path / "p.json")
    share = ["--share", "%s=%s" % (missing, other)]
    for flag in (["--set-backdrop"], ["--set-backdrop-fixed", "0,0,8"]):
        r = run_cli(missing, out, *flag)  # needs --share; names the single-image option, in the wording of --set-tile-dither
        assert r.returncode == 2 and flag[0] in r.stderr and "needs '--share <SOURCE=TARGET>'" in r.stderr and "--backdrop)" in r.stderr, r.stderr
        for extra, name in [(["--devices", "0,1"], "--devices"), (["--backdrop"], "--backdrop"), (["--backdrop-fixed", "1,2,3"], "--backdrop-fixed"),
                            (["--max-set-tiles", "100"], "--max-set-tiles"), (["--refit-set-tiles", "2"], "--refit-set-tiles"),
                            (["--set-tilemap", other], "--set-tilemap"), (["--ordered-dither", "4", "--set-tile-dither", "1"], "--set-tile-dither"),
                            (["--ordered-dither", "4", "--set-levels", "frame"], "--set-levels"),
                            (["--ordered-dither", "4", "--set-tile-levels-out", other], "--set-tile-levels-out"),
                            (["--ordered-dither", "4", "--set-tile-levels-in", other], "--set-tile-levels-in")]:
            r = run_cli(missing, out, *share, *flag, *extra)
            assert r.returncode == 2 and "cannot be used with" in r.stderr and name in r.stderr and flag[0] in r.stderr, (flag, extra, r.stderr)
        for sizes in (["-s", "16"], ["-c", "16", "-s", "15"]):  # the sizes --backdrop refuses
            r = run_cli(missing, out, *share, *flag, *sizes)
            assert r.returncode == 2 and "--subpalette-size <= 15" in r.stderr and "<= 253" in r.stderr, r.stderr
    for bad in ("1,2", "1,2,32", "1,2,3x"):
        r = run_cli(missing, out, *share, "--set-backdrop-fixed", bad)
        assert r.returncode == 2 and "--set-backdrop-fixed" in r.stderr and "invalid value" in r.stderr
    r = run_cli(missing, out, *share, "--set-backdrop", "--set-backdrop-fixed", "1,2,3")
    assert r.returncode == 2 and "cannot be used with" in r.stderr
    r = run_cli(missing, out, *share, "--backdrop")  # unchanged: its present message and exit code
    assert r.returncode == 1 and "do not carry the backdrop colour yet" in r.stderr
    r = run_cli(missing, out, *share, "--resume", missing)  # --resume stays refused for a plain set
    assert r.returncode == 2 and "--resume" in r.stderr
    assert "Using source image" not in r.stdout and not os.path.exists(out) and not os.path.exists(other)
    h = run_cli("--help")
    assert h.returncode == 0 and "--set-backdrop " in h.stderr and "--set-backdrop-fixed <R,G,B>" in h.stderr


# ---- on the GPU ----------------------------------------------------------------------------------------------------------

def make_set(S, imgs, Cn, Sz, flags, backdrop=True, chunk=64, ordered_dither=None):
    ctxs = [S.OptimizedImage(f, Cn, Sz, backdrop=True, **flags) for f in imgs]
    for c in ctxs:
        c.set_chunk(chunk)
    return ctxs, S.SharedPalette(ctxs, ordered_dither=ordered_dither, backdrop=backdrop)


def close_all(sp, ctxs):
    sp.close()
    for c in ctxs:
        c.close()


def start(S, O, imgs, Cn, Sz, flags, B0=None):
    """A backdrop set behind its initialisers and the model in the same state."""
    ctxs, sp = make_set(S, imgs, Cn, Sz, flags)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    if B0 is not None:
        sp.backdrop = B0
    return ctxs, sp


def assert_same_state(ctxs, sp, sm):
    assert np.array_equal(sp.palette, sm.regular) and np.array_equal(sp.backdrop, sm.B)
    for c, m in zip(ctxs, sm.m):
        assert np.array_equal(c.palette, sm.regular) and np.array_equal(c.backdrop, sm.B)
        assert np.array_equal(c.tile_palettes, m.o.tile_palettes) and np.array_equal(c.palette_map, m.palette_map)


@pytest.mark.gpu
def test_creation(S, O):
    """F = 3 with the transparent square (at 256 x 104, the smallest height that shows it)."""
    from snesimage_amd import _ffi
    L = _ffi.load()
    imgs = SM.creation_frames(3)
    want = SM.stack_backdrop(O, imgs, {})
    assert not any(np.array_equal(M.mean_backdrop(f), want) for f in imgs)  # the stack's mean is no member's own
    ctxs, sp = make_set(S, imgs, 2, 3, {})
    assert sp.has_backdrop and sp.sub_size == 3 and sp.palette.shape == (6, 3)
    assert np.array_equal(sp.backdrop, want)
    for c in ctxs:  # a member's own getters keep working
        assert np.array_equal(c.backdrop, want) and c.palette.shape == (6, 3) and c.palette_map.max() <= 3
    sp.backdrop = [3, 30, 7]
    assert all(np.array_equal(c.backdrop, [3, 30, 7]) for c in ctxs)
    with pytest.raises(S.SnesImageError) as e:
        sp.backdrop = [3, 32, 7]
    assert e.value.code == ERR_ARG
    reg = (np.arange(18, dtype=np.uint8).reshape(6, 3) * 5) % 32  # the palette setter takes the regular entries and leaves B
    sp.palette = reg
    assert np.array_equal(sp.palette, reg) and np.array_equal(sp.backdrop, [3, 30, 7])
    sm = SM.SetModel(O, imgs, 2, 3, {}, init=False)
    sm.set_state(reg, [3, 30, 7])
    assert_same_state(ctxs, sp, sm)
    assert rel(sp.error(), sm.error()) < REL
    sp.close()
    sp = S.SharedPalette(ctxs, backdrop=[1, 2, 30])  # the given colour
    assert np.array_equal(sp.backdrop, [1, 2, 30]) and all(np.array_equal(c.backdrop, [1, 2, 30]) for c in ctxs)
    sp.close()
    with pytest.raises(S.SnesImageError) as e:
        S.SharedPalette(ctxs, backdrop=[1, 2, 32])
    assert e.value.code == ERR_ARG
    # snesimage_shared_create still refuses backdrop members, with its present code
    with pytest.raises(S.SnesImageError) as e:
        S.SharedPalette(ctxs)
    assert e.value.code == UNSUPPORTED and "SNES_BACKDROP" in str(e.value)
    # a plain member is refused, and told where it belongs
    plain = S.OptimizedImage(imgs[0], 2, 4)
    plain.set_chunk(64)
    with pytest.raises(S.SnesImageError) as e:
        S.SharedPalette([ctxs[0], plain], backdrop=True)
    assert e.value.code == ERR_ARG and "snesimage_shared_create" in str(e.value)
    plain.close()
    # members whose regular entries differ are refused; members that differ in B alone are not (the set writes B)
    ctxs[1].backdrop = [9, 9, 9]
    sp = S.SharedPalette(ctxs, backdrop=True)
    assert np.array_equal(ctxs[1].backdrop, want)
    sp.close()
    pal = ctxs[1].palette
    pal[0] = (pal[0] + 1) % 32
    ctxs[1].palette = pal
    with pytest.raises(S.SnesImageError) as e:
        S.SharedPalette(ctxs, backdrop=True)
    assert e.value.code == ERR_STATE
    ctxs[0].step(S.METHOD_RANDOM, 2, 0, 0, 1, 0)  # a refused member is its own again
    for c in ctxs:
        c.close()
    # SNES_NES: B is a table colour; no opaque pixel: 0, 0, 0
    ctxs, sp = make_set(S, imgs, 2, 3, dict(nes=True))
    assert np.array_equal(sp.backdrop, SM.stack_backdrop(O, imgs, dict(nes=True)))
    assert any(np.array_equal(sp.backdrop, O.nes_color(k)) for k in range(56))
    close_all(sp, ctxs)
    ctxs, sp = make_set(S, [np.zeros_like(f) for f in imgs], 2, 3, {})
    assert sp.backdrop.tolist() == [0, 0, 0]
    close_all(sp, ctxs)
    assert L.snesimage_shared_get_backdrop_rgb5(None, None) == ERR_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("F,H,geom,flags", [(2, 32, (2, 3), {}), (3, 32, (2, 3), dict(perceptual=True)), (2, 56, (4, 7), {}), (3, 32, (1, 3), {})],
                         ids=["F2", "F3-perceptual", "F2-256x56-4x7", "F3-one-subpalette"])
def test_initialisers_equal_the_stacked_oracle(S, O, F, H, geom, flags):
    Cn, Sz = geom
    imgs = SM.frames(F, H)
    ctxs, sp = make_set(S, imgs, Cn, Sz, flags)
    B0 = sp.backdrop
    sm = SM.SetModel(O, imgs, Cn, Sz, flags)
    sp.initialize_tiles()
    assert np.array_equal(sp.backdrop, B0)  # B is not an initialiser's to move
    for c, t in zip(ctxs, sm.tiles_after_init):
        assert np.array_equal(c.tile_palettes, t)
    assert np.array_equal(sp.palette, sm.regular_after_init)
    sp.recalculate_palettes()
    assert np.array_equal(sp.backdrop, B0) and np.array_equal(B0, sm.B)
    assert_same_state(ctxs, sp, sm)  # tile palettes, regular entries, B, every member's map under the expanded palette
    e_g, e_m = sp.error(), sm.error()
    print("E %.17g against the model's %.17g: rel %.3e" % (e_g, e_m, rel(e_g, e_m)))
    assert rel(e_g, e_m) < REL
    close_all(sp, ctxs)
    sm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True), dict(dither=True)], ids=["rgb", "perceptual", "dither"])
def test_scores_at_the_backdrop_slot_are_the_summed_model_scores(S, O, flags):
    imgs = SM.frames(3, 32, seed=0x5EED5B10)
    ctxs, sp = start(S, O, imgs, 2, 3, flags)
    sm = SM.SetModel(O, imgs, 2, 3, flags)
    before = [(c.palette, c.backdrop, c.palette_map, c.error()) for c in ctxs]
    cand = O.random_candidates(11, 3, 16).copy()
    cand[0], cand[8] = sm.regular[1], sm.B  # equal to a regular entry; equal to the current B: the incumbent
    e_g = sp.score_candidates(2, 0, cand)
    e_m = sm.tied_candidates(cand)
    print("max rel err of 16 tied candidates over 3 members: %.3e" % float(np.max(np.abs(e_g - e_m) / e_m)))
    assert np.all(np.abs(e_g - e_m) <= REL * e_m)
    assert rel(e_g[8], sm.error()) < REL
    e_r = sp.score_candidates(1, 2, cand)  # a regular slot of the same set
    e_rm = sm.score_candidates(1, 2, cand)
    assert np.all(np.abs(e_r - e_rm) <= REL * e_rm)
    for p, i in [(0, 3), (2, 1), (3, 0)]:
        with pytest.raises(S.SnesImageError) as e:
            sp.score_candidates(p, i, cand)
        assert e.value.code == ERR_ARG
    for c, (pal, B, pmap, err) in zip(ctxs, before):  # the members are left bit-identical
        assert np.array_equal(c.palette, pal) and np.array_equal(c.backdrop, B) and np.array_equal(c.palette_map, pmap) and c.error() == err
    sp.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16)  # and the set still steps
    close_all(sp, ctxs)
    sm.close()


def check_log(log, recs, key):
    for j, r in enumerate(recs):
        e, k, rgb, changed = log[j]
        print("%s call %2d slot (%d, %d): E %.17g model %.17g rel %.2e best_k %d/%d" % (key, j, r["p"], r["i"], e, r["error"], rel(e, r["error"]), k, r["best_k"]))
        assert k == r["best_k"] and np.array_equal(rgb, r["rgb5"]) and changed == r["changed"], (key, j)
        assert rel(e, r["error"]) < REL, (key, j, e, r["error"])


def check_trajectory(S, O, name, modes=("run", 0, 1, 8)):
    flags, n, seed, state, B0 = SM.TRAJ[name]
    Cn, Sz = SM.TRAJ_GEOM
    sm, recs, final = SM.traj_run(O, name)
    imgs = SM.frames(SM.TRAJ_F, SM.TRAJ_H)
    logs = {}
    for mode in modes:
        ctxs, sp = start(S, O, imgs, Cn, Sz, flags, B0)
        if mode == "run":
            log, st = sp.run(n, seed=seed, first_step_id=0, state=state, n_random=SM.N_RANDOM)
        elif mode == 1:  # call by call: everything observable after every call
            st, log = tuple(state), []
            for j, r in enumerate(recs):
                one, st, _ = sp.run_slots(1, seed=seed, first_step_id=j, state=st, window=1, n_random=SM.N_RANDOM)
                log.append(one[0])
                assert np.array_equal(sp.palette, r["regular"]) and np.array_equal(sp.backdrop, r["B"]), (name, j)
                for c, pm in zip(ctxs, r["pmaps"]):
                    assert np.array_equal(c.palette_map, pm), (name, j)
                if r["tied"]:
                    assert np.array_equal(one[0][2], sp.backdrop)
        else:
            log, st, stats = sp.run_slots(n, seed=seed, first_step_id=0, state=state, window=mode, n_random=SM.N_RANDOM)
            assert stats["calls"] == n and (mode == 0 or stats["windows"] < n)
        check_log(log, recs, "%s/%s" % (name, mode))
        assert tuple(st) == tuple(final)
        assert_same_state(ctxs, sp, sm)
        assert [c.as_json() for c in ctxs] == [m.as_json() for m in sm.m]
        logs[mode] = [(e, k, rgb.tolist(), ch) for (e, k, rgb, ch) in log] + [sp.error()] + [c.palette_map.tobytes() for c in ctxs]
        close_all(sp, ctxs)
    first = logs[modes[0]]
    assert all(logs[m] == first for m in modes), "the windows differ from each other: they must be equal bit for bit"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb", "dither"])
def test_trajectory_two_sweeps_and_a_channel_sweep(S, O, name):
    """F = 2, 35 calls from (0, 0, 0, 3): the last random sweep, the channel sweep with the backdrop slot's three channel calls
    and the next sweep, through `run` and through `run_slots` with windows 0, 1 and 8."""
    check_trajectory(S, O, name)


@pytest.mark.gpu
def test_trajectory_nes(S, O):
    """14 NES calls; B starts from a table colour that is not the argmin."""
    check_trajectory(S, O, "nes")


@pytest.mark.gpu
def test_poisoned_storage_gives_the_same_trajectory(S, O):
    from snesimage_amd import _ffi
    _ffi.load().snesimage_debug_poison_alloc(1)
    try:
        check_trajectory(S, O, "rgb", modes=(0, 8))
    finally:
        _ffi.load().snesimage_debug_poison_alloc(0)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,n_calls", [({}, 44), (dict(dither=True), 44), (dict(nes=True), 21)], ids=["rgb", "dither", "nes"])
def test_set_of_one_steps_as_a_plain_backdrop_context(S, flags, n_calls):
    """F = 1: palette, B, map and error bit-identical after every call to snesimage_step on a backdrop context of its own
    (ks_commit_tied against k_commit + tied_spread; regular calls against the single context's)."""
    img = SM.frames(1, 32, seed=0x5EED5B20)[0]
    solo = S.OptimizedImage(img, 2, 3, backdrop=True, **flags)
    solo.set_chunk(64)
    solo.initialize_tiles()
    solo.recalculate_palettes()
    ctxs, sp = start(S, None, [img], 2, 3, flags)
    assert np.array_equal(solo.palette, sp.palette) and np.array_equal(solo.backdrop, sp.backdrop) and np.array_equal(solo.tile_palettes, ctxs[0].tile_palettes)
    nes = bool(flags.get("nes"))
    if nes:
        solo.backdrop = sp.backdrop = [19, 6, 0]
        solo.optimize()
    sched = S.schedule(2, 3, 28 + n_calls, nes, backdrop=True)[0 if nes else 28:][:n_calls]  # (not NES: the channel sweep, then random sweeps)
    moved, methods = 0, set()
    for j, (method, p, idx, ch, _) in enumerate(sched):
        b_before = solo.backdrop
        e_s, c_s = solo.step(method, p, idx, ch, 5, j, 16)
        e_g, c_g = sp.step(method, p, idx, ch, 5, j, 16)
        assert e_g == e_s and np.array_equal(c_g, c_s), (j, p, idx)
        assert np.array_equal(sp.palette, solo.palette) and np.array_equal(sp.backdrop, solo.backdrop), j
        assert np.array_equal(ctxs[0].palette_map, solo.palette_map), j
        assert sp.last_step()[1] == solo.last_step()[2], j
        if p == 2:
            methods.add(method)
            moved += int(not np.array_equal(b_before, solo.backdrop))
    assert moved, "no backdrop call moved B: the comparison shows nothing"
    assert methods == ({S.METHOD_NES} if nes else {S.METHOD_RANDOM, S.METHOD_CHANNEL})
    assert sp.error() == solo.error()
    close_all(sp, ctxs)
    solo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_tied_entries_stay_tied(S, O, flags):
    """After backdrop calls that moved B, entry S of every subpalette of every member holds B on the device, with the rows of
    the palette tables that go with it: a following regular call scores within REL of models set up from the state, and with
    every pixel mapped to the backdrop every tile of every member shows B through its own subpalette's tied entry."""
    imgs = SM.frames(2, 32, seed=0x5EED5B30)
    ctxs, sp = start(S, O, imgs, 2, 3, flags, B0=[0, 0, 0])
    moved = 0
    for j in range(4):  # random, then the three channels of the backdrop slot
        before = sp.backdrop
        sp.step(S.METHOD_RANDOM if j == 0 else S.METHOD_CHANNEL, 2, 0, max(j - 1, 0), 7, j, 16)
        moved += int(not np.array_equal(before, sp.backdrop))
    assert moved, "B did not move: nothing was spread"
    B = sp.backdrop
    sm = SM.SetModel(O, imgs, 2, 3, flags, init=False)
    sm.set_tiles([c.tile_palettes for c in ctxs])
    sm.set_state(sp.palette, B)
    assert_same_state(ctxs, sp, sm)
    assert rel(sp.error(), sm.error()) < REL
    cand = O.random_candidates(3, 9, 16)
    for p, i in [(0, 1), (1, 2)]:  # group-sparse launches on the members' palette tables as the tied commit left them
        e_g, e_m = sp.score_candidates(p, i, cand), sm.score_candidates(p, i, cand)
        assert np.all(np.abs(e_g - e_m) <= REL * e_m), (p, i)
    e, rgb = sp.step(S.METHOD_RANDOM, 1, 1, 0, 7, 20, 16)  # a regular call through the batched launches
    e_m, _, rgb_m, _, _ = sm.call(0, 1, 1, 0, 7, 20, 16)
    assert rel(e, e_m) < REL and np.array_equal(rgb, rgb_m)
    assert_same_state(ctxs, sp, sm)
    sp.close()
    want = np.array(O.snes_as_rgba(B), np.uint8)
    for c, img in zip(ctxs, imgs):  # (the members are their own again)
        assert set(np.unique(c.tile_palettes[:128])) == {0, 1}
        c.palette_map = np.full((32, 256), 3, np.uint8)
        rgba = c.as_rgba()
        assert np.all(rgba[img[..., 3] != 0] == want)
        c.close()
    sm.close()


@pytest.mark.gpu
def test_reassign_tiles_and_tile_sweep_follow_the_members_models(S, O):
    """(4, 3): both paths work on the expanded members as they stand — every call is decided on the member's own pixels."""
    import tile_model as T
    imgs = SM.frames(2, 32, seed=0x5EED5B40)
    ctxs, sp = start(S, O, imgs, 4, 3, {})
    sp.run(6, seed=2, n_random=16)
    sm = SM.SetModel(O, imgs, 4, 3, {}, init=False)
    sm.set_tiles([c.tile_palettes for c in ctxs])
    sm.set_state(sp.palette, sp.backdrop)
    moved = sum(m.o.reassign_tiles() for m in sm.m)
    assert sp.reassign_tiles() == moved
    assert_same_state(ctxs, sp, sm)
    log, stats = sp.tile_sweep(0, 24)
    accepted = 0
    for i, m in enumerate(sm.m):
        want = T.model_tile_sweep(m.o, 0, 24, 4)
        T.assert_log_matches(log[i], want)
        accepted += sum(ch for _, _, ch in want)
    assert stats["accepted"] == accepted and stats["calls"] == 48
    assert moved + accepted > 0, "no tile moved on either path: the comparison shows nothing"
    assert_same_state(ctxs, sp, sm)
    assert rel(sp.error(), sm.error()) < REL
    sp.step(S.METHOD_RANDOM, 4, 0, 0, 1, 100, 16)  # the set goes on from the new tile palettes, at the backdrop slot too
    close_all(sp, ctxs)
    sm.close()


@pytest.mark.gpu
def test_an_ordered_dither_table_goes_with_a_backdrop_set(S, O):
    import ordered_model as OM
    imgs = SM.frames(2, 32, seed=0x5EED5B50)
    table = OM.bayer(4, 32)
    ctxs, sp = make_set(S, imgs, 4, 3, {}, ordered_dither=table)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    B = sp.backdrop
    assert np.array_equal(B, SM.stack_backdrop(O, imgs, {}))  # the mean of the originals, not of the targets
    helper = M.Model(O, imgs[0], 4, 3, {}, init="zero")
    expanded = helper.expanded(sp.palette, B)
    helper.o.close()
    oms = []
    for c, img in zip(ctxs, imgs):
        om = OM.Model(O, img, 4, 4, {}, table)  # the expanded geometry, column 3 = B
        om.set_state(c.tile_palettes, expanded)
        assert np.array_equal(c.palette_map, om.palette_map)
        oms.append(om)
    cand = O.random_candidates(5, 1, 16)
    for slot, entries in [((4, 0), [3, 7, 11, 15]), ((1, 2), [6])]:
        e_m = None
        for om in oms:
            e = om.candidates(entries, cand)
            e_m = e if e_m is None else e_m + e
        e_g = sp.score_candidates(slot[0], slot[1], cand)
        print("ordered table, slot %s: max rel err %.3e" % (slot, float(np.max(np.abs(e_g - e_m) / e_m))))
        assert np.all(np.abs(e_g - e_m) <= REL * e_m), slot
    close_all(sp, ctxs)
    for om in oms:
        om.close()


@pytest.mark.gpu
def test_refusals_leave_the_set_usable(S):
    from snesimage_amd import _ffi
    L = _ffi.load()
    imgs = SM.frames(2, 32, seed=0x5EED5B60)
    ctxs, sp = start(S, None, imgs, 2, 3, {})
    before = sp.error()
    bank = np.zeros((2, 4, 4), np.int8)
    calls = [("snesimage_shared_characters", lambda: sp.characters()), ("snesimage_shared_merge_shortlist", lambda: sp.merge_shortlist(4)),
             ("snesimage_shared_score_merges", lambda: sp.score_merges([0], [1], [1], [2], [0])), ("snesimage_shared_reduce_characters", lambda: sp.reduce_characters(100)),
             ("snesimage_shared_character_fits", lambda: sp.character_fits()), ("snesimage_shared_score_refits", lambda: sp.score_refits([0])),
             ("snesimage_shared_refit_characters", lambda: sp.refit_characters()), ("snesimage_shared_as_tilemap_json", lambda: sp.as_tilemap_json()),
             ("snesimage_shared_set_ordered_dither_bank", lambda: sp.set_ordered_dither_bank(bank)), ("snesimage_shared_set_tile_levels", lambda: sp.set_tile_levels(0, np.zeros(1024, np.uint8))),
             ("snesimage_shared_score_tile_levels", lambda: sp.score_tile_levels([0], [1])), ("snesimage_shared_level_sweep", lambda: sp.level_sweep(0, 4))]
    for name, call in calls:
        with pytest.raises(S.SnesImageError) as e:
            call()
        assert e.value.code == UNSUPPORTED and name in str(e.value), name
        assert sp.error() == before, name
    # a plain set has no backdrop colour, and keeps refusing the slot
    plain = [S.OptimizedImage(f, 2, 3) for f in imgs]
    for c in plain:
        c.set_chunk(64)
    ps = S.SharedPalette(plain)
    for call in (lambda: ps.backdrop, lambda: setattr(ps, "backdrop", [1, 2, 3]), lambda: ps.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16), lambda: ps.score_candidates(2, 0, [[1, 2, 3]])):
        with pytest.raises(S.SnesImageError) as e:
            call()
        assert e.value.code == ERR_ARG
    close_all(ps, plain)
    sp.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16)  # the set still steps, at the backdrop slot and at a regular one
    sp.step(S.METHOD_RANDOM, 0, 1, 0, 1, 1, 16)
    close_all(sp, ctxs)


@pytest.mark.gpu
def test_state_and_lifetime(S):
    imgs = SM.frames(2, 32, seed=0x5EED5B70)
    ctxs, sp = start(S, None, imgs, 2, 3, {})
    sp.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16)
    ctxs[1].backdrop = [(int(ctxs[1].backdrop[0]) + 1) % 32, 2, 3]  # a member changed behind the set's back
    for call in (lambda: sp.step(S.METHOD_RANDOM, 2, 0, 0, 1, 1, 16), lambda: sp.step(S.METHOD_RANDOM, 0, 0, 0, 1, 1, 16), lambda: sp.backdrop,
                 lambda: sp.run_slots(4, seed=1), lambda: sp.error()):
        with pytest.raises(S.SnesImageError) as e:
            call()
        assert e.value.code == ERR_STATE
    with pytest.raises(S.SnesImageError) as e:
        S.SharedPalette([ctxs[0]], backdrop=True)  # still lent to the set
    assert e.value.code == ERR_STATE
    sp.close()
    # a destroyed member retires the set
    sp = S.SharedPalette(ctxs, backdrop=True)
    sp.initialize_tiles()
    ctxs[1].close()
    for call in (lambda: sp.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16), lambda: sp.error(), lambda: sp.backdrop):
        with pytest.raises(S.SnesImageError) as e:
            call()
        assert e.value.code == ERR_STATE
    sp.close()
    ctxs[0].step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16)  # the surviving member is its own again
    ctxs[0].close()


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path, O):
    """Two synthetic frames at 256 x 64, --set-backdrop --calls 40: both JSONs equal backdrop_model.model_json of the model's
    final state; --window 1 writes the same files; --resume with --calls 0 reproduces them; --set-backdrop-fixed keeps its
    colour in slot 0 of every row of every frame."""
    imgs = SM.frames(2, 64, 1, seed=0x5EED5B80)
    src = [tmp_path / ("f%d.rgba" % i) for i in range(2)]
    for p, f in zip(src, imgs):
        p.write_bytes(f.tobytes())

    def run(tag, *extra):
        outs = [str(tmp_path / ("%s%d.json" % (tag, i))) for i in range(2)]
        r = run_cli(str(src[0]), outs[0], "--share", "%s=%s" % (src[1], outs[1]), "-c", "2", "-s", "3", "--candidates", "16", "--seed", "3", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        return [open(o).read() for o in outs], r.stdout

    a, out = run("a", "--set-backdrop", "--calls", "40")
    assert "Backdrop colour of the set" in out and "Sharing one palette between 2 images" in out
    sm, recs, _ = SM.trajectory(O, imgs, 2, 3, {}, 40, 3, (0, 0, 0, 0), 16, guard=False)
    assert any(r["tied"] for r in recs)
    for i, m in enumerate(sm.m):
        assert a[i] == M.model_json(O, sm.regular, sm.B, m.o.tile_palettes, m.palette_map, imgs[i], 2, 3), i
    b16 = int(sm.B[0]) | (int(sm.B[1]) << 5) | (int(sm.B[2]) << 10)
    for js in a:
        d = json.loads(js)
        assert d["palette"][0] == d["palette"][16] == b16
    w1, _ = run("w", "--set-backdrop", "--calls", "40", "--window", "1")
    assert w1 == a
    # --resume: the main frame from the named file, the other from its own target
    for i in range(2):
        (tmp_path / ("r%d.json" % i)).write_text(a[i])
    r, out = run("r", "--set-backdrop", "--resume", str(tmp_path / "a0.json"), "--calls", "0")
    assert r == a and "Resumed the set" in out
    f, _ = run("f", "--set-backdrop-fixed", "0,0,8", "--calls", "30")
    for js in f:
        d = json.loads(js)
        assert d["palette"][0] == d["palette"][16] == 8 << 10
    assert json.loads(f[0])["palette"] == json.loads(f[1])["palette"]
    sm.close()
