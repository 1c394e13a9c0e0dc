"""The shared backdrop colour (include/snesimage_hip.h: SNES_BACKDROP): a 16th colour for every tile.

The model is the unchanged CPU oracle on the expanded geometry (tests/backdrop_model.py): OracleImage(img, C, S + 1) whose
column S holds B.  Errors agree within the project's 1e-11 relative; palettes, B, maps, JSON and scheduler states bit for bit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import backdrop_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = M.REL_ERR
UNSUPPORTED, ERR_ARG = -5, -1

# (name, flags, image variant, height)
CASES = [("rgb", {}, 0, 32), ("perceptual", dict(perceptual=True), 0, 32), ("dither", dict(dither=True), 0, 32),
         ("dither_perceptual", dict(dither=True, perceptual=True), 0, 32), ("alpha", {}, 1, 64)]
CASE_IDS = [c[0] for c in CASES]


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_backdrop_symbols():
    from snesimage_amd import _ffi
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in ("snesimage_get_backdrop_rgb5", "snesimage_set_backdrop_rgb5", "snesimage_schedule_next_backdrop"):
        assert name + "(" in text and name in bound and getattr(lib, name) is not None
    assert "SNES_BACKDROP = 8" in text
    import snesimage_amd
    assert snesimage_amd.BACKDROP == 8


@pytest.mark.parametrize("count,size,nes", [(2, 3, False), (8, 15, False), (1, 7, False), (2, 3, True)])
def test_backdrop_schedule_is_the_reference_scheduler_with_one_more_slot(S, O, count, size, nes):
    got = S.schedule(count, size, 1000, nes, backdrop=True)
    assert got == M.model_schedule(O, count, size, 1000, nes)
    slots = [(p, i) for (_, p, i, _, _) in got]
    assert (count, 0) in slots and all(p < count and i < size for (p, i) in slots if (p, i) != (count, 0))
    assert S.schedule(count, size, 50, nes) == O.schedule(count, size, 50, nes)  # the plain scheduler is untouched


def test_cli_backdrop_argument_rules(tmp_path):
    out = str(tmp_path / "o.json")
    for args, word in [(["-s", "16", "--backdrop"], "--subpalette-size <= 15"), (["-c", "16", "-s", "15", "--backdrop"], "<= 253"),
                       (["--backdrop", "--share", "synth:2=" + str(tmp_path / "p.json")], "--share"), (["--backdrop", "--devices", "0,1"], "--devices"),
                       (["--backdrop-fixed", "1,2"], "--backdrop-fixed"), (["--backdrop-fixed", "1,2,32"], "--backdrop-fixed"),
                       (["--backdrop-fixed", "1,2,3x"], "--backdrop-fixed")]:
        r = run_cli("synth:1", out, *args)
        assert r.returncode == 1 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out)  # said before anything is loaded or a device touched
    assert "--backdrop" in run_cli("--help").stderr


def test_json_rule_on_a_hand_made_map():
    """Slot 0 of every row is B; `tiles` is 0 for a transparent or a backdrop pixel, else map + 1."""
    Cn, Sz = 2, 3
    img = np.zeros((8, 256, 4), np.uint8)
    img[..., 3] = 255
    img[0, 0, 3] = 0  # transparent
    pmap = np.zeros((8, 256), np.uint8)
    pmap[0, 1], pmap[0, 2], pmap[1, 0] = 3, 2, 3  # backdrop, entry 2, backdrop
    regular = np.arange(Cn * Sz * 3, dtype=np.uint8).reshape(-1, 3) % 32
    B = np.array([31, 0, 1], np.uint8)
    d = json.loads(M.model_json(None, regular, B, np.zeros(1024, np.uint8), pmap, img, Cn, Sz))
    b16 = 31 | (0 << 5) | (1 << 10)
    assert d["palette"][0] == b16 and d["palette"][16] == b16 and len(d["palette"]) == 32
    assert d["palette"][1] == 0 | (1 << 5) | (2 << 10) and d["palette"][4:16] == [0] * 12
    assert d["tiles"][0][:3] == [0, 0, 3] and d["tiles"][0][8] == 0 and d["tiles"][0][3] == 1
    assert sorted(d) == ["palette", "tile_palettes", "tiles"] and len(d["tile_palettes"]) == 32


# ---- on the GPU ----------------------------------------------------------------------------------------------------------

def make_pair(S, O, img, Cn, Sz, flags):
    g = S.OptimizedImage(img, Cn, Sz, backdrop=True, **flags)
    B0 = g.backdrop
    g.initialize_tiles()
    g.recalculate_palettes()
    m = M.Model(O, img, Cn, Sz, flags)
    return g, m, B0


def assert_same_state(g, m):
    assert np.array_equal(g.palette, m.regular) and np.array_equal(g.backdrop, m.B)
    assert np.array_equal(g.tile_palettes, m.o.tile_palettes) and np.array_equal(g.palette_map, m.palette_map)


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags,variant,h", CASES + [("nes", dict(nes=True), 0, 32), ("frame", {}, 1, 224)], ids=CASE_IDS + ["nes", "256x224"])
def test_create_and_initialisers(S, O, name, flags, variant, h):
    img = M.image(h, 1, variant)
    Cn, Sz = (4, 7) if h == 224 else (2, 3)
    g, m, B0 = make_pair(S, O, img, Cn, Sz, flags)
    assert np.array_equal(B0, M.mean_backdrop(img, O, bool(flags.get("nes")), bool(flags.get("perceptual"))))
    assert np.array_equal(g.palette, m.regular0) and np.array_equal(g.tile_palettes, m.tiles0)  # the oracle's at (C, S)
    assert g.palette.shape == (Cn * Sz, 3) and g.palette_u16.shape == (Cn * Sz,)
    assert np.array_equal(g.palette_u16, np.array([O.snes_as_u16(c) for c in m.regular], np.uint16))
    assert_same_state(g, m)
    assert g.palette_map.max() <= Sz
    assert np.array_equal(g.as_rgba(), m.as_rgba())
    assert g.as_json() == m.as_json()
    assert rel(g.error(), m.error()) < REL_ERR
    g.close()


@pytest.mark.gpu
def test_create_limits_and_the_plain_context(S):
    img = M.image(32)
    for Cn, Sz in [(1, 16), (16, 15), (32, 7)]:
        with pytest.raises(S.SnesImageError) as e:
            S.OptimizedImage(img, Cn, Sz, backdrop=True)
        assert e.value.code == ERR_ARG
    S.OptimizedImage(img, 15, 15, backdrop=True).close()
    with S.OptimizedImage(img, 2, 3) as g:  # without the flag the slot address and the accessors are refused
        for call in (lambda: g.score_candidates(2, 0, [[1, 2, 3]]), lambda: g.step(0, 2, 0), lambda: g.backdrop):
            with pytest.raises(S.SnesImageError) as e:
                call()
            assert e.value.code == ERR_ARG
    with S.OptimizedImage(img, 2, 3, backdrop=True) as g:  # regular slots are (p < C, i < S); the backdrop slot is (C, 0) alone
        for (p, i) in [(0, 3), (2, 1), (3, 0)]:
            with pytest.raises(S.SnesImageError) as e:
                g.score_candidates(p, i, [[1, 2, 3]])
            assert e.value.code == ERR_ARG
    blank = img.copy()
    blank[..., 3] = 0
    with S.OptimizedImage(blank, 2, 3, backdrop=True) as g:
        assert g.backdrop.tolist() == [0, 0, 0]


def candidate_list(O, m, n, seed):
    cand = O.random_candidates(seed, 77, n).copy()
    cand[0] = m.regular[1]  # equal to a regular entry: the tie goes to the regular entry
    if n > 1:
        cand[n // 2] = m.B  # equal to the current B
    return cand


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags,variant,h", CASES, ids=CASE_IDS)
def test_score_candidates_at_the_backdrop_slot(S, O, name, flags, variant, h):
    from hipmem import DeviceArray
    img = M.image(h, 2, variant)
    Cn, Sz = 2, 3
    g, m, _ = make_pair(S, O, img, Cn, Sz, flags)
    inc = m.error()
    # maps and errors, bit for bit and within the tolerance, on a list a model can afford
    cand = candidate_list(O, m, 64, 5)
    d_c, d_e, d_m = DeviceArray.from_numpy(cand), DeviceArray(64, np.float64, fill=0), DeviceArray((64, h, 256), np.uint8, fill=255)
    g.score_candidates_device(Cn, 0, d_c.ptr, 64, d_e.ptr, d_m.ptr)
    g.sync()
    e_model, maps_model = m.tied_candidates(cand, want_maps=True)
    e_dev, maps_dev = d_e.numpy(), d_m.numpy()
    print("max rel err of 64 tied candidates: %.3e" % float(np.max(np.abs(e_dev - e_model) / e_model)))
    assert np.array_equal(maps_dev, maps_model)
    assert np.all(np.abs(e_dev - e_model) <= REL_ERR * e_model)
    assert rel(e_dev[32], inc) < REL_ERR  # the current B: the incumbent
    d_r = DeviceArray((64, h, 256), np.uint8, fill=255)
    g.remap_candidates_device(Cn, 0, d_c.ptr, 64, d_r.ptr)
    g.sync()
    assert np.array_equal(d_r.numpy(), maps_model)
    # list lengths across the launch groups: every candidate equals what a list of its own gives
    g.set_chunk(512)
    for n in (1, 64, 1025, 4096):
        cand_n = candidate_list(O, m, n, 6)
        e_n = g.score_candidates(Cn, 0, cand_n)
        probe = sorted({0, n // 2, n - 1, min(n - 1, 511), min(n - 1, 512), min(n - 1, 1024)})
        e_probe = m.tied_candidates(cand_n[probe])
        print("n = %d: max rel err at %d probes %.3e" % (n, len(probe), float(np.max(np.abs(e_n[probe] - e_probe) / e_probe))))
        assert np.all(np.abs(e_n[probe] - e_probe) <= REL_ERR * e_probe)
        if n >= 64:  # every other candidate against the same colour scored in the 64-list's run of the same kernels
            again = g.score_candidates(Cn, 0, cand_n[:64])
            assert np.array_equal(again, e_n[:64])
    # a regular slot of the same context
    cand = O.random_candidates(9, 1, 16)
    e_reg = g.score_candidates(1, 2, cand)
    e_mod = m.o.score_candidates(1, 2, cand)
    assert np.all(np.abs(e_reg - e_mod) <= REL_ERR * e_mod)
    assert_same_state(g, m)  # scoring leaves the context as it was
    g.close()


# seeds for which the model alone passes the guard and accepts a backdrop call (found on the CPU; re-checked by the test)
TRAJ = {"rgb": 2, "perceptual": 2, "dither": 4, "dither_perceptual": 1, "alpha": 2}
_models = {}


def model_run(O, key, img, Cn, Sz, flags, n, seed, state, B0):
    if key not in _models:
        _models[key] = M.trajectory(O, img, Cn, Sz, flags, n, seed, state, B0=B0)
    return _models[key]


def check_trajectory(S, O, key, img, Cn, Sz, flags, n, seed, state, windows=(0, 1, 8), B0=None):
    m, recs, final = model_run(O, key, img, Cn, Sz, flags, n, seed, state, B0)
    assert any(r["p"] == Cn and r["changed"] for r in recs), "no backdrop call was accepted: choose another seed"
    for window in windows:
        g = S.OptimizedImage(img, Cn, Sz, backdrop=True, **flags)
        g.initialize_tiles()
        g.recalculate_palettes()
        if B0 is not None:
            g.backdrop = B0
            g.optimize()
        if window == 1:  # call by call: everything observable after every call
            st = tuple(state)
            for j, r in enumerate(recs):
                log, st, _ = g.run_slots(1, seed=seed, first_step_id=j, state=st, window=1)
                assert np.array_equal(g.palette, r["regular"]) and np.array_equal(g.backdrop, r["B"]) and np.array_equal(g.palette_map, r["pmap"]), (key, j)
                assert np.array_equal(log[0][2], r["rgb5"]) and log[0][3] == r["changed"] and rel(log[0][0], r["error"]) < REL_ERR, (key, j)
                if r["p"] == Cn:
                    assert np.array_equal(log[0][2], g.backdrop)
        else:
            log, st, stats = g.run_slots(n, seed=seed, first_step_id=0, state=state, window=window)
            assert stats["calls"] == n
            for j, r in enumerate(recs):
                assert np.array_equal(log[j][2], r["rgb5"]) and log[j][3] == r["changed"], (key, window, j)
                assert rel(log[j][0], r["error"]) < REL_ERR, (key, window, j, log[j][0], r["error"])
        assert st == tuple(final)
        assert_same_state(g, m)
        assert g.as_json() == m.as_json()
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags,variant,h", CASES, ids=CASE_IDS)
def test_trajectory_two_sweeps_and_a_channel_sweep(S, O, name, flags, variant, h):
    """(2,3): the last random sweep of a round, the channel sweep (three calls per entry, the backdrop slot included) and
    the next random sweep — 7 + 21 + 7 calls — through snesimage_run_slots with window 0, 1 and 8."""
    check_trajectory(S, O, name, M.image(h, 0, variant), 2, 3, flags, 35, TRAJ[name], (0, 0, 0, 3))


@pytest.mark.gpu
def test_trajectory_one_sweep_at_4x7(S, O):
    check_trajectory(S, O, "4x7", M.image(32), 4, 7, {}, 29, 2, (0, 0, 0, 0))


@pytest.mark.gpu
def test_trajectory_nes(S, O):
    # (the NES method takes the table's argmin whatever the seed: B starts from a table colour that is not it)
    check_trajectory(S, O, "nes", M.image(32), 2, 3, dict(nes=True), 14, 1, (0, 0, 0, 0), B0=O.nes_color(1))


@pytest.mark.gpu
def test_poisoned_storage_gives_the_same_trajectory(S, O):
    """The tied-slot pack writes every word it later reads: with fresh storage full of NaN bytes nothing changes."""
    from snesimage_amd import _ffi
    _ffi.load().snesimage_debug_poison_alloc(1)
    try:
        check_trajectory(S, O, "rgb", M.image(32), 2, 3, {}, 35, TRAJ["rgb"], (0, 0, 0, 3), windows=(0,))
        check_trajectory(S, O, "dither", M.image(32), 2, 3, dict(dither=True), 35, TRAJ["dither"], (0, 0, 0, 3), windows=(8,))
    finally:
        _ffi.load().snesimage_debug_poison_alloc(0)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(dither=True)], ids=["rgb", "dither"])
def test_split_phase_step_at_the_backdrop_slot(S, flags):
    """step_begin / min-reduce / step_commit over two shards on one device == step()."""
    from hipmem import DeviceArray
    img = M.image(32, 3)
    Cn, Sz = 2, 3
    ref = S.OptimizedImage(img, Cn, Sz, backdrop=True, **flags)
    ref.initialize_tiles()
    ref.recalculate_palettes()
    shards = []
    for _ in range(2):
        s = S.OptimizedImage(img, Cn, Sz, backdrop=True, **flags)
        s.tile_palettes, s.palette, s.backdrop = ref.tile_palettes, ref.palette, ref.backdrop
        s.optimize()
        shards.append(s)
    changed = 0
    for i, (method, ch) in enumerate([(S.METHOD_RANDOM, 0), (S.METHOD_CHANNEL, 1), (S.METHOD_RANDOM, 0)]):
        n = 40 if method == S.METHOD_RANDOM else 32
        b_before = ref.backdrop
        e_ref, b_ref = ref.step(method, Cn, 0, ch, 4, i, 40)
        changed += int(not np.array_equal(b_before, b_ref))
        bufs = [DeviceArray(n, np.float64, fill=0) for _ in range(2)]
        for r, s in enumerate(shards):
            s.step_begin(method, Cn, 0, ch, 4, i, 40, r, 2, bufs[r].ptr)
            s.sync()
        red = DeviceArray.from_numpy(np.minimum(bufs[0].numpy(), bufs[1].numpy()))
        for s in shards:
            s.step_commit(red.ptr)
            e, b, _ = s.last_step()
            assert e == e_ref and np.array_equal(b, b_ref) and np.array_equal(s.backdrop, ref.backdrop)
            assert np.array_equal(s.palette, ref.palette) and np.array_equal(s.palette_map, ref.palette_map)
    assert changed, "no split-phase step moved B: the comparison shows nothing"
    for s in shards + [ref]:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_reassign_tiles_on_the_expanded_context(S, O, flags):
    img = M.image(64, 4)
    g, m, _ = make_pair(S, O, img, 4, 7, flags)
    assert g.reassign_tiles() == m.o.reassign_tiles()
    assert_same_state(g, m)
    assert rel(g.error(), m.error()) < REL_ERR
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(dither=True)], ids=["rgb", "dither"])
def test_tile_sweep_on_the_expanded_context(S, O, flags):
    import tile_model as T
    img = M.image(32, 5)
    g, m, _ = make_pair(S, O, img, 4, 3, flags)
    want = T.model_tile_sweep(m.o, 0, 24, 4)
    log, stats = g.tile_sweep(0, 24)
    T.assert_log_matches(log, want)
    assert_same_state(g, m)
    errs = g.score_tile_moves([3, 5], [1, 2])
    for (t, s), e in zip([(3, 1), (5, 2)], errs):
        assert rel(e, T.model_candidate(m.o, t, s)[0]) < REL_ERR
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(dither=True)], ids=["rgb", "dither"])
def test_set_backdrop_and_palette_map(S, O, flags):
    img = M.image(32, 6, 1)
    Cn, Sz = 2, 3
    g, m, _ = make_pair(S, O, img, Cn, Sz, flags)
    g.backdrop = [3, 30, 7]
    g.optimize()
    m.set_state(m.regular, [3, 30, 7])
    assert_same_state(g, m)
    assert rel(g.error(), m.error()) < REL_ERR and np.array_equal(g.as_rgba(), m.as_rgba())
    with pytest.raises(S.SnesImageError):
        g.backdrop = [3, 32, 7]
    pm = np.full((32, 256), Sz, np.uint8)  # every pixel the backdrop
    g.palette_map = pm
    m.o.palette_map = pm
    assert rel(g.error(), m.error()) < REL_ERR
    rgba = g.as_rgba()
    assert np.array_equal(rgba, m.as_rgba())
    opaque = img[..., 3] != 0
    assert np.all(rgba[opaque] == O.snes_as_rgba([3, 30, 7])) and np.all(rgba[~opaque] == 0)
    pm[0, 0] = Sz + 1
    with pytest.raises(S.SnesImageError) as e:
        g.palette_map = pm
    assert e.value.code == ERR_ARG
    g.close()


@pytest.mark.gpu
def test_batches_groups_sets_and_split_windows_refuse_a_backdrop_context(S):
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = M.image(32)
    g = S.OptimizedImage(img, 2, 3, backdrop=True)
    g.initialize_tiles()
    g.recalculate_palettes()
    before = g.error()
    arr = (C.c_void_p * 1)(g._c)
    for fn in (L.snesimage_batch_create, L.snesimage_group_create, L.snesimage_shared_create):
        out = C.c_void_p()
        assert fn(arr, 1, C.byref(out)) == UNSUPPORTED and not out.value
        assert b"SNES_BACKDROP" in L.snesimage_last_error()
    with pytest.raises(S.SnesImageError) as e:
        g.slots_begin(4, 1, 0, (0, 0, 0, 0))
    assert e.value.code == UNSUPPORTED and "SNES_BACKDROP" in str(e.value)
    with pytest.raises(S.SnesImageError) as e:
        g.slots_commit()
    assert e.value.code == UNSUPPORTED
    assert g.error() == before  # still usable
    g.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0)
    g.close()


@pytest.mark.gpu
def test_cli_round_trip(tmp_path, S):
    """--backdrop --calls N, then --resume with --calls 0: the same JSON; `tiles` is 0 exactly where the map says backdrop or
    the pixel is transparent; --backdrop-fixed keeps the colour it was given."""
    img = M.image(64, 7, 1)
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    a, b, f = str(tmp_path / "a.json"), str(tmp_path / "b.json"), str(tmp_path / "f.json")
    r = run_cli(str(src), a, "-c", "2", "-s", "3", "--backdrop", "--calls", "40", "--seed", "2", "--preview", str(tmp_path / "p.png"))
    assert r.returncode == 0, r.stdout + r.stderr
    r = run_cli(str(src), b, "-c", "2", "-s", "3", "--backdrop", "--resume", a, "--calls", "0")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(a).read() == open(b).read()
    d = json.loads(open(a).read())
    # the same run through the library
    g = S.OptimizedImage(img, 2, 3, backdrop=True)
    g.initialize_tiles()
    g.recalculate_palettes()
    g.run_slots(40, seed=2)
    assert g.as_json() == open(a).read()
    pm, B = g.palette_map, g.backdrop
    assert d["palette"][0] == d["palette"][16] == int(B[0]) | (int(B[1]) << 5) | (int(B[2]) << 10)
    zero = np.zeros((64, 256), bool)
    for t, vals in enumerate(d["tiles"]):
        ty, tx = divmod(t, 32)
        zero[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = np.array(vals).reshape(8, 8) == 0
    assert np.array_equal(zero, (pm == 3) | (img[..., 3] == 0)) and (pm == 3).any()
    g.close()
    r = run_cli(str(src), f, "-c", "2", "-s", "3", "--backdrop-fixed", "1,2,30", "--calls", "30")
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(open(f).read())["palette"][0] == 1 | (2 << 5) | (30 << 10)
