"""Guided calls of a shared-palette set (include/snesimage_hip.h: snesimage_shared_guided_costs, _candidates, _step, _sweep;
SharedPalette.guided_*; cli --set-guided; DESIGN 5f').

The model is tests/set_guided_model.py: the set's cost table is the sum of guided_model.costs over the members, errors are the
members' summed in member order.  Costs (all 32,768) and shortlists agree bit for bit, as do palettes, tile_palettes, every
member's map and the decisions; errors within the project's 1e-11 relative.  The trajectories' inputs are
set_guided_model.CASES; tests/test_set_guided_model.py shows on the CPU that each holds the gap premise and accepts and rejects."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adversarial_images as AI
import guided_model as GM
import ordered_model as OM
import set_backdrop_model as SB
import set_guided_model as SGM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = 1e-11
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
NAMES = ("snesimage_shared_guided_costs", "snesimage_shared_guided_candidates", "snesimage_shared_guided_step_async", "snesimage_shared_guided_step",
         "snesimage_shared_guided_sweep")


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def close(a, b):
    return abs(a - b) <= REL_ERR * abs(b)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_set_guided_symbols():
    from snesimage_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    costs, rgb5 = (C.c_uint64 * 32768)(), (C.c_uint8 * 48)()
    assert lib.snesimage_shared_guided_costs(None, 0, 0, costs) == ERR_ARG
    assert lib.snesimage_shared_guided_candidates(None, 0, 0, 16, rgb5, None) == ERR_ARG
    assert lib.snesimage_shared_guided_step(None, 0, 0, 16, None, None) == ERR_ARG
    assert lib.snesimage_shared_guided_step_async(None, 0, 0, 16) == ERR_ARG
    assert lib.snesimage_shared_guided_sweep(None, 16, None, None) == ERR_ARG
    import snesimage_amd
    for method in ("guided_costs", "guided_candidates", "guided_step", "guided_step_async", "guided_sweep"):
        assert callable(getattr(snesimage_amd.SharedPalette, method))


def test_cli_argument_rules(tmp_path):
    """Everything is said while parsing: the sources do not exist, so a refusal behind a file or device access would exit 1."""
    missing, out, other = str(tmp_path / "none.png"), str(tmp_path / "o.json"), str(tmp_path / "s.json")
    share = ["--share", "%s=%s" % (missing, other)]
    for args, word in [(["--set-guided", "1"], "--share"), (["--set-guided", "1", "--set-guided-shortlist", "8"], "--share"),
                       (share + ["--set-guided", "1", "--devices", "0"], "--devices"), (share + ["--set-guided", "1", "--nes"], "--nes"),
                       (share + ["--nes", "--set-guided", "2", "--set-guided-shortlist", "8"], "--nes"),
                       (share + ["--set-guided", "0"], "--set-guided"), (share + ["--set-guided", "x"], "--set-guided"), (share + ["--set-guided", "-1"], "--set-guided"),
                       (share + ["--set-guided", ""], "--set-guided"), (share + ["--set-guided", "1", "--set-guided-shortlist", "0"], "--set-guided-shortlist"),
                       (share + ["--set-guided", "1", "--set-guided-shortlist", "65"], "--set-guided-shortlist"),
                       (share + ["--set-guided", "1", "--set-guided-shortlist", "k"], "--set-guided-shortlist"), (share + ["--set-guided-shortlist", "8"], "--set-guided"),
                       (["--set-guided-shortlist", "8"], "--set-guided"), (share + ["--guided", "1"], "--share")]:  # (the last: --guided beside --share stays refused)
        r = run_cli(missing, out, *args)
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out) and not os.path.exists(other)
    h = run_cli("--help").stderr
    assert "--set-guided <G>" in h and "--set-guided-shortlist <K>" in h and h.count("default: 16: a choice, not a measurement") >= 3


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

def make_set(S, imgs, Cn, Sz, flags=None, tiles=None, pal=None, B=None, table=None, chunk=64):
    """A set whose members hold the given tile palettes and regular entries (None: as created); B: a backdrop set with that B."""
    ctxs = [S.OptimizedImage(f, Cn, Sz, backdrop=B is not None, **(flags or {})) for f in imgs]
    for j, c in enumerate(ctxs):
        c.set_chunk(chunk)
        if tiles is not None:
            c.tile_palettes = tiles[j]
        if pal is not None:
            c.palette = pal
        c.optimize()
    return ctxs, S.SharedPalette(ctxs, ordered_dither=table, backdrop=None if B is None else B)


def model_set(S, m, table=None):
    """The library's set in the model's state."""
    return make_set(S, m.imgs, m.C, m.S, m.flags, m.tiles, m.palette, m.B, table)


def close_all(sp, ctxs, m=None):
    sp.close()
    for c in ctxs:
        c.close()
    if m is not None:
        m.close()


def assert_costs_equal(got, want, what):
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.shape == want.shape == (32768,)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of 32768 costs differ, first at u = %d: %d against %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def state_of(sp, ctxs):
    return (sp.error(), [c.palette.tobytes() for c in ctxs], [c.tile_palettes.tobytes() for c in ctxs], [c.palette_map.tobytes() for c in ctxs])


def hand_tiles(F, per, pattern):
    """tile_palettes per member from pattern(f, t)."""
    out = []
    for f in range(F):
        t = np.zeros(1024, np.uint8)
        t[:per] = [pattern(f, k) for k in range(per)]
        out.append(t)
    return out


@pytest.mark.gpu
def test_costs_one_tile_row_per_member_and_a_ragged_population(S, O):
    """F = 3 frames of 256 x 8 at 2 x 3; subpalette 1 holds 5 + 20 + 32 = 57 tiles: no multiple of a slice's 16."""
    m = SGM.SetModel(O, SB.frames(3, 8), 2, 3)
    m.set_tiles(hand_tiles(3, 32, lambda f, k: int(k < (5, 20, 32)[f])))
    assert sum(int((t[:32] == 1).sum()) for t in m.tiles) == 57
    ctxs, sp = model_set(S, m)
    before = state_of(sp, ctxs)
    for p, i in ((1, 0), (1, 2), (0, 1)):
        assert_costs_equal(sp.guided_costs(p, i), m.costs(p, i), "3 x (256 x 8), slot (%d, %d)" % (p, i))
    assert state_of(sp, ctxs) == before, "guided_costs changed the state"
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_costs_every_pixel_over_several_whole_slices(S, O):
    m = SGM.SetModel(O, SB.frames(2, 16), 1, 3)  # 2 x 64 tiles in one subpalette: 8,192 pixels, eight slices
    ctxs, sp = model_set(S, m)
    for i in (0, 2):
        assert_costs_equal(sp.guided_costs(0, i), m.costs(0, i), "2 x (256 x 16) at 1 x 3, slot (0, %d)" % i)
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_a_set_of_one_member_equals_that_context(S):
    img = SB.frames(1, 16)[0]
    g = S.OptimizedImage(img, 2, 3)
    g.set_chunk(64)
    g.initialize_tiles()
    g.recalculate_palettes()
    own = [(g.guided_costs(p, i), g.guided_candidates(p, i, 16)) for p, i in ((0, 0), (1, 2))]
    sp = S.SharedPalette([g])
    for (p, i), (cost, (rgb5, c)) in zip(((0, 0), (1, 2)), own):
        assert_costs_equal(sp.guided_costs(p, i), cost, "a set of one, slot (%d, %d)" % (p, i))
        r2, c2 = sp.guided_candidates(p, i, 16)
        assert np.array_equal(r2, rgb5) and np.array_equal(c2, c)
    close_all(sp, [g])


@pytest.mark.gpu
def test_costs_of_a_subpalette_used_by_one_member_or_by_none(S, O):
    m = SGM.SetModel(O, SB.frames(2, 16), 4, 7)
    m.set_tiles(hand_tiles(2, 64, lambda f, k: (k % 3) if f == 0 else (k % 2)))  # subpalette 2: member 0 only; subpalette 3: nobody
    ctxs, sp = model_set(S, m)
    want = m.costs(2, 4)
    assert np.array_equal(want, GM.costs(m.imgs[0], m.tiles[0], m.internal, 4, 7, 2, 4)) and want.any()
    assert_costs_equal(sp.guided_costs(2, 4), want, "a subpalette of member 0 only")
    assert_costs_equal(sp.guided_costs(0, 6), m.costs(0, 6), "a subpalette of both members")
    assert not sp.guided_costs(3, 2).any() and not m.costs(3, 2).any()
    rgb5, cost = sp.guided_candidates(3, 2, 8)  # every cost ties at 0: the lowest colours, the current one left out
    cur = int(GM.pack_u(m.internal[3 * 7 + 2]))
    assert GM.pack_u(rgb5).tolist() == [u for u in range(10) if u != cur][:8] and not cost.any()
    before = state_of(sp, ctxs)
    e, best = sp.guided_step(3, 2, 8)  # no pixel reads the entry: every candidate ties with the incumbent and is rejected
    assert sp.last_step()[1] == -1 and sp.last_step()[3] == 0 and e == before[0] and np.array_equal(best, m.internal[3 * 7 + 2])
    assert state_of(sp, ctxs) == before
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_costs_of_a_one_entry_subpalette_have_no_floor(S):
    imgs = SB.frames(2, 8)
    tiles = hand_tiles(2, 32, lambda f, k: (k + f) % 2)
    pal = np.array([[10, 12, 7], [3, 20, 25]], np.uint8)
    ctxs, sp = make_set(S, imgs, 2, 1, None, tiles, pal)
    want = SGM.set_costs(imgs, tiles, pal, 2, 1, 1, 0)
    px = np.concatenate([f[:, [x for k in range(32) if t[k] == 1 for x in range(8 * k, 8 * k + 8)], :3].reshape(-1, 3) for f, t in zip(imgs, tiles)])
    assert int(want[0]) == int(GM.red_mean_key(px, [0, 0, 0]).sum())  # no floor: the plain sum of keys
    assert_costs_equal(sp.guided_costs(1, 0), want, "2 x 1")
    close_all(sp, ctxs)


@pytest.mark.gpu
def test_costs_with_transparent_pixels_in_one_member(S, O):
    imgs = SB.frames(2, 16)
    imgs[1][3:8, 10:22, 3] = 0      # parts of tiles 1 and 2
    imgs[1][8:16, 64:96, 3] = 0     # tiles 40 .. 43 whole
    imgs[1][0:8, 248:256, 3] = 0    # tile 31 whole
    m = SGM.SetModel(O, imgs, 2, 3)
    ctxs, sp = model_set(S, m)
    for p, i in ((0, 1), (1, 2)):
        assert_costs_equal(sp.guided_costs(p, i), m.costs(p, i), "alpha in member 1, slot (%d, %d)" % (p, i))
    opaque = [f.copy() for f in imgs]
    opaque[1][..., 3] = 255
    assert (SGM.set_costs(opaque, m.tiles, m.internal, 2, 3, 0, 1) != m.costs(0, 1)).any(), "the holes change no cost: the case shows nothing"
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_costs_read_the_members_ordered_dither_targets(S, O):
    table = OM.bayer(4, 64)
    m = SGM.SetModel(O, SB.frames(2, 16), 2, 3)
    ctxs, sp = model_set(S, m, table)
    Ts = [OM.target_image(f, table) for f in m.imgs]
    for c, T, f in zip(ctxs, Ts, m.imgs):
        assert np.array_equal(c.target_rgba(), T) and not np.array_equal(T, f)
    want = m.costs(1, 0, Ts)
    assert_costs_equal(sp.guided_costs(1, 0), want, "Bayer 4 x 4, slot (1, 0)")
    assert (m.costs(1, 0) != want).any(), "the table changes no cost: the case shows nothing"
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_costs_on_a_backdrop_set_regular_and_tied(S, O):
    imgs = SB.frames(2, 16)
    m = SGM.SetModel(O, imgs, 2, 3, {}, SB.stack_backdrop(O, imgs, {}))  # the stack's mean: a B that is some pixels' nearest entry
    ctxs, sp = model_set(S, m)
    assert np.array_equal(sp.backdrop, m.B) and np.array_equal(sp.palette, m.palette)
    assert_costs_equal(sp.guided_costs(1, 1), m.costs(1, 1), "backdrop set, regular slot (1, 1)")
    assert_costs_equal(sp.guided_costs(2, 0), m.costs(2, 0), "backdrop set, the tied slot")
    without_b = SGM.set_costs(m.imgs, m.tiles, m.palette, 2, 3, 1, 1)  # the floor of a regular slot counts B as one of the other entries
    assert (without_b != m.costs(1, 1)).any()
    rgb5, c = sp.guided_candidates(2, 0, 16)
    want_rgb5, want_c = m.candidates(2, 0, 16)
    assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c) and not any(np.array_equal(x, m.B) for x in rgb5)
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_candidates_order_costs_and_lengths(S, O):
    m = SGM.SetModel(O, SB.frames(2, 16), 2, 3)
    ctxs, sp = model_set(S, m)
    before = state_of(sp, ctxs)
    cost = m.costs(1, 2)
    cur = m.internal[1 * 3 + 2]
    for k, n in ((0, 16), (1, 1), (16, 16), (64, 64)):
        rgb5, c = sp.guided_candidates(1, 2, k)
        want_rgb5, want_c = GM.shortlist(cost, cur, k)
        assert rgb5.shape == (n, 3) and np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c), k
        assert not any(np.array_equal(x, cur) for x in rgb5)
        assert np.array_equal(c, cost[GM.pack_u(rgb5)]) and (np.diff(c.astype(np.int64)) >= 0).all()
    assert state_of(sp, ctxs) == before, "guided_candidates changed the state"
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_candidates_tie_rule_on_flat_frames(S):
    """guided_model's flat case on two equal frames: every cost of slot (0, 2) is 0 and the order is the colours' own, the
    slot's current colour, u = 3, left out; slot (1, 0) sees 2 x 512 equal grey pixels: 24 colours lie nearer than the other
    entry, all others tie at 1024 * floor and come in ascending u."""
    imgs = [AI.two_tone(8), AI.two_tone(8)]
    tp = np.zeros(1024, np.uint8)
    tp[16:24] = 1
    pal = np.array([[0, 0, 0], [31, 31, 31], [3, 0, 0], [2, 2, 2], [16, 17, 16], [31, 0, 0]], np.uint8)
    ctxs, sp = make_set(S, imgs, 2, 3, None, [tp, tp], pal)
    want = SGM.set_costs(imgs, [tp, tp], pal, 2, 3, 0, 2)
    assert not want.any()
    assert_costs_equal(sp.guided_costs(0, 2), want, "flat frames, slot (0, 2)")
    rgb5, c = sp.guided_candidates(0, 2, 64)
    assert GM.pack_u(rgb5).tolist() == [u for u in range(65) if u != 3] and not c.any()
    want = SGM.set_costs(imgs, [tp, tp], pal, 2, 3, 1, 0)
    floor = int(GM.red_mean_key([128, 128, 128], [132, 140, 132]))
    assert int(want.max()) == 1024 * floor and (want == 1024 * floor).sum() == 32768 - 24
    assert_costs_equal(sp.guided_costs(1, 0), want, "flat frames, slot (1, 0)")
    rgb5, c = sp.guided_candidates(1, 0, 64)
    want_rgb5, want_c = GM.shortlist(want, pal[3], 64)
    assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c)
    assert (c[:24] < 1024 * floor).all() and (c[24:] == 1024 * floor).all() and GM.pack_u(rgb5[24:]).tolist() == list(range(40))
    close_all(sp, ctxs)


# ---- trajectories ---------------------------------------------------------------------------------------------------------

def case_set(S, r):
    return make_set(S, r["imgs"], r["C"], r["S"], r["flags"], r["tiles"], r["pal0"], r["B0"])


def assert_state(sp, ctxs, rec, what):
    assert np.array_equal(sp.palette, rec["palette"]), what
    if rec["B"] is not None:
        assert np.array_equal(sp.backdrop, rec["B"]), what
    for c, pm in zip(ctxs, rec["pmaps"]):
        assert np.array_equal(c.palette, rec["palette"]) and np.array_equal(c.palette_map, pm), what
    assert close(sp.error(), rec["error"]), (what, sp.error(), rec["error"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_guided_steps_follow_the_model(S, O, name):
    r = SGM.trajectory(O, name)
    ctxs, sp = case_set(S, r)
    assert all(np.array_equal(c.palette_map, pm) and np.array_equal(c.tile_palettes, t) for c, pm, t in zip(ctxs, r["maps0"], r["tiles"])) and close(sp.error(), r["err0"])
    for j, rec in enumerate(r["recs"]):
        what = "%s call %d slot (%d, %d)" % (name, j, rec["p"], rec["i"])
        rgb5, cost = sp.guided_candidates(rec["p"], rec["i"], r["K"])
        assert np.array_equal(rgb5, rec["cand"]) and np.array_equal(cost, rec["costs"]), what
        err, best = sp.guided_step(rec["p"], rec["i"], r["K"])
        e2, k2, b2, ch2 = sp.last_step()
        print("%s: best_k %d (model %d), E %.9f (model %.9f)" % (what, k2, rec["best_k"], err, rec["error"]))
        assert k2 == rec["best_k"] and ch2 == rec["changed"] and np.array_equal(best, rec["rgb5"]) and np.array_equal(b2, rec["rgb5"]) and e2 == err and close(err, rec["error"]), what
        assert_state(sp, ctxs, rec, what)
    close_all(sp, ctxs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_guided_sweep_equals_the_calls_one_by_one_and_the_model(S, O, name):
    r = SGM.trajectory(O, name)
    (ctxs, sp), (tctxs, twin) = case_set(S, r), case_set(S, r)
    log, stats = sp.guided_sweep(r["K"])
    slots = [(p, i) for p in range(r["C"]) for i in range(r["S"])] + ([(r["C"], 0)] if r["backdrop"] else [])
    assert len(log) == len(slots) and stats["calls"] == stats["windows"] == len(slots) and stats["scored"] == stats["useful"] == len(slots) * r["K"] and stats["voided"] == 0
    for j, (p, i) in enumerate(slots):
        twin.guided_step(p, i, r["K"])
        e, k, b, ch = twin.last_step()
        assert log[j][0] == e and log[j][1] == k and np.array_equal(log[j][2], b) and log[j][3] == ch == int(k >= 0), (name, j, log[j], (e, k, b, ch))
    assert stats["accepted"] == sum(x[3] for x in log) and 0 < stats["accepted"]
    assert state_of(sp, ctxs) == state_of(twin, tctxs)
    la, lb = sp.last_step(), twin.last_step()
    assert la[0] == lb[0] and la[1] == lb[1] and np.array_equal(la[2], lb[2]) and la[3] == lb[3]
    n = min(len(slots), len(r["recs"]))
    for j, rec in enumerate(r["recs"][:n]):
        assert (rec["p"], rec["i"]) == slots[j] and log[j][1] == rec["best_k"] and np.array_equal(log[j][2], rec["rgb5"]) and close(log[j][0], rec["error"]), (name, j)
    if n == len(slots):
        assert_state(sp, ctxs, r["recs"][n - 1], name + " after the sweep")
    close_all(sp, ctxs)
    close_all(twin, tctxs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain-f2-2x3", "dither-f2-2x3", "backdrop-f2-2x3"])
def test_the_flags_a_guided_sweep_leaves_serve_the_slot_windows(S, O, name):
    """Two equal sets: a guided sweep, then about ten scheduled calls through the windows (window = 0) on one and call by call
    (window = 1) on the other, end in the same state, record for record."""
    r = SGM.trajectory(O, name)
    out = []
    for window in (0, 1):
        ctxs, sp = case_set(S, r)
        sweep = sp.guided_sweep(r["K"])[0]
        log, st, stats = sp.run_slots(10, seed=7, first_step_id=3, state=(1, 1, 0, 3), window=window, n_random=16)  # the last random calls of a sweep, then channel calls
        out.append(([(x[0], x[1], x[2].tolist(), x[3]) for x in sweep + log], st, stats["accepted"], state_of(sp, ctxs), sp.last_step()[:2]))
        close_all(sp, ctxs)
    assert out[0] == out[1]
    assert out[0][2] > 0, "no scheduled call accepted: the comparison shows little"


# ---- refusals -------------------------------------------------------------------------------------------------------------

def refused(S, fn, code):
    with pytest.raises(S.SnesImageError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def all_refused(S, sp, code):
    refused(S, lambda: sp.guided_costs(0, 0), code)
    refused(S, lambda: sp.guided_candidates(0, 0), code)
    refused(S, lambda: sp.guided_step(0, 0), code)
    refused(S, lambda: sp.guided_step_async(0, 0), code)
    refused(S, lambda: sp.guided_sweep(), code)


@pytest.mark.gpu
def test_refusals_leave_the_set_usable(S, O):
    from snesimage_amd import _ffi
    L = _ffi.load()
    r = SGM.trajectory(O, "plain-f2-2x3")
    ctxs, sp = case_set(S, r)
    before = state_of(sp, ctxs)
    # a failed workspace allocation: all or nothing
    for nth in (0, 2):
        L.snesimage_debug_fail_alloc(nth)
        try:
            assert "workspace" in refused(S, lambda: sp.guided_costs(0, 0), ERR_HIP)
        finally:
            L.snesimage_debug_fail_alloc(-1)
    # arguments
    for fn in (lambda: sp.guided_candidates(0, 0, 65), lambda: sp.guided_step(0, 0, 65), lambda: sp.guided_sweep(65), lambda: sp.guided_step_async(1, 1, 65),
               lambda: sp.guided_costs(0, 3), lambda: sp.guided_costs(2, 1), lambda: sp.guided_step(2, 0), lambda: sp.guided_candidates(2, 0, 4), lambda: sp.guided_step_async(2, 0)):
        refused(S, fn, ERR_ARG)  # k = 65, a slot out of range, the tied slot on a plain set
    refused(S, lambda: sp.step(S.METHOD_RANDOM, 2, 0, 0, 1, 0, 16), ERR_ARG)  # (as snesimage_shared_step refuses it)
    assert L.snesimage_shared_guided_costs(sp._s, 0, 0, None) == ERR_ARG and L.snesimage_shared_guided_candidates(sp._s, 0, 0, 4, None, None) == ERR_ARG
    # a lent member's own guided calls keep answering SNES_ERR_STATE
    g = ctxs[0]
    for fn in (lambda: g.guided_costs(0, 0), lambda: g.guided_candidates(0, 0), lambda: g.guided_step(0, 0), lambda: g.guided_step_async(0, 0), lambda: g.guided_sweep()):
        refused(S, fn, ERR_STATE)
    assert state_of(sp, ctxs) == before
    # an NES set
    nctx = [S.OptimizedImage(f, 2, 3, nes=True) for f in r["imgs"]]
    for c in nctx:
        c.set_chunk(64)
    nsp = S.SharedPalette(nctx)
    nsp.initialize_tiles()
    nsp.recalculate_palettes()
    nbefore = state_of(nsp, nctx)
    all_refused(S, nsp, UNSUPPORTED)
    assert state_of(nsp, nctx) == nbefore
    nsp.step(S.METHOD_NES, 0, 0)
    close_all(nsp, nctx)
    # a member stepped outside the set: what every set call answers
    octx, osp = case_set(S, r)
    octx[1].step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)
    all_refused(S, osp, ERR_STATE)
    close_all(osp, octx)
    # after all of them a guided step still follows the model
    rec = r["recs"][0]
    err, best = sp.guided_step(rec["p"], rec["i"], r["K"])
    assert sp.last_step()[1] == rec["best_k"] and np.array_equal(best, rec["rgb5"]) and close(err, rec["error"])
    assert_state(sp, ctxs, rec, "behind the refusals")
    close_all(sp, ctxs)


@pytest.mark.gpu
def test_more_than_8192_tiles_are_refused(S):
    """Nine members of 256 x 256: 9,216 tiles.  Every entry point answers SNES_ERR_UNSUPPORTED and the set goes on."""
    from snesimage_amd.synth import synth_image
    img = synth_image(0x5EED5A00, 256, 256, 0)
    ctxs = [S.OptimizedImage(img, 1, 3, device=0) for _ in range(9)]
    for c in ctxs:
        c.set_chunk(64)
    sp = S.SharedPalette(ctxs)
    all_refused(S, sp, UNSUPPORTED)
    sp.step(S.METHOD_RANDOM, 0, 1, 0, 3, 0, 8)
    close_all(sp, ctxs)


# ---- the headless driver --------------------------------------------------------------------------------------------------

def drive(S, sp, calls, every, k, seed=1, fixed=False):
    """The CLI's loop on a set, call by call: scheduled calls of 64, one guided sweep of the set behind every `every` sweeps of
    the palette.  fixed: --set-backdrop-fixed, whose schedule and guided sweeps pass the backdrop slot by."""
    sched = S.schedule(sp.sub_count, sp.sub_size, calls + 1)
    sweeps = 0
    for j in range(calls):
        method, p, i, ch, step = sched[j]
        sp.step(method, p, i, ch, seed, j, 64 if method == S.METHOD_RANDOM else 0)
        after = sched[j + 1][4]
        if after != step and after % every == 0:
            if fixed:
                for p, i in [(p, i) for p in range(sp.sub_count) for i in range(sp.sub_size)]:
                    sp.guided_step(p, i, k)
            else:
                sp.guided_sweep(k)
            sweeps += 1
    return sweeps


def cli_calls(S):
    sched = S.schedule(2, 3, 64)
    ends = [j for j in range(63) if sched[j + 1][4] != sched[j][4]]
    return ends[1] + 3  # two sweeps of the palette end inside the run, and it stops in the middle of the third


@pytest.mark.gpu
def test_cli_set_guided_sweeps_write_what_the_library_writes(tmp_path, S):
    from snesimage_amd.synth import synth_image
    calls = cli_calls(S)

    def run(tag, *extra):
        outs = [str(tmp_path / ("%s%d.json" % (tag, i))) for i in range(2)]
        r = run_cli("synth:1", outs[0], "--share", "synth:2=" + outs[1], "-c", "2", "-s", "3", "--seed", "1", "--calls", str(calls), *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        return [open(o).read() for o in outs], r.stdout

    a, out = run("a", "--set-guided", "1", "--set-guided-shortlist", "8")
    assert out.count("Guided sweep of the set: 6 calls, ") == 2, out
    ctxs = [S.OptimizedImage(synth_image(s, 256, 256, 0), 2, 3) for s in (1, 2)]
    sp = S.SharedPalette(ctxs)
    sp.initialize_tiles()
    sp.recalculate_palettes()
    assert drive(S, sp, calls, 1, 8) == 2
    assert [c.as_json() for c in ctxs] == a
    close_all(sp, ctxs)
    b, out = run("b", "--set-guided", "1", "--set-guided-shortlist", "8", "--window", "1")
    assert b == a and out.count("Guided sweep of the set: 6 calls, ") == 2
    plain, _ = run("p")
    assert plain != a, "the guided sweeps changed nothing: the comparison shows nothing"


@pytest.mark.gpu
def test_cli_set_guided_sweeps_pass_a_fixed_backdrop_by(tmp_path, S):
    from snesimage_amd.synth import synth_image

    def run(tag, *extra):
        outs = [str(tmp_path / ("%s%d.json" % (tag, i))) for i in range(2)]
        r = run_cli("synth:1", outs[0], "--share", "synth:2=" + outs[1], "-c", "2", "-s", "3", "--seed", "1", "--set-backdrop-fixed", "1,2,30", "--set-guided", "1",
                    "--set-guided-shortlist", "8", "--calls", "14", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        return [open(o).read() for o in outs], r.stdout

    a, out = run("a", "--window", "1")
    assert out.count("Guided sweep of the set: 6 calls, ") == 2, out
    ctxs = [S.OptimizedImage(synth_image(s, 256, 256, 0), 2, 3, backdrop=True) for s in (1, 2)]
    sp = S.SharedPalette(ctxs, backdrop=(1, 2, 30))
    sp.initialize_tiles()
    sp.recalculate_palettes()
    assert drive(S, sp, 14, 1, 8, fixed=True) == 2
    assert np.array_equal(sp.backdrop, [1, 2, 30]) and [c.as_json() for c in ctxs] == a
    close_all(sp, ctxs)
    b, _ = run("b")
    assert b == a
