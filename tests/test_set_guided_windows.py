"""Guided calls of a set through the slot windows (include/snesimage_hip.h: snesimage_shared_guided_run_slots; DESIGN 5f'''').

The reference of every test is a twin set stepped by guided_step call by call: the windows promise its bits.  The cases and their
recorded decisions are tests/set_guided_window_model.py's, checked against the model on the CPU by
tests/test_set_guided_window_model.py; the head of each trajectory is also compared with the model (set_guided_model.trajectory).
The shortlists the calls scored are read back through the test hook snesimage_shared_debug_guided_capture and compared, call by
call and rejected calls included, with the twin's guided_candidates before its call; the tables of the windows' generator are read
back through snesimage_shared_debug_guided_window_costs and compared, all 32,768 values, with guided_costs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guided_model as GM
import ordered_model as OM
import set_backdrop_model as SB
import set_guided_model as SGM
import set_guided_window_model as SGW
from test_set_guided import assert_costs_equal, case_set, close, close_all, hand_tiles, make_set, refused, state_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
WINDOWS = (0, 1, 2, 3, 64)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def slot_order(sp):
    return [(p, i) for p in range(sp.sub_count) for i in range(sp.sub_size)] + ([(sp.sub_count, 0)] if sp.has_backdrop else [])


def step_twin(twin, n, K, state=(0, 0), shortlists=False):
    """n guided set calls one by one from `state` on -> (log, next state, shortlists before each call)."""
    sl = slot_order(twin)
    at = sl.index(tuple(state))
    log, lists = [], []
    for j in range(n):
        p, i = sl[(at + j) % len(sl)]
        if shortlists:
            lists.append(twin.guided_candidates(p, i, K)[0])
        twin.guided_step(p, i, K)
        log.append(twin.last_step())
    return log, sl[(at + n) % len(sl)], lists


def observed(sp, ctxs):
    e, k, b, ch = sp.last_step()
    return dict(state=state_of(sp, ctxs), backdrop=sp.backdrop.tolist() if sp.has_backdrop else None, last=(e, k, b.tolist(), ch))


def assert_logs_equal(got, want, what):
    assert len(got) == len(want), what
    for j, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3], (what, j, a, b)  # the error's bits


def assert_shortlists_equal(got, want, K, what):
    """Every call's shortlist as the scorers read it, rejected calls included, against the twin's before its call."""
    assert got.shape == (len(want), K, 3), (what, got.shape)
    for j, cand in enumerate(want):
        assert np.array_equal(got[j], cand), (what, "call %d" % j, GM.pack_u(got[j]).tolist(), GM.pack_u(cand).tolist())


_twins = {}


def twin_of_case(S, O, name):
    """The case's three sweeps stepped call by call, once."""
    if name not in _twins:
        r = SGM.trajectory(O, name)
        ctxs, t = case_set(S, r)
        log, state, lists = step_twin(t, SGW.n_calls(name), r["K"], shortlists=True)
        _twins[name] = dict(log=log, state=state, end=observed(t, ctxs), lists=lists)
        close_all(t, ctxs)
    return _twins[name]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_every_window_size_equals_the_calls_one_by_one(S, O, name, window):
    r, want, n = SGM.trajectory(O, name), twin_of_case(S, O, name), SGW.n_calls(name)
    ctxs, sp = case_set(S, r)
    sp.debug_guided_capture()
    log, state, stats = sp.guided_run_slots(n, r["K"], window=window)
    what = "%s window %d" % (name, window)
    assert_shortlists_equal(sp.debug_guided_shortlists(), want["lists"], r["K"], what)
    print(what, stats, "".join(str(x[3]) for x in log))
    assert_logs_equal(log, want["log"], what)
    assert observed(sp, ctxs) == want["end"], what
    assert state == want["state"] == (0, 0)
    assert "".join(str(x[3]) for x in log) == SGW.CHANGED[name], what
    for j, rec in enumerate(r["recs"]):  # the head of the trajectory against the model
        assert log[j][1] == rec["best_k"] and np.array_equal(log[j][2], rec["rgb5"]) and log[j][3] == rec["changed"] and close(log[j][0], rec["error"]), (what, j)
    assert stats["calls"] == n and stats["accepted"] == SGW.CHANGED[name].count("1") and stats["voided"] == 0
    assert stats["useful"] == n * r["K"] <= stats["scored"]
    if window == 1:
        assert stats["windows"] == n and stats["scored"] == stats["useful"]
    elif window:
        sets = SGW.consume(name, window)
        assert stats["windows"] == len(sets) and stats["scored"] == r["K"] * sum(s["taken"] for s in sets), (what, stats)
    if window == 64:
        assert stats["windows"] < n
    close_all(sp, ctxs)


@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_a_run_in_pieces_equals_one_run(S, O, name):
    r, want, n = SGM.trajectory(O, name), twin_of_case(S, O, name), SGW.n_calls(name)
    ctxs, sp = case_set(S, r)
    log, state = [], (0, 0)
    for piece in (1, 5, 7, n - 13):
        part, state, stats = sp.guided_run_slots(piece, r["K"], state=state)
        assert stats["calls"] == piece
        log += part
    assert_logs_equal(log, want["log"], name)
    assert observed(sp, ctxs) == want["end"], name
    assert state == want["state"]
    close_all(sp, ctxs)


def test_a_guided_run_leaves_the_scheduled_windows_as_they_were(S, O):
    """The adaptive size of a set's guided windows is their own: the two scheduled runs around a guided run take the launch sets
    they take on a set whose guided calls were stepped one by one."""
    r = SGM.trajectory(O, "plain-f2-4x7")
    (actx, a), (bctx, b) = case_set(S, r), case_set(S, r)
    la1, sa, ta1 = a.run_slots(40, seed=3, n_random=16)
    lb1, sb, tb1 = b.run_slots(40, seed=3, n_random=16)
    ga, _, gstats = a.guided_run_slots(56, r["K"])
    gb, _, _ = step_twin(b, 56, r["K"])
    assert_logs_equal(ga, gb, "the guided calls between the runs")
    assert gstats["windows"] < 56
    la2, sa2, ta2 = a.run_slots(60, seed=3, first_step_id=40, state=sa, n_random=16)
    lb2, sb2, tb2 = b.run_slots(60, seed=3, first_step_id=40, state=sb, n_random=16)
    assert_logs_equal(la1, lb1, "first scheduled run")
    assert_logs_equal(la2, lb2, "second scheduled run")
    assert sa == sb and sa2 == sb2 and ta1 == tb1 and ta2 == tb2, (ta1, tb1, ta2, tb2)
    assert observed(a, actx) == observed(b, bctx)
    close_all(a, actx)
    close_all(b, bctx)


# ---- the generator's tables --------------------------------------------------------------------------------------------------

def assert_window_costs(sp, slots, what):
    """One window over `slots` (a slot repeats): every call's table is guided_costs of its slot, and nothing else changed."""
    got = sp.debug_guided_window_costs(slots)
    assert got.shape == (len(slots), 32768)
    for j, (p, i) in enumerate(slots):
        assert_costs_equal(got[j], sp.guided_costs(p, i), "%s, call %d slot (%d, %d)" % (what, j, p, i))
    return got


REPEATING = [(0, 0), (0, 1), (1, 2), (0, 2), (1, 0), (0, 1), (1, 1), (0, 0)]


def test_window_tables_from_the_kmeans_start_and_with_equal_entries(S, O):
    r = SGM.trajectory(O, "plain-f2-2x3")
    ctxs, sp = case_set(S, r)
    before = state_of(sp, ctxs)
    got = assert_window_costs(sp, REPEATING, "k-means start")
    assert np.array_equal(got[0], got[7]) and np.array_equal(got[1], got[5]) and got.any()
    assert state_of(sp, ctxs) == before, "the hook changed the state"
    pal = sp.palette
    pal[1] = pal[0]  # two equal entries in subpalette 0: their pixels have a == b, whichever is called the nearest
    pal[5] = pal[3]
    sp.palette = pal
    assert_window_costs(sp, REPEATING, "equal entries")
    close_all(sp, ctxs)


def test_window_tables_of_an_emptied_subpalette_and_of_an_entry_nearest_to_no_pixel(S):
    imgs = SB.frames(2, 16)
    tiles = hand_tiles(2, 64, lambda f, k: 0)  # subpalette 1: no tiles
    pal = np.array([[10, 12, 7], [3, 20, 25], [31, 0, 31], [5, 5, 5], [20, 20, 20], [0, 31, 0]], np.uint8)
    ctxs, sp = make_set(S, imgs, 2, 3, None, tiles, pal)
    got = assert_window_costs(sp, REPEATING, "subpalette 1 emptied")
    assert not got[2].any() and not got[4].any() and not got[6].any() and got[0].any()
    close_all(sp, ctxs)


def test_window_tables_of_one_entry_subpalettes_and_a_list_of_many_slices(S):
    imgs = SB.frames(3, 16)
    tiles = hand_tiles(3, 64, lambda f, k: (k + f) % 3)
    ctxs, sp = make_set(S, imgs, 3, 1, None, tiles, np.array([[10, 12, 7], [3, 20, 25], [28, 27, 30]], np.uint8))
    assert_window_costs(sp, [(0, 0), (1, 0), (2, 0), (1, 0)], "3 x 1")
    close_all(sp, ctxs)
    # 1 x 1 over three frames: the one call's own list is every pixel, 12 slices of 1,024: more than the difference kernel's grid takes at once
    ctxs, sp = make_set(S, imgs, 1, 1, None, hand_tiles(3, 64, lambda f, k: 0), np.array([[10, 12, 7]], np.uint8))
    assert_window_costs(sp, [(0, 0), (0, 0)], "1 x 1")
    close_all(sp, ctxs)


def test_window_tables_with_transparent_pixels(S, O):
    imgs = SB.frames(2, 16)
    imgs[1] = OM.with_hole(imgs[1])
    assert (imgs[1][..., 3] == 0).any()
    m = SGM.SetModel(O, imgs, 2, 3)
    ctxs, sp = make_set(S, m.imgs, m.C, m.S, m.flags, m.tiles, m.palette)
    assert_window_costs(sp, REPEATING, "a hole in member 1")
    close_all(sp, ctxs, m)


def test_window_tables_read_the_ordered_dither_targets(S, O):
    table = OM.bayer(4, 64)
    m = SGM.SetModel(O, SB.frames(2, 16), 2, 3)
    ctxs, sp = make_set(S, m.imgs, m.C, m.S, m.flags, m.tiles, m.palette, None, table)
    got = assert_window_costs(sp, REPEATING, "Bayer 4 x 4")
    Ts = [OM.target_image(f, table) for f in m.imgs]
    assert_costs_equal(got[2], m.costs(1, 2, Ts), "Bayer 4 x 4 against the model on T")
    assert (m.costs(1, 2) != got[2]).any(), "the table changes no cost: the case shows nothing"
    close_all(sp, ctxs, m)


def test_window_tables_of_a_backdrop_sets_regular_slots(S, O):
    imgs = SB.frames(2, 16)
    m = SGM.SetModel(O, imgs, 2, 3, {}, SB.stack_backdrop(O, imgs, {}))  # the stack's mean: a B that is some pixels' nearest entry
    ctxs, sp = make_set(S, m.imgs, m.C, m.S, m.flags, m.tiles, m.palette, m.B)
    got = assert_window_costs(sp, REPEATING, "backdrop set")
    assert_costs_equal(got[6], m.costs(1, 1), "backdrop set against the model")
    refused(S, lambda: sp.debug_guided_window_costs([(0, 0), (2, 0)]), ERR_ARG)  # the tied slot is never a window's
    close_all(sp, ctxs, m)


# ---- what stays call by call ------------------------------------------------------------------------------------------------

def run_against_twin(S, r, n, window, prepare=None):
    (ctxs, sp), (tctxs, twin) = case_set(S, r), case_set(S, r)
    if prepare:
        prepare(sp)
        prepare(twin)
    want, want_state, lists = step_twin(twin, n, r["K"], shortlists=True)
    sp.debug_guided_capture()
    log, state, stats = sp.guided_run_slots(n, r["K"], window=window)
    assert_shortlists_equal(sp.debug_guided_shortlists(), lists, r["K"], "shortlists")
    assert_logs_equal(log, want, "logs")
    assert state == want_state and observed(sp, ctxs) == observed(twin, tctxs)
    close_all(sp, ctxs)
    close_all(twin, tctxs)
    return log, stats


def test_a_cielab_set_is_stepped_call_by_call(S, O):
    r = SGM.trajectory(O, "perceptual-f2-2x3")

    def cielab(sp):
        sp.guided_proxy = "cielab"

    log, stats = run_against_twin(S, r, 8, 0, cielab)
    assert stats["windows"] == stats["calls"] == 8 and stats["scored"] == stats["useful"] == 8 * r["K"]
    assert any(x[3] for x in log)


def child_more_members_than_slot_contexts():
    """Runs in a child process under SNES_WINDOW_MAX=3: a set of two members holds one call per window, so it steps call by call."""
    import snesimage_amd as S
    imgs = SB.frames(2, 16)
    sets = []
    for _ in range(2):
        ctxs = [S.OptimizedImage(f, 2, 3) for f in imgs]
        for c in ctxs:
            c.set_chunk(64)
        sp = S.SharedPalette(ctxs)
        sp.initialize_tiles()
        sp.recalculate_palettes()
        sets.append((ctxs, sp))
    (ctxs, sp), (tctxs, twin) = sets
    want, want_state, _ = step_twin(twin, 8, 16)
    log, state, stats = sp.guided_run_slots(8, 16)
    assert_logs_equal(log, want, "logs")
    assert state == want_state and observed(sp, ctxs) == observed(twin, tctxs)
    assert stats["windows"] == stats["calls"] == 8 and stats["scored"] == stats["useful"] == 8 * 16, stats
    assert any(x[3] for x in log) and not all(x[3] for x in log)
    close_all(sp, ctxs)
    close_all(twin, tctxs)
    print("CHILD-OK")


def test_a_set_of_more_members_than_slot_contexts_is_stepped_call_by_call():
    env = dict(os.environ, SNES_WINDOW_MAX="3", PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, "-c", "import test_set_guided_windows as T; T.child_more_members_than_slot_contexts()"], env=env, cwd=os.path.join(ROOT, "tests"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, r.stdout + r.stderr


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_and_a_failed_workspace_allocation_leave_the_set_usable(S, O):
    from snesimage_amd import _ffi
    import ctypes as C
    L = _ffi.load()
    r = SGM.trajectory(O, "plain-f2-2x3")
    ctxs, sp = case_set(S, r)
    before = state_of(sp, ctxs)
    refused(S, lambda: sp.guided_run_slots(4, 65), ERR_ARG)
    refused(S, lambda: sp.guided_run_slots(4, state=(2, 0)), ERR_ARG)  # the tied slot of a plain set
    refused(S, lambda: sp.guided_run_slots(4, state=(0, 3)), ERR_ARG)
    p, i = C.c_uint32(0), C.c_uint32(0)
    assert L.snesimage_shared_guided_run_slots(sp._s, 4, 16, None, C.byref(i), 0, None, None) == ERR_ARG
    assert L.snesimage_shared_guided_run_slots(sp._s, 4, 16, C.byref(p), None, 0, None, None) == ERR_ARG
    refused(S, lambda: sp.debug_guided_window_costs([(0, 3)]), ERR_ARG)
    refused(S, lambda: sp.debug_guided_window_costs([(0, 0)] * 33), ERR_ARG)  # more calls than a window of two members holds
    refused(S, lambda: sp.debug_guided_window_costs([]), ERR_ARG)
    assert state_of(sp, ctxs) == before
    # the windows' generator workspace: four allocations, all or nothing (the single calls' workspace and the windows' records exist)
    sp.guided_candidates(0, 0, 16)
    sp.reserve_slots(1)
    assert state_of(sp, ctxs) == before
    for nth in (0, 1, 2, 3):
        L.snesimage_debug_fail_alloc(nth)
        try:
            assert "workspace" in refused(S, lambda: sp.guided_run_slots(6, 16), ERR_HIP)
        finally:
            L.snesimage_debug_fail_alloc(-1)
        assert state_of(sp, ctxs) == before
    # an NES set; a member stepped outside the set
    nctx = [S.OptimizedImage(f, 2, 3, nes=True) for f in r["imgs"]]
    for c in nctx:
        c.set_chunk(64)
    nsp = S.SharedPalette(nctx)
    nsp.initialize_tiles()
    nsp.recalculate_palettes()
    nbefore = state_of(nsp, nctx)
    refused(S, lambda: nsp.guided_run_slots(4), UNSUPPORTED)
    assert state_of(nsp, nctx) == nbefore
    close_all(nsp, nctx)
    octx, osp = case_set(S, r)
    octx[1].step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)
    refused(S, lambda: osp.guided_run_slots(4), ERR_STATE)
    close_all(osp, octx)
    # behind all of them the run equals the twin
    tctxs, twin = case_set(S, r)
    want, want_state, _ = step_twin(twin, 12, r["K"])
    log, state, stats = sp.guided_run_slots(12, r["K"])
    assert_logs_equal(log, want, "behind the refusals")
    assert state == want_state and observed(sp, ctxs) == observed(twin, tctxs) and stats["windows"] < 12
    close_all(sp, ctxs)
    close_all(twin, tctxs)


# ---- the headless driver ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fixed", [False, True])
def test_cli_writes_the_same_files_and_info_lines_for_every_window(tmp_path, S, fixed):
    from test_set_guided import cli_calls
    calls = 14 if fixed else cli_calls(S)  # two sweeps of the palette end inside the run (the fixed backdrop runs the plain schedule)
    got = []
    for window in ("0", "1", "3"):
        outs = [str(tmp_path / ("w%s-%d.json" % (window, i))) for i in range(2)]
        extra = ["--set-backdrop-fixed", "1,2,30"] if fixed else []
        r = subprocess.run([CLI, "synth:1", outs[0], "--share", "synth:2=" + outs[1], "-c", "2", "-s", "3", "--seed", "1", "--calls", str(calls), "--set-guided", "1",
                            "--set-guided-shortlist", "8", "--window", window, *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [x for x in r.stdout.splitlines() if "Guided sweep of the set: " in x]
        assert len(lines) == 2 and all("Guided sweep of the set: 6 calls, " in x for x in lines), r.stdout
        got.append(([open(o).read() for o in outs], [x[x.index("Guided sweep"):] for x in lines]))
    assert got[0] == got[1] == got[2]
