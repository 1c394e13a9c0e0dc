"""Guided calls through the slot windows (include/snesimage_hip.h: snesimage_guided_run_slots; DESIGN 5f''').

The reference of every test is a twin context stepped by guided_step call by call: the windows promise its bits.  The cases
and their recorded decisions are tests/guided_window_model.py's, checked against the model on the CPU by
tests/test_guided_window_model.py; the head of each trajectory is also compared with the model (guided_model.trajectory).
The shortlists the calls scored are read back through the test hook snesimage_debug_guided_capture and compared, call by call
and rejected calls included, with the twin's guided_candidates before its call."""
import os
import subprocess

import numpy as np
import pytest

import guided_model as GM
import guided_window_model as GW
import ordered_model as OM
from test_guided import case_context, close, refused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
WINDOWS = (0, 1, 2, 3, 64)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def slot_order(g):
    return [(p, i) for p in range(g.sub_count) for i in range(g.sub_size)] + ([(g.sub_count, 0)] if g.has_backdrop else [])


def step_twin(twin, n, K, state=(0, 0), shortlists=False):
    """n guided calls one by one from `state` on -> (log, next state, shortlists before each call)."""
    sl = slot_order(twin)
    at = sl.index(tuple(state))
    log, lists = [], []
    for j in range(n):
        p, i = sl[(at + j) % len(sl)]
        if shortlists:
            lists.append(twin.guided_candidates(p, i, K)[0])
        twin.guided_step(p, i, K)
        e, b, k = twin.last_step()
        log.append((e, k, b, int(k >= 0)))
    return log, sl[(at + n) % len(sl)], lists


def observed(g):
    e, b, k = g.last_step()
    return dict(palette=g.palette, backdrop=g.backdrop if g.has_backdrop else None, pmap=g.palette_map, error=g.error(), last=(e, b.tolist(), k))


def assert_logs_equal(got, want, what):
    assert len(got) == len(want), what
    for j, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3], (what, j, a, b)  # the error's bits


def assert_observed_equal(g, want, what):
    got = observed(g)
    assert np.array_equal(got["palette"], want["palette"]) and np.array_equal(got["pmap"], want["pmap"]), what
    assert want["backdrop"] is None or np.array_equal(got["backdrop"], want["backdrop"]), what
    assert got["error"] == want["error"] and got["last"] == want["last"], (what, got["error"], want["error"], got["last"], want["last"])


def assert_shortlists_equal(got, want, K, what):
    """Every call's shortlist as the scorer read it, rejected calls included, against the twin's before its call."""
    assert got.shape == (len(want), K, 3), (what, got.shape)
    for j, cand in enumerate(want):
        assert np.array_equal(got[j], cand), (what, "call %d" % j, GM.pack_u(got[j]).tolist(), GM.pack_u(cand).tolist())


_twins = {}


def twin_of_case(S, O, name):
    """The case's three sweeps stepped call by call, once."""
    if name not in _twins:
        r = GM.trajectory(O, name)
        t = case_context(S, r)
        log, state, lists = step_twin(t, GW.n_calls(name), r["K"], shortlists=True)
        _twins[name] = dict(log=log, state=state, end=observed(t), lists=lists)
        t.close()
    return _twins[name]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_every_window_size_equals_the_calls_one_by_one(S, O, name, window):
    r, want, n = GM.trajectory(O, name), twin_of_case(S, O, name), GW.n_calls(name)
    g = case_context(S, r)
    g.debug_guided_capture()
    log, state, stats = g.guided_run_slots(n, r["K"], window=window)
    what = "%s window %d" % (name, window)
    assert_shortlists_equal(g.debug_guided_shortlists(), want["lists"], r["K"], what)
    print(what, stats, "".join(str(x[3]) for x in log))
    assert_logs_equal(log, want["log"], what)
    assert_observed_equal(g, want["end"], what)
    assert state == want["state"] == (0, 0)
    assert "".join(str(x[3]) for x in log) == GW.CHANGED[name], what
    for j, rec in enumerate(r["recs"]):
        assert log[j][1] == rec["best_k"] and np.array_equal(log[j][2], rec["rgb5"]) and log[j][3] == rec["changed"] and close(log[j][0], rec["error"]), (what, j)
    assert stats["calls"] == n and stats["useful"] <= stats["scored"] and stats["accepted"] == GW.CHANGED[name].count("1")
    assert stats["useful"] == n * r["K"]
    if window == 1:
        assert stats["windows"] == n and stats["scored"] == stats["useful"] and stats["voided"] == 0
    elif window:
        sets = GW.consume(name, window)
        assert stats["windows"] == len(sets) and stats["scored"] == r["K"] * sum(s["taken"] for s in sets), (what, stats)
    if window == 64:
        assert stats["windows"] < n
    if name == "plain-4x7" and window in (2, 3):
        assert stats["voided"] > 0, "no window was enqueued ahead and voided on the device"
    g.close()


@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_a_run_in_pieces_equals_one_run(S, O, name):
    r, want, n = GM.trajectory(O, name), twin_of_case(S, O, name), GW.n_calls(name)
    g = case_context(S, r)
    log, state = [], (0, 0)
    for piece in (1, 5, 7, n - 13):
        part, state, stats = g.guided_run_slots(piece, r["K"], state=state)
        assert stats["calls"] == piece
        log += part
    assert_logs_equal(log, want["log"], name)
    assert_observed_equal(g, want["end"], name)
    assert state == want["state"]
    g.close()


def test_a_guided_run_leaves_the_scheduled_windows_as_they_were(S, O):
    """The adaptive size and the clean streak of guided windows are their own: the two scheduled runs around a guided run take the
    launch sets they take on a context whose guided calls were stepped one by one."""
    r = GM.trajectory(O, "plain-4x7")
    a, b = case_context(S, r), case_context(S, r)
    la1, sa, ta1 = a.run_slots(40, seed=3)
    lb1, sb, tb1 = b.run_slots(40, seed=3)
    ga, _, gstats = a.guided_run_slots(56, r["K"])
    gb, _, _ = step_twin(b, 56, r["K"])
    assert_logs_equal(ga, gb, "the guided calls between the runs")
    assert gstats["windows"] < 56
    la2, sa2, ta2 = a.run_slots(60, seed=3, first_step_id=40, state=sa)
    lb2, sb2, tb2 = b.run_slots(60, seed=3, first_step_id=40, state=sb)
    assert_logs_equal(la1, lb1, "first scheduled run")
    assert_logs_equal(la2, lb2, "second scheduled run")
    assert sa == sb and sa2 == sb2 and ta1 == tb1 and ta2 == tb2, (ta1, tb1, ta2, tb2)
    assert_observed_equal(a, observed(b), "after the three runs")
    a.close()
    b.close()


def started(S, img, C, Sz, table=None, **flags):
    g = S.OptimizedImage(img, C, Sz, **flags)
    if table is not None:
        g.set_ordered_dither(table)
    g.initialize_tiles()
    if Sz > 1:
        g.recalculate_palettes()
    else:  # (the k-means of a subpalette needs two entries)
        g.palette = [[10, 12, 7], [20, 9, 25]][:C]
        g.optimize()
    return g


def twin_in_state(S, g, img, C, Sz, table=None, **flags):
    t = S.OptimizedImage(img, C, Sz, **flags)
    if table is not None:
        t.set_ordered_dither(table)
    t.tile_palettes, t.palette = g.tile_palettes, g.palette
    t.optimize()
    return t


def run_against_twin(S, g, t, n, K, state, window, what):
    want, want_state, lists = step_twin(t, n, K, state, shortlists=True)
    g.debug_guided_capture()
    log, got_state, stats = g.guided_run_slots(n, K, state=state, window=window)
    got_lists = g.debug_guided_shortlists()
    g.debug_guided_capture(False)
    assert_shortlists_equal(got_lists, lists, K, what)
    print(what, stats, "".join(str(x[3]) for x in log))
    assert_logs_equal(log, want, what)
    assert got_state == want_state
    assert_observed_equal(g, observed(t), what)
    for j, x in enumerate(log):  # an accepted colour is the twin's shortlist entry best_k
        assert (x[1] >= 0) == bool(x[3]) and (x[1] < 0 or np.array_equal(x[2], lists[j][x[1]])), (what, j)
    return log, stats, got_lists


@pytest.mark.parametrize("window", [3, 64])
def test_window_on_one_subpalette_and_two_slices_per_list(S, window):
    img = GM.image(8, 5)  # 256 x 8 at 1 x 4: every call's list holds all 2,048 pixels, two slices
    g = started(S, img, 1, 4)
    t = twin_in_state(S, g, img, 1, 4)
    log, stats, lists = run_against_twin(S, g, t, 12, 16, (0, 0), window, "1 x 4 window %d" % window)
    assert stats["windows"] < 12
    g.close()
    t.close()


@pytest.mark.parametrize("window", [3, 64])
def test_window_with_empty_lists_in_its_middle(S, window):
    img = GM.image(24, 7)

    def emptied(g):
        tp = g.tile_palettes
        assert (tp == 3).any()
        tp[tp == 3] = 0
        g.tile_palettes = tp
        g.optimize()

    g = started(S, img, 4, 7)
    emptied(g)
    t = twin_in_state(S, g, img, 4, 7)
    assert not g.guided_costs(3, 2).any()
    pal = g.palette
    log, stats, lists = run_against_twin(S, g, t, 30, 8, (2, 5), window, "4 x 7 without subpalette 3, window %d" % window)
    assert not any(x[3] for x in log[2:9]), "a call on the unused subpalette was accepted: all its costs and all its errors tie"
    for i in range(7):  # calls 2 .. 8 are slots (3, 0) .. (3, 6): every cost is 0, so the order is the colours' own, the slot's colour left out
        cur = int(GM.pack_u(pal[3 * 7 + i]))
        assert GM.pack_u(lists[2 + i]).tolist() == [u for u in range(9) if u != cur][:8], (window, i)
    g.close()
    t.close()


def test_window_with_transparent_pixels(S):
    img = OM.with_hole(GM.image(104, 8, variant=1))
    g = started(S, img, 2, 3)
    t = twin_in_state(S, g, img, 2, 3)
    run_against_twin(S, g, t, 12, 16, (0, 0), 64, "alpha image")
    g.close()
    t.close()


def test_window_reads_the_ordered_dither_target(S):
    img, table = GM.image(16, 9), OM.bayer(4, 64)
    g = started(S, img, 2, 3, table)
    assert not np.array_equal(g.target_rgba(), img)
    t = twin_in_state(S, g, img, 2, 3, table)
    run_against_twin(S, g, t, 12, 16, (0, 0), 64, "Bayer 4 x 4")
    g.close()
    t.close()


@pytest.mark.parametrize("kind", ["dither-one-entry", "cielab"])
def test_what_the_windows_do_not_cover_is_stepped_call_by_call(S, kind):
    img = GM.image(8, 6)
    flags = dict(dither=True) if kind == "dither-one-entry" else {}
    g = started(S, img, 2, 1, **flags)
    t = twin_in_state(S, g, img, 2, 1, **flags)
    if kind == "cielab":
        g.guided_proxy = t.guided_proxy = "cielab"
    log, stats, lists = run_against_twin(S, g, t, 6, 16, (0, 0), 0, kind)
    assert stats["windows"] == stats["calls"] == 6 and stats["scored"] == stats["useful"] == 6 * 16
    g.close()
    t.close()


def test_refusals_leave_the_context_usable(S):
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = GM.image(16, 12)

    def state(g):
        return (g.error(), g.palette.tobytes(), g.palette_map.tobytes())

    g = started(S, img, 2, 3, nes=True)
    before = state(g)
    refused(S, lambda: g.guided_run_slots(4), UNSUPPORTED)
    assert state(g) == before
    g.close()
    g = started(S, img, 2, 3)
    g.set_chunk(64)
    before = state(g)
    sp = S.SharedPalette([g])
    refused(S, lambda: g.guided_run_slots(4), ERR_STATE)  # lent to a set
    sp.close()
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    refused(S, lambda: g.guided_run_slots(4), ERR_STATE)  # between the phases of a split-phase step
    g.step_commit(buf.ptr)
    before = state(g)
    refused(S, lambda: g.guided_run_slots(4, 65), ERR_ARG)
    refused(S, lambda: g.guided_run_slots(4, state=(2, 0)), ERR_ARG)
    refused(S, lambda: g.guided_run_slots(4, state=(0, 3)), ERR_ARG)
    # the windows' generator workspace: two allocations, all or nothing (the single calls' workspace and the windows' records exist)
    g.guided_costs(0, 0)
    g.slots_reserve(1)
    assert state(g) == before
    for nth in (0, 1):
        L.snesimage_debug_fail_alloc(nth)
        try:
            assert "workspace" in refused(S, lambda: g.guided_run_slots(6, 8), ERR_HIP)
        finally:
            L.snesimage_debug_fail_alloc(-1)
        assert state(g) == before
    t = twin_in_state(S, g, img, 2, 3)
    run_against_twin(S, g, t, 12, 8, (0, 0), 0, "behind the refusals")
    g.close()
    t.close()


def test_cli_writes_the_same_file_for_every_window(tmp_path):
    img = GM.image(16, 13)
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    outs = []
    for window in ("0", "3", "1"):
        out = str(tmp_path / ("w%s.json" % window))
        r = subprocess.run([CLI, str(src), out, "-c", "2", "-s", "3", "--seed", "1", "--guided", "1", "--guided-shortlist", "8", "--calls", "40", "--window", window],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("Guided sweep: 6 calls, ") >= 2, r.stdout
        outs.append(open(out).read())
    assert outs[0] == outs[1] == outs[2]
