"""The recorded decisions of tests/guided_window_model.py against the model, the premises the GPU tests of the guided windows
rest on, and the ABI of snesimage_guided_run_slots — all on the CPU."""
import ctypes as C
import os

import pytest

import guided_model as GM
import guided_window_model as GW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_recorded_decisions_are_the_models(O, name):
    recs, min_gap = GW.run(O, name)  # asserts the gap premise at every comparison
    sl = GW.slots(name)
    changed = "".join(str(r["changed"]) for r in recs)
    print("%s: %d calls, smallest non-zero gap %.2e, changed %s" % (name, len(recs), min_gap, changed))
    assert len(recs) == GW.n_calls(name) == len(GW.CHANGED[name]) and min_gap > GM.MIN_GAP
    assert [(r["p"], r["i"]) for r in recs] == [sl[j % len(sl)] for j in range(len(recs))]
    assert changed == GW.CHANGED[name]
    # the trajectory the GPU tests of the single calls follow is the head of this one
    for a, b in zip(GM.trajectory(O, name)["recs"], recs):
        assert (a["p"], a["i"], a["best_k"], a["changed"]) == (b["p"], b["i"], b["best_k"], b["changed"]) and a["error"] == b["error"]


@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_windows_over_the_recorded_decisions_void_calls_and_come_back_clean(name):
    """One combination cannot hold the second premise: the last of plain-4x7's 84 calls accepts, so at window 64 — where a clean
    window would take everything that is left — the last window accepts and none before it is clean.  That is asserted as it is;
    plain-4x7 has clean windows at 2 and 3 (below), the other four cases at 64 as well."""
    n = GW.n_calls(name)
    for window in (3, 64):
        sets = GW.consume(name, window)
        assert sum(s["used"] for s in sets) == n and all(1 <= s["used"] <= s["taken"] <= window for s in sets)
        assert any(s["accepted"] and s["used"] < s["taken"] for s in sets), (name, window, "no window voids calls behind its acceptance")
        if (name, window) == ("plain-4x7", 64):
            assert GW.CHANGED[name].endswith("1") and all(s["accepted"] for s in sets)
        else:
            assert any(not s["accepted"] for s in sets), (name, window, "no clean window")
    assert [s["taken"] for s in GW.consume(name, 1)] == [1] * n
    if GM.CASES[name][5]:  # a window ends in front of the tied slot, which is a launch set of its own
        per = len(GW.slots(name))
        for s in GW.consume(name, 64):
            assert s["taken"] == 1 or (s["first"] % per) + s["taken"] <= per - 1


@pytest.mark.parametrize("window", [2, 3])
def test_plain_4x7_has_a_window_enqueued_ahead_that_is_voided(window):
    """Behind two clean windows the next one is enqueued while its predecessor runs; when the predecessor accepts, the device
    voids it.  So: clean, clean, then an accepting window with calls left behind it."""
    sets = GW.consume("plain-4x7", window)
    acc = [s["accepted"] for s in sets]
    hits = [j for j in range(2, len(sets)) if acc[j - 2:j + 1] == [0, 0, 1] and sets[j]["first"] + sets[j]["taken"] < GW.n_calls("plain-4x7")]
    assert hits, acc


def test_abi_declares_binds_and_exports_guided_run_slots():
    from snesimage_amd import _ffi
    import snesimage_amd
    name = "snesimage_guided_run_slots"
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    lib = _ffi.load()
    assert name + "(" in text and name in {n for n, _, _ in _ffi.SIGNATURES} and getattr(lib, name) is not None
    p, i = C.c_uint32(0), C.c_uint32(0)
    assert lib.snesimage_guided_run_slots(None, 1, 16, C.byref(p), C.byref(i), 0, None, None) == ERR_ARG
    assert callable(snesimage_amd.OptimizedImage.guided_run_slots)
    # the test hook that hands out the shortlists a run scored
    for hook in ("snesimage_debug_guided_capture", "snesimage_debug_guided_shortlists"):
        assert hook + "(" in text and hook in {n for n, _, _ in _ffi.SIGNATURES} and getattr(lib, hook) is not None
    n, k = C.c_uint32(7), C.c_uint32(7)
    assert lib.snesimage_debug_guided_capture(None, 1) == ERR_ARG
    assert lib.snesimage_debug_guided_shortlists(None, None, 0, C.byref(n), C.byref(k)) == ERR_ARG
