"""The recorded decisions of tests/set_guided_window_model.py against the model, the premises the GPU tests of a set's guided
windows rest on, the identity their generator rests on, and the ABI of snesimage_shared_guided_run_slots — all on the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import set_guided_model as SGM
import set_guided_window_model as SGW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_recorded_decisions_are_the_models(O, name):
    recs, min_gap = SGW.run(O, name)  # asserts the gap premise at every comparison
    sl = SGW.slots(name)
    changed = "".join(str(r["changed"]) for r in recs)
    print("%s: %d calls, smallest non-zero gap %.2e, changed %s" % (name, len(recs), min_gap, changed))
    assert len(recs) == SGW.n_calls(name) == len(SGW.CHANGED[name]) and min_gap > SGM.MIN_GAP
    assert [(r["p"], r["i"]) for r in recs] == [sl[j % len(sl)] for j in range(len(recs))]
    assert changed == SGW.CHANGED[name]
    assert "0" in changed and "1" in changed, "the case does not both accept and reject"
    # the trajectory the GPU tests of the single calls follow is the head of this one
    for a, b in zip(SGM.trajectory(O, name)["recs"], recs):
        assert (a["p"], a["i"], a["best_k"], a["changed"]) == (b["p"], b["i"], b["best_k"], b["changed"]) and a["error"] == b["error"]


@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_windows_over_the_recorded_decisions_void_calls_and_come_back_clean(name):
    """One combination cannot hold the second premise: the backdrop case never rejects three calls in a row in front of its tied
    slot, so at window 3 every window accepts.  That is asserted as it is; the case has clean windows at 2, the other five cases
    at 2 and at 3."""
    n = SGW.n_calls(name)
    for window in (2, 3):
        sets = SGW.consume(name, window)
        assert sum(s["used"] for s in sets) == n and all(1 <= s["used"] <= s["taken"] <= window for s in sets)
        assert any(s["accepted"] and s["used"] < s["taken"] for s in sets), (name, window, "no window voids calls behind its acceptance")
        if (name, window) == ("backdrop-f2-2x3", 3):
            assert all(s["accepted"] for s in sets)
        else:
            assert any(not s["accepted"] and s["taken"] == window for s in sets), (name, window, "no clean window")
    assert [s["taken"] for s in SGW.consume(name, 1)] == [1] * n
    assert all(s["taken"] <= SGW.kmax(name) for s in SGW.consume(name, 64))
    if SGM.CASES[name][5] is not None:  # a window ends in front of the tied slot, which is a launch set of its own
        per = len(SGW.slots(name))
        for s in SGW.consume(name, 64):
            assert s["taken"] == 1 or (s["first"] % per) + s["taken"] <= per - 1


def test_a_window_holds_the_same_slot_twice():
    """The 2 x 3 plain cases have six slots and windows of up to 64 / F calls: the slot order wraps inside one window, in windows
    that void calls in all four, and in a clean window, all of whose calls take effect, in two."""
    for name in ("plain-f2-2x3", "plain-f3-2x3", "perceptual-f2-2x3", "dither-f2-2x3"):
        per = len(SGW.slots(name))
        sets = SGW.consume(name, 64)
        assert any(s["taken"] > per and s["accepted"] for s in sets), name
        if name in ("plain-f2-2x3", "perceptual-f2-2x3"):
            assert any(s["used"] > per and not s["accepted"] for s in sets), (name, "no clean window wraps the slot order")


@pytest.mark.parametrize("name", ["plain-f2-2x3", "backdrop-f2-2x3", "backdrop-mean-f2-2x3"])
def test_one_table_per_subpalette_plus_one_correction_per_call_is_the_cost_table(O, name):
    """cost_{p,i} = A_p + D_{p,i} for every regular slot, all 32,768 colours, against set_guided_model.set_costs, on two cases and
    on a backdrop set whose B, the stack's mean, is one of the entries the floor runs over AND some pixels' nearest entry."""
    if name == "backdrop-mean-f2-2x3":
        import set_backdrop_model as SB
        imgs = SB.frames(2, 16)
        m = SGM.SetModel(O, imgs, 2, 3, {}, SB.stack_backdrop(O, imgs, {}))
    else:
        m = SGM.case_model(O, name)
    nearest_b = 0
    for p in range(m.C):
        A, D = SGW.window_costs(m.imgs, m.tiles, m.internal, m.Si, p)
        assert A.any()
        for i in range(m.S):
            want = SGM.set_costs(m.imgs, m.tiles, m.internal, m.C, m.Si, p, i)
            assert np.array_equal(A + D[i], want), (name, p, i)
        if m.backdrop:
            nearest_b += int(D[m.S].any())
    assert name != "backdrop-mean-f2-2x3" or nearest_b > 0, "B is nearest to no pixel: the case does not show that B can be j*"
    m.close()


def test_the_identity_holds_with_equal_entries_and_one_entry():
    """Two equal entries in a subpalette (a == b for their pixels, whichever is called j*), and a one-entry subpalette (b is
    0xFFFFFFFF: A + D is the plain sum of keys)."""
    import set_backdrop_model as SB
    imgs = SB.frames(2, 8)
    tiles = [np.array([(k + f) % 2 for k in range(32)] + [0] * 992, np.uint8) for f in range(2)]
    pal = np.array([[10, 12, 7], [3, 20, 25], [10, 12, 7], [31, 31, 0], [3, 20, 25], [3, 20, 25]], np.uint8)
    for p in range(2):
        A, D = SGW.window_costs(imgs, tiles, pal, 3, p)
        for i in range(3):
            assert np.array_equal(A + D[i], SGM.set_costs(imgs, tiles, pal, 2, 3, p, i)), (p, i)
    assert not D[1].any() and not D[2].any()  # subpalette 1 holds one colour three times: entry 0 is every pixel's j*, and a == b
    one = np.array([[10, 12, 7], [3, 20, 25]], np.uint8)
    for p in range(2):
        A, D = SGW.window_costs(imgs, tiles, one, 1, p)
        assert np.array_equal(A + D[0], SGM.set_costs(imgs, tiles, one, 2, 1, p, 0)), p


def test_abi_declares_binds_and_exports_the_entry_point_and_its_hooks():
    from snesimage_amd import _ffi
    import snesimage_amd
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snesimage_hip.h")).read(), flags=re.S)
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in ("snesimage_shared_guided_run_slots", "snesimage_shared_debug_guided_capture", "snesimage_shared_debug_guided_shortlists", "snesimage_shared_debug_guided_window_costs"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound and getattr(lib, name) is not None
    p, i, n, k = C.c_uint32(0), C.c_uint32(0), C.c_uint32(7), C.c_uint32(7)
    assert lib.snesimage_shared_guided_run_slots(None, 1, 16, C.byref(p), C.byref(i), 0, None, None) == ERR_ARG
    assert lib.snesimage_shared_debug_guided_capture(None, 1) == ERR_ARG
    assert lib.snesimage_shared_debug_guided_shortlists(None, None, 0, C.byref(n), C.byref(k)) == ERR_ARG
    assert lib.snesimage_shared_debug_guided_window_costs(None, C.byref(p), C.byref(i), 1, None) == ERR_ARG
    for method in ("guided_run_slots", "debug_guided_capture", "debug_guided_shortlists", "debug_guided_window_costs"):
        assert callable(getattr(snesimage_amd.SharedPalette, method))


def test_cli_takes_a_window_for_the_guided_sweeps_of_a_set(tmp_path):
    """--share refuses --window above 1 on its own (the scheduled windows of a set are sized by the library) and takes it with
    --set-guided; said while parsing: the sources do not exist."""
    import subprocess
    cli = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
    missing, out = str(tmp_path / "none.png"), str(tmp_path / "o.json")
    share = ["--share", "%s=%s" % (missing, str(tmp_path / "s.json"))]
    r = subprocess.run([cli, missing, out, *share, "--window", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--window" in r.stderr
    r = subprocess.run([cli, missing, out, *share, "--window", "3", "--set-guided", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot be used with" not in r.stderr, r.stderr  # past the argument rules: the source is missing
    assert not os.path.exists(out)
