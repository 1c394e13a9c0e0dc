"""The model of a set's per-tile dither levels (tests/set_level_model.py) against its own premises, on the CPU.  Every input the
GPU tests use (set_level_model.CASES) is checked here: a full tied sweep holds the gap premise on the summed error at every
comparison, accepts and rejects calls, accepts at least one call that makes a single frame worse, rejects at least one call a
frame alone would have accepted, and moves a tile off the start level — what tells a tied decision from per-frame decisions."""
import numpy as np
import pytest

import set_level_model as SM


def test_total_sums_in_member_order():
    es = [0.1, 0.2, 0.3, 1e-17]
    assert SM.total(es) == ((0.1 + 0.2) + 0.3) + 1e-17 and SM.total([0.25]) == 0.25


@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_inputs_of_the_gpu_tests_tell_tied_from_per_frame(O, name):
    imgs, bank, start, m, tps, pal = SM.case_setup(O, name)
    assert all((f.levels[:m.ntile] == start).all() for f in m.frames)
    assert all(np.array_equal(f.palette, pal) for f in m.frames)
    before = m.error()
    log = m.tied_sweep()  # asserts the gap premise on E at every comparison
    errs = [before] + [e for e, _, _ in log]
    assert all(b <= a for a, b in zip(errs, errs[1:])), "a tied sweep never raises E"
    st = m.stats
    print("%s: %d accepted, %d rejected, %d accepted with a member worse, %d rejected though a member alone accepts, E %.6f -> %.6f, smallest non-zero gap %.2e" % (
        name, st["accepted"], st["rejected"], st["accepted_member_worse"], st["rejected_member_alone"], before, errs[-1], m.min_gap))
    assert st["accepted"] + st["rejected"] == m.ntile == len(log) and st["accepted"] == sum(ch for _, _, ch in log)
    assert st["accepted"] > 0 and st["rejected"] > 0 and m.min_gap > SM.MIN_GAP
    assert st["accepted_member_worse"] > 0 and st["rejected_member_alone"] > 0
    assert any(ch and lv != start for _, lv, ch in log)
    assert errs[-1] == m.error() and errs[-1] < before
    lv = m.levels
    assert all(np.array_equal(lv[0], lv[i]) for i in range(m.F)), "a tied sweep leaves every frame on the same levels"
    m.close()


def test_per_frame_sweep_is_the_single_image_model(O):
    """frame_sweep is level_model.Model.level_sweep frame after frame, and leaves frames on different levels somewhere."""
    name = "set2-row-2x3-L2"
    imgs, bank, start, m, tps, pal = SM.case_setup(O, name)
    logs = m.frame_sweep()
    assert len(logs) == m.F and all(len(l) == m.ntile for l in logs)
    assert m.min_gap > SM.MIN_GAP
    lv = m.levels
    assert (lv[0] != lv[1]).any()
    assert m.error() == SM.total([l[-1][0] for l in logs])
    m.close()


@pytest.mark.parametrize("name", sorted(SM.FLOW_SEED))
def test_flow_of_the_gpu_tests_holds_the_premises(O, name):
    """A tied sweep, then scheduled calls of the set on the T(level) it left (set_level_model.flow): the gap premise holds on the
    summed error at every comparison, and calls behind the sweep change the palette — a slot context still reading the target
    image from in front of the sweep would score against the wrong picture."""
    r = SM.flow(O, name)
    print("%s: sweep %d of %d accepted, calls %s, smallest non-zero gap %.2e" % (name, sum(ch for _, _, ch in r["sweep"]), len(r["sweep"]), [c[2] for c in r["calls"]], r["min_gap"]))
    assert r["min_gap"] > SM.MIN_GAP and sum(c[2] for c in r["calls"]) > 0
    assert any(not np.array_equal(a, b) for a, b in zip(r["maps1"], r["maps2"]))
