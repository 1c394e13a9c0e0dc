"""The premises of the set's refit tests, checked on the model alone (tests/set_refit_model.py over the CPU oracle; no device):
the states of tests/test_set_refit.py decide what they are meant to decide, so that a later change of an input cannot empty
the GPU tests silently; and the fit of a class whose tiles sit in different members, by hand."""
from types import SimpleNamespace

import numpy as np
import pytest

import character_model as M
import refit_model as R
import set_refit_model as SR

# what the definition gives on the states, recorded from the model: (eligible, spanning members, scored, accepted, accepted spanning,
# accepted with a member's own error rising)
EXPECTED = {"dither_6": (6, 4, 6, 5, 3, 3), "dither_26": (17, 15, 17, 15, 13, 8), "rgb_32": (13, 10, 4, 2, 2, None)}
_SEEN = {}


@pytest.mark.parametrize("state", list(SR.STATES))
def test_states_meet_their_premises(O, state):
    """The gap guard holds at every decision (SetRefit.sweep asserts it); the counts are the recorded ones."""
    imgs, count, size, flags, K, merges, oms, sb = SR.reduced_state(O, state)
    rf = SR.SetRefit(sb)
    snap = rf.snapshot()
    E0 = SR.joint([o.error() for o in oms])
    recs, accepted, U = rf.sweep()
    assert all(r["gap"] is None or r["gap"] == 0.0 or r["gap"] > SR.MIN_GAP for r in recs)
    got = (len(snap), sum(len(c["touched"]) >= 2 for c in snap), sum(r["scored"] for r in recs), accepted,
           sum(r["changed"] and r["touched"] >= 2 for r in recs), sum(r["changed"] and r["member_rose"] for r in recs))
    want = EXPECTED[state]
    assert got[:5] == want[:5] and (want[5] is None or got[5] == want[5]), (state, got)
    assert recs[-1]["error"] == SR.joint([o.error() for o in oms]) and (recs[-1]["error"] < E0) == (accepted > 0)
    assert U <= sb.G and all(r["error"] <= r["before"] for r in recs)
    _SEEN[state] = recs
    for o in oms:
        o.close()


def test_the_states_together_decide_everything(O):
    """Over the three states: an accepted call that spans two members, a scored call that is rejected, a skipped call, and an
    accepted call that raises a member's own error while E falls."""
    for state in SR.STATES:
        if state not in _SEEN:
            imgs, count, size, flags, K, merges, oms, sb = SR.reduced_state(O, state)
            _SEEN[state] = SR.SetRefit(sb).sweep()[0]
            for o in oms:
                o.close()
    recs = [r for state in SR.STATES for r in _SEEN[state]]
    assert any(r["changed"] and r["touched"] >= 2 for r in recs), "no accepted call spans two members"
    assert any(r["scored"] and not r["changed"] for r in recs), "no scored call is rejected"
    assert any(not r["scored"] for r in recs), "no call is skipped"
    assert any(r["changed"] and r["member_rose"] for r in recs), "no accepted call raises a member's own error"
    rgb = _SEEN["rgb_32"]
    assert sum(r["scored"] and not r["changed"] for r in rgb) == 2 and sum(not r["scored"] for r in rgb) == 9


def test_fit_of_a_class_whose_tiles_sit_in_different_members():
    """Two members of two tiles each (ntile = 2): the class is global tiles 1 (member 0, tile 1, subpalette 0) and 2 (member 1,
    tile 0, subpalette 1, drawn under flip 3).  Subpalette 0 = (black, mid grey, white), subpalette 1 = (red, black, black)."""
    pal8 = np.array([[[0, 0, 0], [128, 128, 128], [255, 255, 255]], [[255, 0, 0], [0, 0, 0], [0, 0, 0]]], np.int64)
    orig = np.zeros((4, 64, 3), np.int64)
    orig[0, :] = orig[3, :] = [90, 200, 30]  # tiles outside the class: whatever they hold, the fit does not read them
    orig[1, :32] = [250, 250, 250]           # global tile 1: upper half nearly white, lower half nearly black
    orig[1, 32:] = [5, 5, 5]
    orig[2, :] = [1, 1, 1]                   # global tile 2 (under flip 3): nearly black everywhere ...
    orig[2, 63] = [255, 10, 10]              # ... except its last pixel, which shows position 0 of the representative
    tp = np.array([1, 0, 1, 0])
    tiles, flips = np.array([1, 2]), np.array([0, 3])
    fitted, gain, cost = R.fit_class(orig, pal8, tp, tiles, flips, np.zeros(64, np.int64))
    k = M.red_mean_keys
    c0 = [int(k([250, 250, 250], pal8[0][v]) + k([255, 10, 10], pal8[1][v])) for v in range(3)]
    assert cost[0].tolist() == c0 and fitted[0] == int(np.argmin(c0))
    assert fitted[1:32].tolist() == [2] * 31  # white for member 0's tile, black for member 1's
    c40 = [int(k([5, 5, 5], pal8[0][v]) + k([1, 1, 1], pal8[1][v])) for v in range(3)]
    assert cost[40].tolist() == c40 and fitted[32:].tolist() == [1] * 32  # the lower of the two black entries of subpalette 1
    assert cost[63].tolist() == c40 and R.spread(fitted, 3)[63] == fitted[0]
    assert gain == int((cost[R.Q, 0] - cost.min(axis=1)).sum()) and gain > 0
    other = orig.copy()
    other[0], other[3] = 7, 9
    assert R.fit_class(other, pal8, tp, tiles, flips, np.zeros(64, np.int64))[0].tolist() == fitted.tolist()
    # ... and through SetRefit.snapshot on a stand-in for the SetBudget: the class, its touched members, its fit
    chars = np.zeros((4, 64), np.uint8)
    chars[0], chars[3] = 1, 2
    cur = np.arange(64) % 3
    chars[1] = cur + 1
    chars[2] = M.flip_char(chars[1], 3)
    rep, flip, U, size = M.classes(chars)
    assert rep.tolist() == [0, 1, 1, 3] and flip[2] == 3
    buds = [SimpleNamespace(orig=orig[:2], tp=tp[:2], pal8=pal8), SimpleNamespace(orig=orig[2:], tp=tp[2:], pal8=pal8)]
    sb = SimpleNamespace(buds=buds, G=4, ntile=2, pinned=np.zeros(4, bool), state=lambda: (chars, rep, flip, U, size), values=lambda: chars.astype(np.int64) - 1)
    snap = SR.SetRefit(sb).snapshot()
    assert len(snap) == 1 and snap[0]["rep"] == 1 and snap[0]["touched"] == [0, 1] and snap[0]["tiles"].tolist() == [1, 2]
    assert snap[0]["fitted"].tolist() == fitted.tolist() and snap[0]["cur"].tolist() == cur.tolist()
    assert snap[0]["gain"] == int((cost[R.Q, cur] - cost.min(axis=1)).sum())
    sb.pinned = np.array([False, False, True, False])  # a pinned tile in the OTHER member: the class is not eligible
    assert SR.SetRefit(sb).snapshot() == []
