"""The premises of tests/test_set_guided.py, proved on the CPU: on every case of set_guided_model.CASES the model's guided calls
hold the gap premise at every comparison, at least one call accepts and one rejects, and on the backdrop case the tied call
accepts; and the set's cost table is the sum of the members' tables."""
import numpy as np
import pytest

import guided_model as GM
import set_backdrop_model as SB
import set_guided_model as SGM


@pytest.mark.parametrize("name", sorted(SGM.CASES))
def test_cases_hold_the_gap_premise_and_accept_and_reject(O, name):
    r = SGM.trajectory(O, name)  # (check_gap asserts inside every call)
    F, H, C, S, flags, B0, K, n = SGM.CASES[name]
    assert len(r["recs"]) == n and r["min_gap"] > SGM.MIN_GAP
    acc = sum(x["changed"] for x in r["recs"])
    print("%s: %d accepted, %d rejected, lowest gap %.1e" % (name, acc, n - acc, r["min_gap"]))
    assert 0 < acc < n
    for x in r["recs"]:
        assert x["cand"].shape == (K, 3) and x["errs"].shape == (K,)
    if B0 is not None:
        last = r["recs"][-1]
        assert last["tied"] and last["changed"] and not np.array_equal(last["B"], B0), "the tied call must accept"
        assert [x["tied"] for x in r["recs"]] == [False] * (n - 1) + [True]


def test_the_set_table_is_the_sum_of_the_members_tables(O):
    rng = np.random.default_rng(0x5E7)
    imgs = SB.frames(3, 16)
    m = SGM.SetModel(O, imgs, 2, 3)
    tiles = []
    for _ in imgs:
        t = np.zeros(1024, np.uint8)
        t[:64] = rng.integers(0, 2, 64)
        tiles.append(t)
    m.set_tiles(tiles)
    for p, i in ((0, 0), (1, 2)):
        want = np.zeros(GM.NCOL, np.uint64)
        for img, t in zip(imgs, tiles):
            want += GM.costs(img, t, m.internal, 2, 3, p, i)
        got = m.costs(p, i)
        assert got.dtype == np.uint64 and np.array_equal(got, want) and got.any()
    m.close()
    b = SGM.SetModel(O, imgs[:2], 2, 3, {}, (31, 31, 31))
    want = np.zeros(GM.NCOL, np.uint64)
    for img, t in zip(b.imgs, b.tiles):
        want += GM.costs(img, t, b.internal, 2, 4, -1, 3)
    assert np.array_equal(b.costs(2, 0), want) and want.any()
    b.close()
