"""The model of guided calls (tests/guided_model.py) against the oracle's own key and against its premises, on the CPU.  Every
input the GPU tests' trajectories use (guided_model.CASES) is checked here: the guided calls hold the gap premise at every
comparison and accept and reject at least one call."""
import numpy as np
import pytest

import guided_model as GM


def test_red_mean_key_equals_the_oracles(O):
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 256, (500, 3)), rng.integers(0, 256, (500, 3))
    a[:4], b[:4] = [[0, 0, 0], [255, 255, 255], [255, 0, 255], [0, 255, 0]], [[255, 255, 255], [0, 0, 0], [0, 255, 0], [255, 0, 255]]
    keys = GM.red_mean_key(a, b)
    assert keys.max() <= 299505150
    for x, y, k in zip(a, b, keys):
        assert int(k) == O.red_mean_key(x, y)


def test_costs_follow_the_definition_pixel_by_pixel(O):
    """The vectorised table against the definition spelt out, on a few colours of one slot: a sum over the subpalette's opaque
    pixels of min(floor, key), the floor over the other entries."""
    img = GM.image(8, 3)
    img[2:6, 40:90, 3] = 0
    m = GM.Model(O, img, 2, 3)
    cost = m.costs(1, 2)
    tp, pal8 = m.tile_palettes, GM.expand5(m.internal).reshape(2, 3, 3)
    rng = np.random.default_rng(1)
    for u in [0, 32767, int(GM.pack_u(m.internal[5]))] + [int(v) for v in rng.integers(0, 32768, 5)]:
        c8 = GM.expand5(GM.unpack_u(u))
        total = 0
        for y in range(8):
            for x in range(256):
                if img[y, x, 3] == 0 or tp[x // 8] != 1:
                    continue
                floor = min(int(GM.red_mean_key(img[y, x, :3], pal8[1, j])) for j in (0, 1))
                total += min(floor, int(GM.red_mean_key(img[y, x, :3], c8)))
        assert int(cost[u]) == total, u
    m.close()


def test_shortlist_orders_by_cost_then_colour_and_leaves_the_current_colour_out():
    cost = np.full(GM.NCOL, 9, np.uint64)
    cost[[5, 70, 3]] = [1, 1, 0]
    rgb5, c = GM.shortlist(cost, GM.unpack_u(5), 4)
    assert [int(v) for v in GM.pack_u(rgb5)] == [3, 70, 0, 1] and [int(v) for v in c] == [0, 1, 9, 9]
    assert GM.shortlist(cost, GM.unpack_u(5))[0].shape == (16, 3)


def test_one_entry_subpalettes_have_no_floor(O):
    img = GM.image(8, 4)
    m = GM.Model(O, img, 1, 2)
    two = m.costs(0, 0)
    one = GM.costs(m.T, m.tile_palettes, m.internal[:1], 1, 1, 0, 0)
    assert (one >= two).all() and int(one[0]) == int(GM.red_mean_key(img[..., :3].reshape(-1, 3), [0, 0, 0]).sum())
    m.close()


@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_inputs_of_the_gpu_tests_hold_the_premises(O, name):
    r = GM.trajectory(O, name)  # asserts the gap premise at every comparison
    recs = r["recs"]
    accepted = sum(c["changed"] for c in recs)
    errs = [r["err0"]] + [c["error"] for c in recs]
    print("%s: %d calls, %d accepted, error %.6f -> %.6f, smallest non-zero gap %.2e" % (name, len(recs), accepted, errs[0], errs[-1], r["min_gap"]))
    assert 0 < accepted < len(recs) and r["min_gap"] > GM.MIN_GAP
    assert all(b <= a for a, b in zip(errs, errs[1:])), "a guided call never raises the error"
    for j, c in enumerate(recs):
        # the best candidate against the incumbent and the runner-up: equal, or further apart than any rounding the GPU tests allow
        e = np.sort(np.append(c["errs"], errs[j]))
        for other in e[1:3]:
            gap = abs(other - e[0]) / e[0]
            assert gap == 0.0 or gap > GM.MIN_GAP, (name, c["p"], c["i"], gap)
        assert not any(np.array_equal(x, c["rgb5"]) for x in c["cand"]) or c["changed"]
    if r["backdrop"]:
        assert (recs[-1]["p"], recs[-1]["i"]) == (r["C"], 0) and (recs[-1]["pmap"] == r["S"]).any(), "the tied slot is called and pixels show the backdrop"
