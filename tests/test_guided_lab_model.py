"""The model of the CIELAB proxy (tests/guided_lab_model.py) against the definition spelt out and against its premises, on the
CPU.  Every picture and slot the GPU tests compare (guided_lab_model.TABLE_CASES, CASES, SET_CASES, the CLI's run) is checked
here: its CIELAB shortlist differs from the redmean shortlist of guided_model, and every trajectory holds the gap premise of
tests/test_guided_model.py at every comparison and both accepts and rejects calls."""
import numpy as np
import pytest

import guided_lab_model as LM
import guided_model as GM


def test_q_on_hand_values():
    f = np.float32
    assert [int(v) for v in LM.q([0.0, 1.0, 0.5, 2.0 ** -16, 2.0 ** -17, 1.0 + 2.0 ** -16, 3.75])] == [0, 65536, 32768, 1, 0, 65537, 245760]
    assert int(LM.q(f(256.0 - 2.0 ** -15))) == 16777214 and int(LM.q(f(256.0 - 2.0 ** -16))) == 0xFFFFFF and int(LM.q(f(256.0))) == 0xFFFFFF and int(LM.q(f(300.5))) == 0xFFFFFF and int(LM.q(f(65535.0))) == 0xFFFFFF
    d = f(12.3456789)
    assert int(LM.q(d)) == int(float(d) * 65536.0), "the product by 2^16 is exact in f32: the truncation is the real number's"
    v = np.sort(np.random.default_rng(3).random(1000).astype(f) * f(120))
    assert (np.diff(LM.q(v).astype(np.int64)) >= 0).all(), "q is monotone"
    assert int(np.minimum(LM.q(v[17]), LM.q(v[400]))) == int(LM.q(min(v[17], v[400])))


def test_the_pictures_carry_few_colours_none_of_them_a_bgr555_colour():
    expansions = set(int(v) for v in GM.expand5(np.arange(32)))
    for name in LM.TABLE_CASES:
        h, seed, C, S, flags, backdrop, table, hole, first, slots = LM.TABLE_CASES[name]
        img = LM.image(h, seed, two=table is not None)
        col = np.unique(img[..., :3].reshape(-1, 3), axis=0)
        assert 2 <= len(col) <= (2 if table is not None else 16), (name, len(col))
        assert not any(all(int(v) in expansions for v in c) for c in col), name
    for f in LM.frames(3, 8):
        assert len(np.unique(f[..., :3].reshape(-1, 3), axis=0)) <= 16


def test_costs_follow_the_definition_pixel_by_pixel(O):
    """The table against the definition spelt out in a triple loop (tiles, pixels, entries) on an 8-tile population, on a few
    colours: every distance straight from the oracle, nothing cached, Python integers."""
    img = LM.image(8, 3)
    img[2:6, 20:50, 3] = 0
    m = LM.Model(O, img, 2, 4, dict(perceptual=True))
    tp = np.ones(1024, np.uint8)
    tp[2:10] = 0  # tiles 2 .. 9: the population of subpalette 0
    m.set_tile_palettes(tp)
    cost = m.costs(0, 2)
    pal8 = GM.expand5(m.internal).reshape(2, 4, 3).astype(np.uint8)

    def q1(d):
        return min(int(np.float32(d) * np.float32(65536.0)), 0xFFFFFF)

    rng = np.random.default_rng(1)
    for u in [0, 32767, int(GM.pack_u(m.internal[2]))] + [int(v) for v in rng.integers(0, 32768, 5)]:
        c8 = GM.expand5(GM.unpack_u(u)).astype(np.uint8)
        total = 0
        for t in range(2, 10):
            for k in range(64):
                y, x = k // 8, 8 * t + k % 8
                if img[y, x, 3] == 0:
                    continue
                floor = 0xFFFFFFFF
                for j in (0, 1, 3):
                    floor = min(floor, q1(O.distance_cielab(pal8[0, j], img[y, x, :3])))
                total += min(floor, q1(O.distance_cielab(c8, img[y, x, :3])))
        assert int(cost[u]) == total, u
    assert int(cost.max()) < 8 * 64 * 2 ** 24
    m.close()


def test_one_entry_subpalettes_have_no_floor(O):
    img, tp, pal = LM.no_floor_case()
    for p, n in ((0, 20), (1, 12)):
        cost = LM.costs(O, img, tp, pal, 2, 1, p, 0)
        px = img[:, 8 * (0 if p == 0 else 20):8 * (20 if p == 0 else 32), :3].reshape(-1, 3)
        assert len(px) == 64 * n
        for u in (0, 12345, 32767):
            assert int(cost[u]) == sum(int(LM.q(LM.distances(O, c)[u])) for c in px)  # the plain sum of q(d)
        cur = pal[p]
        assert not np.array_equal(GM.shortlist(cost, cur, 16)[0], GM.shortlist(GM.costs(img, tp, pal, 2, 1, p, 0), cur, 16)[0])


@pytest.mark.parametrize("name", sorted(LM.TABLE_CASES))
def test_the_shortlists_of_the_gpu_tests_differ_from_redmean(O, name):
    m = LM.table_model(O, name)
    for p, i in LM.TABLE_CASES[name][-1]:
        cur = m.internal[m.entries(p, i)[0][0]]
        lab, red = m.costs(p, i), m.redmean_costs(p, i)
        assert lab.any() and int(lab.max()) < 2 ** 43
        for K in (16, 64):
            assert not np.array_equal(GM.shortlist(lab, cur, K)[0], GM.shortlist(red, cur, K)[0]), (name, p, i, K)
    m.close()


def check_trajectory(name, r):
    recs = r["recs"]
    accepted = sum(c["changed"] for c in recs)
    errs = [r["err0"]] + [c["error"] for c in recs]
    print("%s: %d calls, %d accepted, error %.6f -> %.6f, smallest non-zero gap %.2e" % (name, len(recs), accepted, errs[0], errs[-1], r["min_gap"]))
    assert 0 < accepted < len(recs) and r["min_gap"] > GM.MIN_GAP
    assert all(b <= a for a, b in zip(errs, errs[1:])), "a guided call never raises the error"
    for j, c in enumerate(recs):
        e = np.sort(np.append(c["errs"], errs[j]))
        for other in e[1:3]:
            gap = abs(other - e[0]) / e[0]
            assert gap == 0.0 or gap > GM.MIN_GAP, (name, c["p"], c["i"], gap)
        assert not np.array_equal(c["cand"], c["red"]), "%s call %d: the CIELAB shortlist is the redmean one: the GPU test shows nothing" % (name, j)


@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_inputs_of_the_gpu_tests_hold_the_premises(O, name):
    check_trajectory(name, LM.trajectory(O, name))  # (the model asserts the gap premise at every comparison)


@pytest.mark.parametrize("name", sorted(LM.SET_CASES))
def test_inputs_of_the_set_tests_hold_the_premises(O, name):
    r = LM.set_trajectory(O, name)
    check_trajectory(name, r)
    if r["backdrop"]:
        assert recs_end_on_the_tied_slot(r)


def recs_end_on_the_tied_slot(r):
    last = r["recs"][-1]
    return (last["p"], last["i"]) == (r["C"], 0) and last["tied"]


def test_the_cli_run_holds_the_premises(O):
    r = LM.cli_trajectory(O)  # (every scheduled and guided call asserts the gap premise)
    accepted = sum(c["changed"] for c in r["sweep"])
    print("cli: %d calls, guided sweep %d of %d accepted, smallest non-zero gap %.2e" % (r["calls"], accepted, len(r["sweep"]), r["min_gap"]))
    assert 0 < accepted < len(r["sweep"]) and r["min_gap"] > GM.MIN_GAP
