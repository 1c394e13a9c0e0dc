"""The model of per-tile ordered-dither levels (tests/level_model.py) against the model of one table (tests/ordered_model.py)
and against its own premises, on the CPU.  Every input the GPU tests use (level_model.CASES) is checked here: the sweep holds
the gap premise at every comparison, accepts and rejects at least one call, and moves at least one tile off the start level."""
import numpy as np
import pytest

import level_model as LM
import ordered_model as OM


def test_ladder_follows_the_formula():
    b = LM.ladder(4, 32, 4)
    assert b.shape == (4, 4, 4) and not b[0].any()
    for j, a in enumerate((0, 10, 21, 32)):
        if j:
            assert np.array_equal(b[j], OM.bayer(4, a))
    assert np.array_equal(LM.ladder(8, 7, 8)[1], OM.bayer(8, 1))


def test_one_table_reproduces_the_ordered_model(O):
    img = LM.with_hole(LM.image(24, 3))
    table = OM.bayer(16, 96)
    assert np.array_equal(LM.target_image(img, table[None], np.zeros(1024, np.uint8)), OM.target_image(img, table))
    m = LM.Model(O, img, 2, 3, {}, table[None])
    one = OM.Model(O, img, 2, 3, {}, table)
    m.kmeans_start()
    one.kmeans_start()
    assert np.array_equal(m.T, one.T) and np.array_equal(m.palette_map, one.palette_map) and m.error() == one.error()
    log = m.level_sweep(0, 8)
    assert [(lv, ch) for _, lv, ch in log] == [(0, 0)] * 8 and all(e == one.error() for e, _, _ in log)


def test_target_image_takes_each_tile_from_its_level():
    img = LM.image(24, 1)
    bank = LM.ladder(16, 64, 4)
    rng = np.random.default_rng(3)
    levels = rng.integers(0, 4, 1024).astype(np.uint8)
    T = LM.target_image(img, bank, levels)
    assert np.array_equal(T[..., 3], img[..., 3])
    for t in (0, 31, 32, 64 + 17, 95):
        y, x = 8 * (t // 32), 8 * (t % 32)
        assert np.array_equal(T[y:y + 8, x:x + 8], OM.target_image(img, bank[levels[t]])[y:y + 8, x:x + 8])
    # rows 16..23 of a 16 x 16 table's second period start: the phase is the picture's, not the tile's
    assert np.array_equal(T[16:24, :8], OM.target_image(img, bank[levels[64]])[16:24, :8])


def test_composed_map_is_optimize_against_the_composed_target(O):
    """The premise of the tile-wise composition: without error diffusion a pixel's choice depends on T at that pixel alone."""
    img = LM.with_hole(LM.image(24, 2))
    m = LM.Model(O, img, 2, 3, dict(perceptual=True), LM.ladder(8, 48, 4), 3)
    m.kmeans_start()
    rng = np.random.default_rng(5)
    m.set_levels(rng.integers(0, 4, 1024))
    s = m.slot_model()
    assert np.array_equal(s.palette_map, m.palette_map) and s.error() == m.error()
    e, cm = m.candidate(40, (int(m.levels[40]) + 1) % 4)
    lv = m.levels.copy()
    lv[40] = (int(lv[40]) + 1) % 4
    m.set_levels(lv)
    assert np.array_equal(m.palette_map, cm) and m.error() == e


@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_inputs_of_the_gpu_tests_hold_the_premises(O, name):
    img, bank, start, m, B = LM.case_setup(O, name)
    assert (m.levels[:m.ntile] == start).all()
    before = m.error()
    log = m.level_sweep()  # asserts the gap premise at every comparison
    errs = [before] + [e for e, _, _ in log]
    assert all(b <= a for a, b in zip(errs, errs[1:])), "a sweep never raises the error"
    accepted = sum(ch for _, _, ch in log)
    print("%s: %d calls, %d accepted, error %.6f -> %.6f, smallest non-zero gap %.2e" % (name, len(log), accepted, before, errs[-1], m.min_gap))
    assert 0 < accepted < len(log) and m.min_gap > LM.MIN_GAP
    assert any(ch and lv != start for _, lv, ch in log)
    assert errs[-1] == m.error() and errs[-1] < before
    if B is not None:
        assert (m.palette_map == m.S - 1).any(), "no pixel shows the backdrop: the case shows nothing"
    m.close()


@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_flow_of_the_gpu_tests_holds_the_premises(O, name):
    """Calls, a sweep, calls (level_model.flow): the sweep behind two optimizer calls still accepts and rejects, and calls on both
    sides of it change the palette — so a pack or a contested list left over from in front of the sweep would be a wrong one."""
    r = LM.flow(O, name)
    accepted = sum(ch for _, _, ch in r["sweep"])
    print("%s: pre %s, sweep %d of %d accepted, post %s, smallest non-zero gap %.2e" % (name, [c[2] for c in r["pre"]], accepted, len(r["sweep"]), [c[2] for c in r["post"]], r["min_gap"]))
    assert 0 < accepted < len(r["sweep"]) and r["min_gap"] > LM.MIN_GAP
    assert sum(c[2] for c in r["pre"]) > 0 and sum(c[2] for c in r["post"]) > 0
