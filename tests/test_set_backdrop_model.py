"""The model of a backdrop set (tests/set_backdrop_model.py) on the inputs of tests/test_set_backdrop.py: the premises the
GPU comparisons rest on, proved on the CPU."""
import numpy as np
import pytest

import backdrop_model as M
import set_backdrop_model as SM


@pytest.mark.parametrize("name", sorted(SM.TRAJ))
def test_trajectory_inputs_hold_the_gap_premise_and_decide_both_ways(O, name):
    """trajectory() runs with guard=True: every pair of joint errors compared is equal exactly or apart by more than
    MIN_GAP relative (check_gap raises otherwise).  Among the backdrop calls at least one accepts and one rejects."""
    sm, recs, final = SM.traj_run(O, name)
    flags, n, seed, state, B0 = SM.TRAJ[name]
    assert len(recs) == n
    tied = [r for r in recs if r["tied"]]
    assert all(r["p"] == SM.TRAJ_GEOM[0] and r["i"] == 0 for r in tied)
    assert any(r["accepted"] for r in tied), "no backdrop call accepts: choose another seed or start colour"
    assert any(not r["accepted"] for r in tied), "no backdrop call rejects: choose another seed or start colour"
    assert any(r["accepted"] for r in recs if not r["tied"])
    if name == "nes":
        assert np.array_equal(B0, O.nes_color(20)) and tied[0]["changed"]  # a table colour that is not the argmin
    else:
        assert {r["method"] for r in tied} == {0, 1} and len(tied) == 5  # two random sweeps' and the channel sweep's three
    # column S of every member holds B, and every member's map is optimize() of the final palette
    for m in sm.m:
        pal = m.o.palette.reshape(SM.TRAJ_GEOM[0], SM.TRAJ_GEOM[1] + 1, 3)
        assert np.all(pal[:, SM.TRAJ_GEOM[1]] == sm.B) and np.array_equal(m.regular, sm.regular)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("F", [1, 3])
def test_stack_mean_is_the_mean_of_the_concatenated_image(O, F, variant):
    imgs = SM.frames(F, SM.ALPHA_H if variant == 1 else 32, variant)
    if variant == 1:
        assert all((img[..., 3] == 0).any() and (img[..., 3] != 0).any() for img in imgs)  # the transparent square
    want = M.mean_backdrop(np.concatenate(imgs, axis=0))
    assert np.array_equal(SM.stack_backdrop_by_hand(imgs), want)
    assert np.array_equal(SM.stack_backdrop(O, imgs, {}), want)
    nes = SM.stack_backdrop(O, imgs, dict(nes=True))
    assert any(np.array_equal(nes, O.nes_color(k)) for k in range(56))
    blank = [np.zeros_like(img) for img in imgs]
    assert SM.stack_backdrop_by_hand(blank).tolist() == [0, 0, 0] and SM.stack_backdrop(O, blank, {}).tolist() == [0, 0, 0]


def test_set_of_one_model_is_the_single_context_model(O):
    """F = 1: the set model's calls are backdrop_model.Model's, so the GPU's set-of-one comparison has one meaning."""
    img = SM.frames(1, 32)[0]
    sm = SM.SetModel(O, [img], 2, 3, {})
    one = M.Model(O, img, 2, 3, {})
    assert np.array_equal(sm.regular, one.regular) and np.array_equal(sm.B, one.B) and sm.error() == one.error()
    for j, (method, p, i, ch, _) in enumerate(M.model_schedule(O, 2, 3, 8)):
        e, k, rgb, changed, tied = sm.call(method, p, i, ch, 4, j, 16)
        e1, rgb1, changed1 = one.call(method, p, i, ch, 4, j, 16)
        assert e == e1 and np.array_equal(rgb, rgb1) and changed == changed1 and tied == (p == 2)
    assert np.array_equal(sm.m[0].palette_map, one.palette_map)


def test_creation_frames_tell_the_stack_mean_from_a_member_mean(O):
    imgs = SM.creation_frames(3)
    want = SM.stack_backdrop(O, imgs, {})
    assert np.array_equal(want, SM.stack_backdrop_by_hand(imgs))
    assert not any(np.array_equal(M.mean_backdrop(f), want) for f in imgs)
    assert all((f[..., 3] == 0).any() for f in imgs)
