"""The premises of the set's character-budget tests, checked on the model alone (tests/set_character_model.py over the CPU
oracle; no device): the trajectory inputs of tests/test_set_characters.py decide what they are meant to decide, and the
packed key that the product sorts by orders as the tuple of the definition does."""
import json

import numpy as np
import pytest

import character_model as M
import set_character_model as SM


def test_global_key_order_equals_the_tuple_order():
    """cost << 28 | gt << 15 | gb << 2 | f with gt, gb < 8192 and cost <= 64 * 299,505,150 < 2^35: one 64-bit key."""
    worst = 64 * int(M.red_mean_keys([255, 0, 255], [0, 255, 0]))
    assert worst == 64 * 299505150 and worst < 1 << 35
    rng = np.random.default_rng(4)
    tup = [(int(rng.integers(0, 3)) * int(rng.integers(0, worst + 1)), int(rng.integers(8192)), int(rng.integers(8192)), int(rng.integers(4))) for _ in range(4000)]
    tup += [(worst, 8191, 8191, 3), (0, 0, 0, 0), (5, 8191, 0, 0), (5, 0, 8191, 3), (6, 0, 0, 0)]
    keys = [(c << 28) | (t << 15) | (b << 2) | f for c, t, b, f in tup]
    assert max(keys) < (1 << 64) - 1  # below "no candidate"
    assert [t for _, t in sorted(zip(keys, tup))] == sorted(tup) and len(set(keys)) == len(set(tup))


def test_classes_across_members_count_a_shared_character_once():
    rng = np.random.default_rng(5)
    a, b = rng.integers(1, 4, 64).astype(np.uint8), rng.integers(1, 4, 64).astype(np.uint8)
    zero = np.zeros(64, np.uint8)
    member0 = np.stack([a, b, zero, M.flip_char(a, 1)])
    member1 = np.stack([M.flip_char(b, 3), zero, M.flip_char(a, 2), a])
    rep, flip, U, size = M.classes(np.concatenate([member0, member1]))
    assert rep.tolist() == [0, 1, 2, 0, 1, 2, 0, 0] and flip.tolist() == [0, 0, 0, 1, 3, 0, 2, 0]
    assert U == 3 and U < M.classes(member0)[2] + M.classes(member1)[2]


@pytest.mark.parametrize("name", list(SM.TRAJECTORIES))
def test_trajectory_inputs_meet_their_premises(O, name):
    """The gap guard holds at every decision (SetBudget.step asserts it); a winner with rank > 0; a step that raises E; a merge
    whose donor sits in another member; a winner that is not the candidate with the lowest member error."""
    imgs, count, size, flags, K, steps = SM.trajectory_inputs(name)
    tps, pal = SM.stack_start(O, imgs, count, size, **flags)
    oms = SM.oracle_members(O, imgs, tps, pal, count, size, **flags)
    sb = SM.SetBudget(O, oms, imgs)
    U0 = sb.state()[3]
    recs, U = sb.reduce(U0 - steps, K)
    assert len(recs) == steps and U == U0 - steps
    SM.assert_trajectory_decides(recs)
    E = 0.0
    for i, o in enumerate(oms):
        E = o.error() if i == 0 else E + o.error()
    assert recs[-1]["error"] == E
    tiles = [t for o in oms for t in json.loads(o.as_json())["tiles"]]
    assert M.count_unique(tiles) == U
    for o in oms:
        o.close()
