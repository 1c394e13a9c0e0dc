"""Duplicate colours of a candidate list are scored once: the lowest index that carries a colour is scored, every
other holder of it takes that candidate's error, and the table that says who holds what is left clear for the next call.

Nothing a caller sees may move: every comparison here is `np.array_equal` / `==` against a context created with
SNES_DEDUP=0 (the path as it was), and for one case of every test family against the dense path (SNES_SPARSE=0) as well.

Which lists take which path in this file: on a default context every list scored here takes the new path except one, the
1,000-candidate list of test_a_list_below_the_threshold (all other lists hold 1,500 to 4,096 candidates; the same 1,000-candidate
list is also put through the new path by a context with SNES_DEDUP_MIN=1).  The library cannot be asked which path a list took,
so that case pins the short list's *result* (default == SNES_DEDUP=0 == forced on == dense), not its launches.  The reference
contexts (SNES_DEDUP=0, SNES_SPARSE=0) take the old paths by construction.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAGS = [{}, {"perceptual": True}]
FLAG_IDS = ["rgb", "perceptual"]


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


@pytest.fixture(scope="module")
def start(S, img256_alpha):
    """The k-means start of the test image, computed once per distance: (tile_palettes, palette)."""
    out = {}
    for perceptual in (False, True):
        g = S.OptimizedImage(img256_alpha, 8, 15, perceptual=perceptual)
        g.initialize_tiles()
        g.recalculate_palettes()
        out[perceptual] = (g.tile_palettes, g.palette)
        g.close()
    return out


def context(S, img, start, monkeypatch, env=None, chunk=0, **flags):
    """A context at the k-means start, created with `env` in the environment (the library reads its switches at creation)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    g = S.OptimizedImage(img, 8, 15, **flags)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if chunk:
        g.set_chunk(chunk)
    g.tile_palettes, g.palette = start[bool(flags.get("perceptual"))]
    g.optimize()
    return g


def list_with_repeats(rng, n, n_colours, must_hold):
    """n candidates drawn from n_colours distinct colours (`must_hold` among them), every colour at least once, shuffled."""
    colours = {tuple(int(v) for v in c) for c in must_hold}
    while len(colours) < n_colours:
        colours.add(tuple(int(v) for v in rng.integers(0, 32, 3)))
    colours = np.array(sorted(colours), np.uint8)
    rng.shuffle(colours)
    pick = np.concatenate([np.arange(n_colours), rng.integers(0, n_colours, n - n_colours)])
    rng.shuffle(pick)
    return colours[pick]


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("chunk", [0, 1024], ids=["one-launch-group-per-lane", "groups-of-1024"])
def test_list_of_300_colours_4096_long(S, img256_alpha, start, flags, chunk, monkeypatch):
    """4,096 candidates from 300 colours in shuffled order, the slot's own colour among them, on two slots.  With launch
    groups of 1,024 the holders of one colour fall into different groups and lanes (a group may then scan before an earlier
    group has marked its candidates: the copy at the end settles it).  Raw bytes of 32 and more wrap in the 8-bit expansion
    (33 expands like 2, 40 like 9): such a candidate is the same image as its wrapped twin and must come out with the same error."""
    new = context(S, img256_alpha, start, monkeypatch, chunk=chunk, **flags)
    old = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP": "0"}, chunk=chunk, **flags)
    dense = context(S, img256_alpha, start, monkeypatch, {"SNES_SPARSE": "0"}, **flags) if not chunk else None
    pal = start[bool(flags.get("perceptual"))][1]
    rng = np.random.default_rng(300)
    for sp, si in ((2, 3), (6, 11)):
        cand = list_with_repeats(rng, 4096, 300, [pal[sp * 15 + si], (2, 9, 30)])
        cand[7], cand[4000], cand[2222] = (33, 9, 30), (2, 40, 30), (63, 63, 63)  # wrapped twins of (2, 9, 30); a colour no triple below 32 expands to
        assert len({tuple(c) for c in cand}) <= 303
        e_new = new.score_candidates(sp, si, cand)
        e_old = old.score_candidates(sp, si, cand)
        assert np.array_equal(e_new, e_old), ((sp, si), int(np.sum(e_new != e_old)))
        twins = [k for k in range(4096) if tuple(cand[k]) in ((2, 9, 30), (33, 9, 30), (2, 40, 30))]
        assert len(twins) >= 3 and len({e_new[k] for k in twins}) == 1
        if dense is not None:
            assert np.array_equal(e_new, dense.score_candidates(sp, si, cand)), (sp, si)
    for g in (new, old, dense):
        if g is not None:
            g.close()


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_one_colour_only_and_no_repeats_at_all(S, img256_alpha, start, flags, monkeypatch):
    """The two ends: 2,048 times one colour (one candidate scored, 2,047 copies) and 2,048 distinct colours (nothing to copy)."""
    new = context(S, img256_alpha, start, monkeypatch, **flags)
    old = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP": "0"}, **flags)
    dense = context(S, img256_alpha, start, monkeypatch, {"SNES_SPARSE": "0"}, **flags)
    same = np.tile(np.array([[9, 20, 5]], np.uint8), (2048, 1))
    keys = np.random.default_rng(7).permutation(32768)[:2048]
    distinct = np.stack([keys & 31, (keys >> 5) & 31, (keys >> 10) & 31], axis=1).astype(np.uint8)
    for cand in (same, distinct):
        e_new = new.score_candidates(1, 4, cand)
        assert np.array_equal(e_new, old.score_candidates(1, 4, cand))
        assert np.array_equal(e_new, dense.score_candidates(1, 4, cand))
    assert len(set(new.score_candidates(5, 0, same).tolist())) == 1
    for g in (new, old, dense):
        g.close()


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_twenty_random_calls_from_the_kmeans_start(S, img256_alpha, start, flags, monkeypatch):
    """The optimizer's own lists (about 245 repeats in 4,096): error, colour, best_k — the LOWEST index of the winning colour,
    as the commit's ascending scan with a strict `<` picks it —, palette and palette_map after every call."""
    new = context(S, img256_alpha, start, monkeypatch, **flags)
    old = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP": "0"}, **flags)
    repeats = 0
    for i, (_, p, idx, ch, _) in enumerate(S.schedule(8, 15, 20)):
        cand = S.random_candidates(3, 50 + i, 4096)
        repeats += 4096 - len({tuple(c) for c in cand})
        for g in (new, old):
            g.step_async(S.METHOD_RANDOM, p, idx, ch, 3, 50 + i, 4096)
        (e_n, b_n, k_n), (e_o, b_o, k_o) = new.last_step(), old.last_step()
        assert e_n == e_o and np.array_equal(b_n, b_o) and k_n == k_o, (i, e_n, e_o, k_n, k_o)
        assert np.array_equal(new.palette, old.palette) and np.array_equal(new.palette_map, old.palette_map), i
    assert repeats > 20 * 150  # (the lists did hold what this test is about)
    new.close()
    old.close()


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_two_shards_each_with_its_own_list(S, img256_alpha, start, flags, monkeypatch):
    """step_begin with shard_count 2: every shard removes the repeats of its OWN list (candidates r, r + 2, ...), writes its
    errors with stride 2 into a vector preset to +inf; the element-wise minimum — what the all-reduce forms — equals the
    unsharded call's vector, and the commit of it leaves both shards in the unsharded call's state."""
    from hipmem import DeviceArray
    n = 4096
    ref = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP": "0"}, **flags)
    whole = context(S, img256_alpha, start, monkeypatch, **flags)
    shards = [context(S, img256_alpha, start, monkeypatch, **flags) for _ in range(2)]
    for i, (p, idx) in enumerate([(0, 0), (3, 7), (0, 0)]):
        v_ref, v_whole = DeviceArray(n, np.float64, fill=0), DeviceArray(n, np.float64, fill=0)
        ref.step_begin(S.METHOD_RANDOM, p, idx, 0, 4, 70 + i, n, 0, 1, v_ref.ptr)
        whole.step_begin(S.METHOD_RANDOM, p, idx, 0, 4, 70 + i, n, 0, 1, v_whole.ptr)
        ref.sync()
        whole.sync()
        e_ref = v_ref.numpy()
        assert np.array_equal(v_whole.numpy(), e_ref)
        bufs = [DeviceArray(n, np.float64, fill=0) for _ in range(2)]
        for r, s in enumerate(shards):
            s.step_begin(S.METHOD_RANDOM, p, idx, 0, 4, 70 + i, n, r, 2, bufs[r].ptr)
            s.sync()
        h0, h1 = bufs[0].numpy(), bufs[1].numpy()
        assert np.isinf(h0[1::2]).all() and np.isinf(h1[0::2]).all()
        red_np = np.minimum(h0, h1)
        assert np.array_equal(red_np, e_ref), (i, int(np.sum(red_np != e_ref)))
        red = DeviceArray.from_numpy(red_np)
        ref.step_commit(v_ref.ptr)
        whole.step_commit(v_whole.ptr)
        want = ref.last_step()
        for s in shards + [whole]:
            if s is not whole:
                s.step_commit(red.ptr)
            e, b, k = s.last_step()
            assert e == want[0] and np.array_equal(b, want[1]) and k == want[2], (i, e, want[0], k, want[2])
            assert np.array_equal(s.palette, ref.palette) and np.array_equal(s.palette_map, ref.palette_map), i
    for g in shards + [whole, ref]:
        g.close()


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_the_table_is_left_clear(S, img256_alpha, start, flags, monkeypatch):
    """A call with repeats, then a call on another slot whose list shares colours with the first — at other indices, so that
    an entry left behind would name the wrong candidate: the second call's errors equal a fresh context's."""
    used = context(S, img256_alpha, start, monkeypatch, **flags)
    fresh = context(S, img256_alpha, start, monkeypatch, **flags)
    old = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP": "0"}, **flags)
    rng = np.random.default_rng(41)
    first = list_with_repeats(rng, 3000, 500, [])
    second = np.concatenate([list_with_repeats(rng, 1500, 900, []), first[::-1][:1000]])
    rng.shuffle(second)
    assert {tuple(c) for c in first} & {tuple(c) for c in second}
    e_first = used.score_candidates(4, 9, first)
    assert np.array_equal(e_first, old.score_candidates(4, 9, first))
    e_used = used.score_candidates(0, 13, second)
    assert np.array_equal(e_used, fresh.score_candidates(0, 13, second))
    assert np.array_equal(e_used, old.score_candidates(0, 13, second))
    assert np.array_equal(used.score_candidates(4, 9, first), e_first)  # and back again
    for g in (used, fresh, old):
        g.close()


def test_a_list_below_the_threshold(S, img256_alpha, start, monkeypatch):
    """1,000 candidates with repeats: below SNES_DEDUP_MIN (1,024) the call is the old one.  What can be pinned from outside is
    its result: the default context, one without the feature and one with the feature forced onto every list agree."""
    new = context(S, img256_alpha, start, monkeypatch)
    old = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP": "0"})
    forced = context(S, img256_alpha, start, monkeypatch, {"SNES_DEDUP_MIN": "1"})
    dense = context(S, img256_alpha, start, monkeypatch, {"SNES_SPARSE": "0"})
    cand = list_with_repeats(np.random.default_rng(5), 1000, 120, [start[False][1][7 * 15 + 1]])
    e = new.score_candidates(7, 1, cand)
    for g in (old, forced, dense):
        assert np.array_equal(e, g.score_candidates(7, 1, cand))
    for g in (new, old, forced, dense):
        g.close()
