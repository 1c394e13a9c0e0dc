"""Ordered (Bayer) dithering on the parallel remap path (include/snesimage_hip.h: snesimage_set_ordered_dither).

The model is the unchanged CPU oracle twice (tests/ordered_model.py): one over the target image T makes the nearest-colour
choices, one over the original measures the error of the map chosen.  Maps, palettes and decisions agree bit for bit, errors
within the project's 1e-11 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ordered_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = M.REL_ERR
ERR_ARG, ERR_STATE, UNSUPPORTED = -1, -3, -5


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def bits(log):
    return [(float(e).hex(), int(k), tuple(int(v) for v in rgb), int(ch)) for (e, k, rgb, ch) in log]


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_bayer_known_answers(S):
    assert S.bayer_offsets(2, 64).ravel().tolist() == [-24, 8, 24, -8]
    assert S.bayer_offsets(2, 4).ravel().tolist() == [-2, 1, 2, -1]  # the half-way cases round away from zero
    assert S.bayer_offsets(4, 32).ravel().tolist() == [-15, 1, -11, 5, 9, -7, 13, -3, -9, 7, -13, 3, 15, -1, 11, -5]
    t = S.bayer_offsets(8, 255)
    assert (int(t.min()), int(t.max())) == (-126, 126)
    t = S.bayer_offsets(16, 255)
    assert (int(t.min()), int(t.max())) == (-127, 127) and t.dtype == np.int8 and t.shape == (16, 16)
    for bad in ((3, 32), (0, 32), (32, 32), (4, 0), (4, 256)):
        with pytest.raises(ValueError):
            S.bayer_offsets(*bad)


@pytest.mark.parametrize("n", [2, 4, 8, 16])
@pytest.mark.parametrize("amplitude", [1, 31, 32, 255])
def test_bayer_tables_sum_to_zero_and_follow_the_definition(S, n, amplitude):
    t = S.bayer_offsets(n, amplitude)
    assert int(t.astype(np.int64).sum()) == 0
    assert np.array_equal(t, M.bayer(n, amplitude))


def test_abi_declares_binds_and_exports_the_ordered_dither_symbols():
    from snesimage_amd import _ffi
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in ("snesimage_set_ordered_dither", "snesimage_get_ordered_dither", "snesimage_get_target_rgba", "snesimage_bayer_offsets"):
        assert name + "(" in text and name in bound and getattr(lib, name) is not None
    assert lib.snesimage_set_ordered_dither(None, None, 0) == ERR_ARG


def test_model_with_an_all_zero_table_is_the_plain_oracle(O):
    img = M.image(16, 0)
    m = M.Model(O, img, 2, 3, {}, np.zeros((4, 4), np.int8))
    o = O.OracleImage(img, 2, 3)
    m.kmeans_start()
    o.initialize_tiles()
    o.recalculate_palettes()
    assert np.array_equal(m.T, img) and np.array_equal(m.palette_map, o.palette_map) and m.error() == o.error()
    cand = O.random_candidates(3, 0, 6)
    e_m, maps_m = m.candidates([1 * 3 + 2], cand, want_maps=True)
    e_o, maps_o = o.score_candidates(1, 2, cand, want_maps=True)
    assert np.array_equal(e_m, e_o) and np.array_equal(maps_m, maps_o)
    for j, (method, p, i, ch, _) in enumerate(O.schedule(2, 3, 4)):
        e, rgb, _ = m.call(method, [p * 3 + i], ch, 1, j)
        e_o, rgb_o = o.step(method, p, i, ch, 1, j)
        assert e == e_o and np.array_equal(rgb, rgb_o)
    assert np.array_equal(m.palette, o.palette) and np.array_equal(m.palette_map, o.palette_map) and m.as_json() == o.as_json()


def test_model_target_image_clamps_and_keeps_alpha():
    img = M.with_hole(M.image(32, 1))
    img[0] = 0
    img[1, :, :3] = 255
    t = M.target_image(img, M.bayer(2, 64))  # rows [-24, 8] and [24, -8]
    assert np.array_equal(t[..., 3], img[..., 3])
    assert np.array_equal(t[0, :4, 0], [0, 8, 0, 8]) and np.array_equal(t[1, :4, 0], [255, 247, 255, 247])
    assert np.array_equal(t[2:, :, :3].astype(int), np.clip(img[2:, :, :3].astype(int) + np.tile(M.bayer(2, 64), (15, 128))[..., None], 0, 255))


def test_cli_ordered_dither_argument_rules(tmp_path):
    out = str(tmp_path / "o.json")
    for args, word in [(["--ordered-dither", "4", "-d"], "--dither"), (["--dither", "--ordered-dither", "8"], "--dither"),
                       (["--ordered-dither", "3"], "--ordered-dither"), (["--ordered-dither", "0"], "--ordered-dither"),
                       (["--ordered-dither", "32"], "--ordered-dither"), (["--ordered-dither", "4x"], "--ordered-dither"),
                       (["--dither-amplitude", "32"], "--ordered-dither"), (["--ordered-dither", "4", "--dither-amplitude", "0"], "--dither-amplitude"),
                       (["--ordered-dither", "4", "--dither-amplitude", "256"], "--dither-amplitude")]:
        r = run_cli("synth:1", out, *args)
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out)  # said before anything is loaded or a device touched
    r = run_cli("synth:1", out, "--ordered-dither")
    assert r.returncode == 2
    h = run_cli("--help").stderr
    assert "--ordered-dither" in h and "--dither-amplitude" in h and "default: 32" in h


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

def make_pair(S, O, img, count, size, flags, table):
    """A product context and the model, both with `table`, at the k-means initialisers."""
    g = S.OptimizedImage(img, count, size, **flags)
    g.set_ordered_dither(table)
    g.initialize_tiles()
    g.recalculate_palettes()
    m = M.Model(O, img, count, size, flags, table)
    m.kmeans_start()
    return g, m


def assert_same_state(g, m):
    assert np.array_equal(g.tile_palettes, m.tile_palettes) and np.array_equal(g.palette, m.palette) and np.array_equal(g.palette_map, m.palette_map)


@pytest.mark.gpu
@pytest.mark.parametrize("perceptual", [False, True], ids=["rgb", "perceptual"])
def test_target_image(S, perceptual):
    """T == numpy's, with transparent pixels, with rows of 0 and 255 (both clamps), for every table size; alpha untouched."""
    img = M.with_hole(M.image(32, 1))
    img[3] = (0, 0, 0, 255)
    img[4] = (255, 255, 255, 255)
    img[5, :, :3] = (0, 255, 128)
    g = S.OptimizedImage(img, 2, 3, perceptual=perceptual)
    assert g.ordered_dither is None and np.array_equal(g.target_rgba(), img)
    rng = np.random.default_rng(7)
    for table in (M.bayer(2, 96), M.bayer(4, 64), M.bayer(8, 48), M.bayer(16, 255), rng.integers(-128, 128, (8, 8)).astype(np.int8)):
        g.set_ordered_dither(table)
        t = g.target_rgba()
        assert np.array_equal(t, M.target_image(img, table)) and np.array_equal(t[..., 3], img[..., 3])
        assert np.array_equal(g.ordered_dither, table)
        assert t[3, :, :3].min() == 0 and t[4, :, :3].max() == 255
    g.set_ordered_dither(None)
    assert g.ordered_dither is None and np.array_equal(g.target_rgba(), img)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags,count,size,h,n,amp", [("rgb-8x15", {}, 8, 15, 32, 4, 64), ("perceptual-8x15", dict(perceptual=True), 8, 15, 32, 8, 48),
                                                          ("rgb-4x7", {}, 4, 7, 40, 2, 96), ("perceptual-4x7", dict(perceptual=True), 4, 7, 40, 4, 64)])
def test_optimize_and_error(S, O, name, flags, count, size, h, n, amp):
    img = M.image(h, 4, 1 if h == 40 else 0)
    table = M.bayer(n, amp)
    g, m = make_pair(S, O, img, count, size, flags, table)
    assert_same_state(g, m)
    e_g, e_m = g.error(), m.error()
    print("%s: error %r, model %r, rel %.3e" % (name, e_g, e_m, rel(e_g, e_m)))
    assert rel(e_g, e_m) < REL_ERR
    plain = O.OracleImage(img, count, size, **flags)
    plain.tile_palettes, plain.palette = m.tile_palettes, m.palette
    plain.optimize()
    assert not np.array_equal(plain.palette_map, m.palette_map), "the table changes no pixel's choice: the comparison shows nothing"
    # a palette set from outside
    pal = O.random_candidates(11, 0, count * size)
    g.palette = pal
    g.optimize()
    m.set_state(m.tile_palettes, pal)
    assert_same_state(g, m)
    assert rel(g.error(), m.error()) < REL_ERR
    g.close()


def candidate_list(O, current, seed):
    """64 candidates with the incumbent's colour (32) and a duplicate (40 == 7)."""
    cand = O.random_candidates(seed, 0, 64)
    cand[32] = current
    cand[40] = cand[7]
    return cand


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_score_candidates_on_a_regular_slot(S, O, flags):
    from hipmem import DeviceArray
    h = 32
    img = M.image(h, 5)
    g, m = make_pair(S, O, img, 2, 3, flags, M.bayer(4, 64))
    p, i = 1, 2
    inc = m.error()
    cand = candidate_list(O, m.palette[p * 3 + i], 5)
    e_model, maps_model = m.candidates([p * 3 + i], cand, want_maps=True)
    d_c, d_e, d_m = DeviceArray.from_numpy(cand), DeviceArray(64, np.float64, fill=0), DeviceArray((64, h, 256), np.uint8, fill=255)
    g.score_candidates_device(p, i, d_c.ptr, 64, d_e.ptr, d_m.ptr)  # maps asked for: the dense path
    g.sync()
    e_dense = d_e.numpy()
    print("max rel err of 64 candidates: %.3e" % float(np.max(np.abs(e_dense - e_model) / e_model)))
    assert np.array_equal(d_m.numpy(), maps_model)
    assert np.all(np.abs(e_dense - e_model) <= REL_ERR * e_model)
    assert rel(e_dense[32], inc) < REL_ERR and e_dense[40] == e_dense[7]
    e_sparse = g.score_candidates(p, i, cand)  # the group-sparse path
    assert np.array_equal(e_sparse, e_dense)
    d_r = DeviceArray((64, h, 256), np.uint8, fill=255)
    g.remap_candidates_device(p, i, d_c.ptr, 64, d_r.ptr)
    g.sync()
    assert np.array_equal(d_r.numpy(), maps_model)
    assert_same_state(g, m)  # scoring leaves the context as it was
    g.close()


@pytest.mark.gpu
def test_score_candidates_on_the_backdrop_slot(S, O):
    """A backdrop context takes a table like any other: B is one more entry in the choice against T; its initial value is
    the mean of the original."""
    import backdrop_model as BM
    from hipmem import DeviceArray
    h, Cn, Sz = 32, 2, 3
    img = M.image(h, 6)
    table = M.bayer(4, 64)
    g = S.OptimizedImage(img, Cn, Sz, backdrop=True)
    g.set_ordered_dither(table)
    g.initialize_tiles()
    g.recalculate_palettes()
    B = BM.mean_backdrop(img)
    assert np.array_equal(g.backdrop, B)
    m = M.Model(O, img, Cn, Sz + 1, {}, table)  # the expanded context: column Sz holds B
    tp, regular, _ = m.kmeans_start(Cn, Sz)
    pal = np.zeros((Cn, Sz + 1, 3), np.uint8)
    pal[:, :Sz] = regular.reshape(Cn, Sz, 3)
    pal[:, Sz] = B
    m.set_state(tp, pal.reshape(-1, 3))
    assert np.array_equal(g.tile_palettes, tp) and np.array_equal(g.palette, regular) and np.array_equal(g.palette_map, m.palette_map)
    assert (m.palette_map == Sz).any(), "no pixel shows the backdrop: the comparison shows nothing"
    tied = [q * (Sz + 1) + Sz for q in range(Cn)]
    cand = candidate_list(O, B, 8)
    e_model, maps_model = m.candidates(tied, cand, want_maps=True)
    d_c, d_e, d_m = DeviceArray.from_numpy(cand), DeviceArray(64, np.float64, fill=0), DeviceArray((64, h, 256), np.uint8, fill=255)
    g.score_candidates_device(Cn, 0, d_c.ptr, 64, d_e.ptr, d_m.ptr)
    g.sync()
    e_dense = d_e.numpy()
    assert np.array_equal(d_m.numpy(), maps_model)
    assert np.all(np.abs(e_dense - e_model) <= REL_ERR * e_model)
    assert rel(e_dense[32], m.error()) < REL_ERR and e_dense[40] == e_dense[7]
    assert np.array_equal(g.score_candidates(Cn, 0, cand), e_dense)
    # a regular slot of the same context, sparse against dense against the model
    cand = candidate_list(O, regular[1 * Sz + 1], 9)
    e_model = m.candidates([1 * (Sz + 1) + 1], cand)
    d_c.upload(cand)
    g.score_candidates_device(1, 1, d_c.ptr, 64, d_e.ptr, d_m.ptr)
    g.sync()
    e_dense = d_e.numpy()
    assert np.all(np.abs(e_dense - e_model) <= REL_ERR * e_model)
    assert np.array_equal(g.score_candidates(1, 1, cand), e_dense)
    g.close()


# (h, count, size, n, A, image seed, variant, flags, calls): the four model trajectories (the model passes its premise on each with margin); candidate seed 1, step_id = call number.
# synth_image's variant 1 clears alpha from row 96 on, so "variant1-32" has no transparent pixel; "hole-32" is a fifth picture
# that has (M.with_hole): the model's premise is asserted on it like on the others
TRAJ = {
    "rgb-16": (16, 2, 3, 4, 64, 0, 0, {}, 35),
    "variant1-32": (32, 2, 3, 8, 48, 1, 1, {}, 35),
    "hole-32": (32, 2, 3, 4, 64, 5, 0, {}, 35),
    "rgb-40-4x7": (40, 4, 7, 2, 96, 2, 0, {}, 29),
    "perceptual-16": (16, 2, 3, 4, 64, 3, 0, dict(perceptual=True), 35),
}
_models = {}


def traj_image(key):
    h, _, _, _, _, s, variant = TRAJ[key][:7]
    img = M.image(h, s, variant)
    return M.with_hole(img) if key.startswith("hole") else img


def model_run(O, key):
    if key not in _models:
        h, count, size, n, amp, s, variant, flags, calls = TRAJ[key]
        _models[key] = M.trajectory(O, traj_image(key), count, size, flags, M.bayer(n, amp), calls, 1)
    return _models[key]


def check_trajectory(S, O, key, windows=(0, 8, 1)):
    h, count, size, n, amp, s, variant, flags, calls = TRAJ[key]
    img, table = traj_image(key), M.bayer(n, amp)
    m, recs, final = model_run(O, key)
    print("%s: %d calls, %d changed the palette, smallest non-zero gap %.2e" % (key, calls, sum(r["changed"] for r in recs), m.min_gap))
    assert sum(r["changed"] for r in recs) >= 5 and m.min_gap > M.MIN_GAP
    logs = []
    for window in windows:
        g = S.OptimizedImage(img, count, size, **flags)
        g.set_ordered_dither(table)
        g.initialize_tiles()
        g.recalculate_palettes()
        if window == 1:  # call by call: everything observable after every call
            st, log = (0, 0, 0, 0), []
            for j, r in enumerate(recs):
                one, st, _ = g.run_slots(1, seed=1, first_step_id=j, state=st, window=1)
                log += one
                assert np.array_equal(g.palette, r["palette"]) and np.array_equal(g.palette_map, r["pmap"]), (key, j)
        else:
            log, st, stats = g.run_slots(calls, seed=1, first_step_id=0, state=(0, 0, 0, 0), window=window)
            assert stats["calls"] == calls
        for j, r in enumerate(recs):
            assert np.array_equal(log[j][2], r["rgb5"]) and log[j][3] == r["changed"], (key, window, j)
            assert rel(log[j][0], r["error"]) < REL_ERR, (key, window, j, log[j][0], r["error"])
        assert st == tuple(final)
        assert_same_state(g, m)
        assert g.as_json() == m.as_json()
        logs.append(bits(log))
        g.close()
    assert all(l == logs[0] for l in logs)  # the windows equal each other bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["rgb-16", "variant1-32", "hole-32", "rgb-40-4x7"])
def test_trajectory_through_the_slot_windows(S, O, key):
    check_trajectory(S, O, key)


@pytest.mark.gpu
def test_trajectory_with_poisoned_storage(S, O):
    """The perceptual trajectory with fresh group-sparse storage full of NaN bytes: nothing that no kernel wrote is read."""
    from snesimage_amd import _ffi
    _ffi.load().snesimage_debug_poison_alloc(1)
    try:
        check_trajectory(S, O, "perceptual-16")
    finally:
        _ffi.load().snesimage_debug_poison_alloc(0)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_split_phase_step(S, flags):
    """step_begin / min-reduce / step_commit over two shards on one context == step()."""
    from hipmem import DeviceArray
    img, table = M.image(32, 7), M.bayer(8, 48)
    ref = S.OptimizedImage(img, 2, 3, **flags)
    ref.set_ordered_dither(table)
    ref.initialize_tiles()
    ref.recalculate_palettes()
    s = S.OptimizedImage(img, 2, 3, **flags)
    s.set_ordered_dither(table)
    s.tile_palettes, s.palette = ref.tile_palettes, ref.palette
    s.optimize()
    changed = 0
    sched = S.schedule(2, 3, 80)
    calls = [c for c in sched if c[0] == S.METHOD_RANDOM][:6] + [c for c in sched if c[0] == S.METHOD_CHANNEL][:6]
    for j, (method, p, i, ch, _) in enumerate(calls):
        n = 64 if method == S.METHOD_RANDOM else 32
        before = ref.palette[p * 3 + i]
        e_ref, b_ref = ref.step(method, p, i, ch, 4, j)
        changed += int(not np.array_equal(before, b_ref))
        parts = []
        for r in range(2):  # both shards scored by the one context, one after the other, against the same state
            buf = DeviceArray(n, np.float64, fill=0)
            s.step_begin(method, p, i, ch, 4, j, n, r, 2, buf.ptr)
            s.sync()
            parts.append(buf.numpy())
        assert np.all(np.isinf(parts[0][1::2])) and np.all(np.isinf(parts[1][0::2]))
        red = DeviceArray.from_numpy(np.minimum(parts[0], parts[1]))
        s.step_commit(red.ptr)
        e, b, _ = s.last_step()
        assert e == e_ref and np.array_equal(b, b_ref), j
        assert np.array_equal(s.palette, ref.palette) and np.array_equal(s.palette_map, ref.palette_map), j
    assert changed, "no split-phase step changed the palette: the comparison shows nothing"
    s.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_initialisers_cluster_the_original(S, O, flags):
    """tile_palettes and palette are the plain oracle's on the original; the closing optimize() sees T."""
    img, table = M.with_hole(M.image(32, 8)), M.bayer(4, 64)
    g, m = make_pair(S, O, img, 4, 7, flags, table)
    plain = O.OracleImage(img, 4, 7, **flags)
    plain.initialize_tiles()
    assert np.array_equal(g.tile_palettes, plain.tile_palettes)
    plain.recalculate_palettes()
    assert np.array_equal(g.tile_palettes, plain.tile_palettes) and np.array_equal(g.palette, plain.palette)
    assert np.array_equal(g.palette_map, m.palette_map) and not np.array_equal(g.palette_map, plain.palette_map)
    # what initialisers fed T would give differs: the test tells the two builds apart
    wrong = O.OracleImage(m.T, 4, 7, **flags)
    wrong.initialize_tiles()
    wrong.recalculate_palettes()
    assert not np.array_equal(wrong.palette, plain.palette)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_reassign_tiles_and_tile_sweep(S, O, flags):
    """reassign_tiles takes its costs against T; a tile sweep over the first 32 tiles equals the model's tile calls, before and
    after the reassignment, for window 0 and 1."""
    import tile_model as T
    img, table = M.image(32, 9), M.bayer(4, 64)
    g, m = make_pair(S, O, img, 4, 3, flags, table)
    pal, changes = g.palette, 0
    for stage in range(2):
        if stage:
            moved = m.reassign_tiles()
            assert g.reassign_tiles() == moved and moved > 0
            assert_same_state(g, m)
            assert rel(g.error(), m.error()) < REL_ERR
        tp = g.tile_palettes
        want = T.model_tile_sweep(m.tile_oracle(), 0, 32, 4)
        changes += sum(ch for (_, _, ch) in want)
        for window in (0, 1):
            g.tile_palettes, g.palette = tp, pal
            g.optimize()
            log, _ = g.tile_sweep(0, 32, window=window)
            T.assert_log_matches(log, want)
            assert_same_state(g, m)
    assert changes, "no tile call moved a tile: the comparison shows nothing"
    errs = g.score_tile_moves([3, 5], [1, 2])
    for (t, s), e in zip([(3, 1), (5, 2)], errs):
        assert rel(e, T.model_candidate(m.tile_oracle(), t, s)[0]) < REL_ERR
    g.close()


@pytest.mark.gpu
def test_batch_of_four_images(S, O):
    """A batch steps every image exactly as the model steps it alone (candidate stream of image i keyed (1 + i, call))."""
    from snesimage_amd.throughput import ImageBatch
    table, n_calls = M.bayer(4, 64), 8
    imgs = [M.image(16, 10 + i) for i in range(4)]
    b = ImageBatch(list(enumerate(imgs)), 2, 3, batched=True, groups=1, ordered_dither=table)
    b.initialize()
    b.run(n_calls)
    errs = b.errors()
    accepted = 0
    for i, img in enumerate(imgs):
        m, recs, _ = M.trajectory(O, img, 2, 3, {}, table, n_calls, 1 + i)
        accepted += sum(r["changed"] for r in recs)
        assert_same_state(b.images[i], m)
        assert rel(errs[i], recs[-1]["error"]) < REL_ERR
    assert accepted, "no batched call changed a palette: the comparison shows nothing"
    b.close()


def set_model_call(models, method, p, i, ch, seed, step_id):
    """One optimizer call on a set of models: E_k = the members' errors summed in member order; lib.rs:216-219 on E."""
    O = models[0].O
    size = models[0].S
    before = models[0].palette[p * size + i].copy()
    if method == 0:
        cand = O.random_candidates(seed, step_id, 64)
    else:
        cand = np.repeat(before[None, :], 32, 0)
        cand[:, ch] = np.arange(32)
    best = 0.0
    for m in models:
        best += m.error()
    per = [m.candidates([p * size + i], cand) for m in models]
    best_k = -1
    for k in range(len(cand)):
        e = 0.0
        for v in per:
            e += v[k]
        M.check_gap(e, best)
        if e < best:
            best, best_k = e, k
    for m in models:
        pal = m.palette
        if best_k >= 0:
            pal[p * size + i] = cand[best_k]
        m.set_state(m.tile_palettes, pal)
    return best, models[0].palette[p * size + i].copy()


@pytest.mark.gpu
def test_set_of_three_frames(S, O):
    table, n_calls = M.bayer(4, 64), 10
    imgs = [M.image(16, 20 + i) for i in range(3)]

    def make_set(tab):
        ctxs = [S.OptimizedImage(f, 2, 3) for f in imgs]
        for c in ctxs:
            c.set_chunk(64)
        sp = S.SharedPalette(ctxs, ordered_dither=tab)
        sp.initialize_tiles()
        sp.recalculate_palettes()
        return ctxs, sp

    ctxs, sp = make_set(table)
    off, sp_off = make_set(None)  # the initialisers cluster the member stack of the originals: the table does not move them
    for c, o in zip(ctxs, off):
        assert np.array_equal(c.tile_palettes, o.tile_palettes) and np.array_equal(c.palette, o.palette)
    sp_off.close()
    for o in off:
        o.close()
    models = []
    for f, c in zip(imgs, ctxs):
        m = M.Model(O, f, 2, 3, {}, table)
        m.set_state(c.tile_palettes, c.palette)
        assert np.array_equal(c.palette_map, m.palette_map)
        models.append(m)
    assert rel(sp.error(), sum(m.error() for m in models)) < REL_ERR
    twin_ctxs, twin = make_set(table)
    log1, st1, _ = twin.run_slots(n_calls, seed=3, window=1)
    log0, st0, _ = sp.run_slots(n_calls, seed=3, window=0)
    assert st0 == st1 and bits(log0) == bits(log1)
    changed = 0
    for j, (method, p, i, ch, _) in enumerate(S.schedule(2, 3, n_calls)):
        e, rgb = set_model_call(models, method, p, i, ch, 3, j)
        assert np.array_equal(log0[j][2], rgb) and rel(log0[j][0], e) < REL_ERR, j
        changed += log0[j][3]
    assert changed, "no call changed the shared palette: the comparison shows nothing"
    for c, t, m in zip(ctxs, twin_ctxs, models):
        assert_same_state(c, m)
        assert_same_state(t, m)
    sp.close()
    twin.close()
    for c in ctxs + twin_ctxs:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, dict(perceptual=True)], ids=["rgb", "perceptual"])
def test_off_means_off(S, flags):
    img = M.image(16, 30)

    def fresh(table=None, prepare=None):
        g = S.OptimizedImage(img, 2, 3, **flags)
        if prepare:
            prepare(g)
        if table is not None:
            g.set_ordered_dither(table)
        g.initialize_tiles()
        g.recalculate_palettes()
        return g

    def observe(g):
        cand = S.random_candidates(2, 0, 64)
        out = [g.error(), g.palette_map.tobytes(), g.score_candidates(1, 1, cand).tobytes()]
        log, st, _ = g.run_slots(12, seed=1)
        return out + [bits(log), st, g.palette.tobytes(), g.palette_map.tobytes(), g.error()]

    never = observe(fresh())
    g = fresh(np.zeros((4, 4), np.int8))  # an all-zero table
    assert g.ordered_dither is not None and observe(g) == never
    g.close()
    g = fresh(prepare=lambda c: (c.set_ordered_dither(M.bayer(8, 200)), c.optimize(), c.set_ordered_dither(None)))  # n = 0 after a non-zero table
    assert g.ordered_dither is None and observe(g) == never
    g.close()
    # a table set after a run (slot contexts already built) == a fresh context with that table
    table = M.bayer(4, 64)
    g = fresh()
    g.run_slots(12, seed=1)
    tp, pal = g.tile_palettes, g.palette
    g.set_ordered_dither(table)
    g.optimize()
    f = S.OptimizedImage(img, 2, 3, **flags)
    f.set_ordered_dither(table)
    f.tile_palettes, f.palette = tp, pal
    f.optimize()
    assert g.error() == f.error() and np.array_equal(g.palette_map, f.palette_map)
    log_g, st_g, _ = g.run_slots(12, seed=1, first_step_id=12, state=(0, 0, 0, 2))
    log_f, st_f, _ = f.run_slots(12, seed=1, first_step_id=12, state=(0, 0, 0, 2))
    assert bits(log_g) == bits(log_f) and st_g == st_f
    assert np.array_equal(g.palette, f.palette) and np.array_equal(g.palette_map, f.palette_map) and g.error() == f.error()
    # and off again after that run: the context without a table, in the same state
    g.set_ordered_dither(None)
    g.optimize()
    f.set_ordered_dither(None)
    f.optimize()
    p = S.OptimizedImage(img, 2, 3, **flags)
    p.tile_palettes, p.palette = g.tile_palettes, g.palette
    p.optimize()
    assert g.error() == p.error() and np.array_equal(g.palette_map, p.palette_map)
    assert bits(g.run_slots(6, seed=2)[0]) == bits(p.run_slots(6, seed=2)[0])
    for c in (g, f, p):
        c.close()


@pytest.mark.gpu
def test_refusals(S):
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = M.image(16, 31)
    table = M.bayer(4, 64)
    tp = table.ctypes.data_as(_ffi._i8p)

    def ctx(tab=None, **flags):
        c = S.OptimizedImage(img, 2, 3, **flags)
        c.set_chunk(64)
        if tab is not None:
            c.set_ordered_dither(tab)
        return c

    def refused(call, code):
        with pytest.raises(S.SnesImageError) as e:
            call()
        assert e.value.code == code, str(e.value)

    g = ctx()
    g.initialize_tiles()
    g.recalculate_palettes()
    before = g.error()
    # SNES_ERR_ARG: null context, n outside {0, 2, 4, 8, 16}, null table with n > 0
    assert L.snesimage_set_ordered_dither(None, tp, 4) == ERR_ARG
    for n in (1, 3, 5, 32):
        assert L.snesimage_set_ordered_dither(g._c, tp, n) == ERR_ARG
    assert L.snesimage_set_ordered_dither(g._c, None, 4) == ERR_ARG
    assert g.ordered_dither is None and g.error() == before
    # SNES_ERR_UNSUPPORTED: a table on a SNES_DITHER context (switching "off" there is no error)
    d = ctx(dither=True)
    refused(lambda: d.set_ordered_dither(table), UNSUPPORTED)
    d.set_ordered_dither(None)
    d.close()
    # SNES_ERR_STATE: between the phases of a split-phase step ...
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    refused(lambda: g.set_ordered_dither(table), ERR_STATE)
    g.step_commit(buf.ptr)
    # ... and of a split-phase window
    taken, _ = g.slots_begin(4, 1, 1, (0, 1, 0, 0))
    refused(lambda: g.set_ordered_dither(table), ERR_STATE)
    g.slots_commit(0, taken)
    g.set_ordered_dither(table)  # usable afterwards
    g.optimize()
    assert g.error() != before
    # ... and on a context lent to a batch, a set or a group
    a, b = ctx(table), ctx(table)
    for create, destroy in ((L.snesimage_batch_create, L.snesimage_batch_destroy), (L.snesimage_shared_create, L.snesimage_shared_destroy)):
        arr = (C.c_void_p * 2)(a._c, b._c)
        h = C.c_void_p()
        assert create(arr, 2, C.byref(h)) == 0, L.snesimage_last_error()
        refused(lambda: a.set_ordered_dither(None), ERR_STATE)
        refused(lambda: b.set_ordered_dither(M.bayer(2, 8)), ERR_STATE)
        destroy(h)
    arr1 = (C.c_void_p * 1)(a._c)
    h = C.c_void_p()
    assert L.snesimage_group_create(arr1, 1, C.byref(h)) == 0, L.snesimage_last_error()
    refused(lambda: a.set_ordered_dither(None), ERR_STATE)
    refused(lambda: a.set_ordered_dither(M.bayer(2, 8)), ERR_STATE)
    L.snesimage_group_destroy(h)
    # members whose tables differ: SNES_ERR_ARG from all three, as for differing flags
    other = table.copy()
    other[3, 3] += 1
    b.set_ordered_dither(other)
    c = ctx(None)
    for x, y in ((a, b), (a, c), (c, a)):
        arr = (C.c_void_p * 2)(x._c, y._c)
        for create in (L.snesimage_batch_create, L.snesimage_shared_create, L.snesimage_group_create):
            h = C.c_void_p()
            assert create(arr, 2, C.byref(h)) == ERR_ARG and not h.value, create
    assert b"ordered-dither" in L.snesimage_last_error()
    b.set_ordered_dither(table)  # the contexts are their own again
    a.initialize_tiles()
    for x in (a, b, c, g):
        x.close()


@pytest.mark.gpu
def test_cli_round_trip(tmp_path, S, O):
    """--ordered-dither 4 writes the model's JSON; --resume (naming the option again) continues to the file an uninterrupted run
    writes; --share with one more frame runs."""
    img = M.with_hole(M.image(64, 40))
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    a, b, c = str(tmp_path / "a.json"), str(tmp_path / "b.json"), str(tmp_path / "c.json")
    common = ["-c", "2", "-s", "3", "--ordered-dither", "4", "--seed", "1"]
    r = run_cli(str(src), a, *common, "--calls", "12", "--preview", str(tmp_path / "p.png"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Ordered dithering: 4 x 4" in r.stdout
    m, recs, _ = M.trajectory(O, img, 2, 3, {}, M.bayer(4, 32), 12, 1)
    assert sum(x["changed"] for x in recs) > 0
    assert open(a).read() == m.as_json()
    # an uninterrupted run of 0 further calls from the first file: --resume re-derives the map from palette and tile palettes against T
    r = run_cli(str(src), b, *common, "--resume", a, "--calls", "0")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(b).read() == open(a).read()
    r = run_cli(str(src), c, "-c", "2", "-s", "3", "--resume", a, "--calls", "0")  # without the option the map is the plain one
    assert r.returncode == 0 and open(c).read() != open(a).read()
    # six further calls from the file == the library continuing from that state without an interruption
    r = run_cli(str(src), c, *common, "--resume", a, "--calls", "6")
    assert r.returncode == 0, r.stdout + r.stderr
    g = S.OptimizedImage(img, 2, 3)
    g.set_ordered_dither(S.bayer_offsets(4, 32))
    g.tile_palettes, g.palette = m.tile_palettes, m.palette
    g.optimize()
    g.run_slots(6, seed=1)
    assert g.as_json() == open(c).read()
    g.close()
    # the library driven the same way
    g = S.OptimizedImage(img, 2, 3)
    g.set_ordered_dither(S.bayer_offsets(4, 32))
    g.initialize_tiles()
    g.recalculate_palettes()
    g.run_slots(12, seed=1)
    assert g.as_json() == open(a).read()
    g.close()
    frame = tmp_path / "f.rgba"
    frame.write_bytes(M.with_hole(M.image(64, 41)).tobytes())
    s0, s1 = str(tmp_path / "s0.json"), str(tmp_path / "s1.json")
    r = run_cli(str(src), s0, *common, "--dither-amplitude", "48", "--calls", "6", "--share", str(frame) + "=" + s1)
    assert r.returncode == 0, r.stdout + r.stderr
    import json
    assert json.loads(open(s0).read())["palette"] == json.loads(open(s1).read())["palette"]
