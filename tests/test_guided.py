"""Guided calls (include/snesimage_hip.h: snesimage_guided_costs, _candidates, _step, _sweep).

The model is tests/guided_model.py: the definition in numpy integers over the CPU oracle.  Costs, shortlists, palettes, maps and
decisions agree bit for bit, errors within the project's 1e-11 relative.  The trajectories' inputs are guided_model.CASES;
tests/test_guided_model.py shows on the CPU that the model's calls on each of them hold the gap premise and accept and reject."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adversarial_images as AI
import guided_model as GM
import ordered_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "snesimage_amd", "snesimage_cli")
REL_ERR = GM.REL_ERR
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
NAMES = ("snesimage_guided_costs", "snesimage_guided_candidates", "snesimage_guided_step", "snesimage_guided_sweep")


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def close(a, b):
    return abs(a - b) <= REL_ERR * abs(b)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_guided_symbols():
    from snesimage_amd import _ffi
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in NAMES + ("snesimage_guided_step_async",):
        assert name + "(" in text and name in bound and getattr(lib, name) is not None
    costs, rgb5 = (C.c_uint64 * 32768)(), (C.c_uint8 * 48)()
    assert lib.snesimage_guided_costs(None, 0, 0, costs) == ERR_ARG
    assert lib.snesimage_guided_candidates(None, 0, 0, 16, rgb5, None) == ERR_ARG
    assert lib.snesimage_guided_step(None, 0, 0, 16, None, None) == ERR_ARG
    assert lib.snesimage_guided_step_async(None, 0, 0, 16) == ERR_ARG
    assert lib.snesimage_guided_sweep(None, 16, None, None) == ERR_ARG
    import snesimage_amd
    for method in ("guided_costs", "guided_candidates", "guided_step", "guided_sweep"):
        assert callable(getattr(snesimage_amd.OptimizedImage, method))


def test_cli_argument_rules(tmp_path):
    out, share = str(tmp_path / "o.json"), "synth:2=" + str(tmp_path / "s.json")
    for args, word in [(["--guided", "1", "--share", share], "--share"), (["--guided", "1", "--devices", "0"], "--devices"), (["--guided", "1", "--nes"], "--nes"),
                       (["--guided", "1", "--guided-shortlist", "8", "--share", share], "--share"), (["--nes", "--guided", "2", "--guided-shortlist", "8"], "--nes"),
                       (["--guided", "0"], "--guided"), (["--guided", "x"], "--guided"), (["--guided", "-1"], "--guided"), (["--guided", ""], "--guided"),
                       (["--guided", "1", "--guided-shortlist", "0"], "--guided-shortlist"), (["--guided", "1", "--guided-shortlist", "65"], "--guided-shortlist"),
                       (["--guided", "1", "--guided-shortlist", "k"], "--guided-shortlist"), (["--guided-shortlist", "8"], "--guided")]:
        r = run_cli("synth:1", out, *args)
        assert r.returncode == 2 and "error:" in r.stderr and word in r.stderr, (args, r.stderr)
        assert "Using source image" not in r.stdout and not os.path.exists(out) and not os.path.exists(str(tmp_path / "s.json"))  # said before any file or device is touched
    h = run_cli("--help").stderr
    assert "--guided <G>" in h and "--guided-shortlist <K>" in h and "default: 16: a choice, not a measurement" in h


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

def context(S, m, table=None):
    """A library context in the model's state."""
    g = S.OptimizedImage(m.img, m.C, m.S, backdrop=m.backdrop, **m.flags)
    if table is not None:
        g.set_ordered_dither(table)
    g.tile_palettes, g.palette = m.tile_palettes, m.palette
    if m.backdrop:
        g.backdrop = m.B
    g.optimize()
    return g


def assert_costs_equal(got, want, what):
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.shape == want.shape == (32768,)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of 32768 costs differ, first at u = %d: %d against %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
def test_costs_one_tile_row_and_more_than_one_slice(S, O):
    m = GM.Model(O, GM.image(8, 5), 1, 4)  # 2,048 pixels in one subpalette: two slices of the list
    g = context(S, m)
    before = (g.error(), g.palette.tobytes(), g.palette_map.tobytes())
    for i in (0, 3):
        assert_costs_equal(g.guided_costs(0, i), m.costs(0, i), "1 x 4 slot (0, %d)" % i)
    assert (g.error(), g.palette.tobytes(), g.palette_map.tobytes()) == before, "guided_costs changed the state"
    g.close()
    m.close()


@pytest.mark.gpu
def test_costs_of_a_one_entry_subpalette_have_no_floor(S):
    img = GM.image(8, 6)
    g = S.OptimizedImage(img, 1, 1)
    g.palette = [[10, 12, 7]]
    g.optimize()
    want = GM.costs(img, np.zeros(1024, np.uint8), np.array([[10, 12, 7]], np.uint8), 1, 1, 0, 0)
    assert int(want[0]) == int(GM.red_mean_key(img[..., :3].reshape(-1, 3), [0, 0, 0]).sum())  # no floor: the plain sum of keys
    assert_costs_equal(g.guided_costs(0, 0), want, "1 x 1")
    g.close()


@pytest.mark.gpu
def test_costs_of_an_unused_subpalette_are_zero(S, O):
    m = GM.Model(O, GM.image(24, 7), 4, 7)
    tp = m.tile_palettes
    tp[tp == 3] = 0
    m.set_tile_palettes(tp)
    g = context(S, m)
    assert not g.guided_costs(3, 2).any() and not m.costs(3, 2).any()
    assert_costs_equal(g.guided_costs(0, 6), m.costs(0, 6), "4 x 7 slot (0, 6) with the tiles of subpalette 3")
    rgb5, cost = g.guided_candidates(3, 2, 8)  # every cost ties at 0: the lowest colours, the current one left out
    cur = int(GM.pack_u(m.internal[3 * 7 + 2]))
    assert GM.pack_u(rgb5).tolist() == [u for u in range(10) if u != cur][:8] and not cost.any()
    g.close()
    m.close()


@pytest.mark.gpu
def test_costs_with_transparent_pixels(S, O):
    img = OM.with_hole(GM.image(104, 8, variant=1))  # whole transparent tiles (rows 96..103) and partly transparent ones: 26,624 - 1,312 pixels
    assert (img[96:, 96:160, 3] == 0).all() and (img[..., 3] == 0).sum() == 8 * 64 + 16 * 50
    m = GM.Model(O, img, 2, 3)
    g = context(S, m)
    for p, i in ((0, 1), (1, 2)):
        assert_costs_equal(g.guided_costs(p, i), m.costs(p, i), "alpha image slot (%d, %d)" % (p, i))
    g.close()
    m.close()


@pytest.mark.gpu
def test_costs_read_the_ordered_dither_target(S, O):
    table = OM.bayer(4, 64)
    m = GM.Model(O, GM.image(16, 9), 2, 3, {}, table)
    g = context(S, m, table)
    assert np.array_equal(g.target_rgba(), m.T) and not np.array_equal(m.T, m.img)
    want = m.costs(1, 0)
    assert_costs_equal(g.guided_costs(1, 0), want, "Bayer 4 x 4 slot (1, 0)")
    plain = GM.costs(m.img, m.tile_palettes, m.internal, 2, 3, 1, 0)
    assert (plain != want).any(), "the table changes no cost: the case shows nothing"
    g.close()
    m.close()


@pytest.mark.gpu
def test_costs_on_a_backdrop_context_regular_and_tied(S, O):
    m = GM.Model(O, GM.image(16, 10), 2, 3, {}, None, True)
    g = context(S, m)
    assert np.array_equal(g.backdrop, m.B)
    assert_costs_equal(g.guided_costs(1, 1), m.costs(1, 1), "backdrop context, regular slot (1, 1)")
    assert_costs_equal(g.guided_costs(2, 0), m.costs(2, 0), "backdrop context, the tied slot")
    without_b = GM.costs(m.T, m.tile_palettes, m.palette, 2, 3, 1, 1)  # the floor of a regular slot counts B as one of the other entries
    assert (without_b != m.costs(1, 1)).any()
    g.close()
    m.close()


@pytest.mark.gpu
def test_candidates_order_costs_and_lengths(S, O):
    m = GM.Model(O, GM.image(16, 11), 2, 3)
    g = context(S, m)
    before = (g.error(), g.palette.tobytes(), g.palette_map.tobytes())
    cost = m.costs(1, 2)
    cur = m.internal[1 * 3 + 2]
    for k, n in ((0, 16), (1, 1), (16, 16), (64, 64)):
        rgb5, c = g.guided_candidates(1, 2, k)
        want_rgb5, want_c = GM.shortlist(cost, cur, k)
        assert rgb5.shape == (n, 3) and np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c), k
        assert not any(np.array_equal(x, cur) for x in rgb5)
        assert np.array_equal(c, cost[GM.pack_u(rgb5)]) and (np.diff(c.astype(np.int64)) >= 0).all()
    assert (g.error(), g.palette.tobytes(), g.palette_map.tobytes()) == before, "guided_candidates changed the state"
    # the current colour is the cheapest of all only if it is left out on purpose: put the proxy's best into the slot
    best = GM.shortlist(cost, cur, 1)[0][0]
    pal = m.internal
    pal[5] = best
    m.set_internal(pal)
    g.palette = m.palette
    g.optimize()
    rgb5, c = g.guided_candidates(1, 2, 4)
    want_rgb5, want_c = GM.shortlist(m.costs(1, 2), best, 4)
    assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c) and not any(np.array_equal(x, best) for x in rgb5)
    assert np.array_equal(m.costs(1, 2), cost), "the table does not depend on the slot's own colour: the floor runs over the other entries"
    refused(S, lambda: g.guided_candidates(1, 2, 65), ERR_ARG)
    refused(S, lambda: g.guided_candidates(2, 0, 4), ERR_ARG)
    refused(S, lambda: g.guided_costs(0, 3), ERR_ARG)
    g.close()
    m.close()


@pytest.mark.gpu
def test_candidates_tie_rule_on_a_flat_picture(S):
    """two_tone: black and white pixels, and flat grey in columns 128..191.  The grey tiles use subpalette 1; subpalette 0 holds
    black and white exactly, so every pixel of slot (0, 2) has floor 0, every cost is 0 and the order is the colours' own —
    with the slot's current colour, u = 3, left out.  Slot (1, 0) sees 512 equal pixels, grey 128, beside an entry at (132, 140, 132):
    24 colours lie nearer than that entry, every other colour costs 512 * floor, and the shortlist of 64 is the 24 by cost and
    then the lowest colours of the tie."""
    img = AI.two_tone(8)
    tp = np.zeros(1024, np.uint8)
    tp[16:24] = 1
    pal = np.array([[0, 0, 0], [31, 31, 31], [3, 0, 0], [2, 2, 2], [16, 17, 16], [31, 0, 0]], np.uint8)
    g = S.OptimizedImage(img, 2, 3)
    g.tile_palettes, g.palette = tp, pal
    g.optimize()
    want = GM.costs(img, tp, pal, 2, 3, 0, 2)
    assert not want.any()
    assert_costs_equal(g.guided_costs(0, 2), want, "flat picture, slot (0, 2)")
    rgb5, c = g.guided_candidates(0, 2, 64)
    assert GM.pack_u(rgb5).tolist() == [u for u in range(65) if u != 3] and not c.any()
    want = GM.costs(img, tp, pal, 2, 3, 1, 0)
    floor = int(GM.red_mean_key([128, 128, 128], [132, 140, 132]))
    assert int(want.max()) == 512 * floor and (want == 512 * floor).sum() == 32768 - 24, "all but 24 colours lie beyond the floor and tie"
    assert_costs_equal(g.guided_costs(1, 0), want, "flat picture, slot (1, 0)")
    rgb5, c = g.guided_candidates(1, 0, 64)
    want_rgb5, want_c = GM.shortlist(want, pal[3], 64)
    assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c)
    assert (c[:24] < 512 * floor).all() and (c[24:] == 512 * floor).all() and GM.pack_u(rgb5[24:]).tolist() == list(range(40))
    g.close()


def case_context(S, r):
    g = S.OptimizedImage(r["img"], r["C"], r["S"], backdrop=r["backdrop"], **r["flags"])
    g.tile_palettes, g.palette = r["tp"], r["pal0"]
    if r["backdrop"]:
        g.backdrop = r["B0"]
    g.optimize()
    return g


def assert_state(g, rec, what):
    assert np.array_equal(g.palette, rec["palette"]), what
    if rec["B"] is not None:
        assert np.array_equal(g.backdrop, rec["B"]), what
    assert np.array_equal(g.palette_map, rec["pmap"]), what
    assert close(g.error(), rec["error"]), (what, g.error(), rec["error"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_guided_steps_follow_the_model(S, O, name):
    r = GM.trajectory(O, name)
    g = case_context(S, r)
    assert np.array_equal(g.palette_map, r["map0"]) and close(g.error(), r["err0"])
    for j, rec in enumerate(r["recs"]):
        what = "%s call %d slot (%d, %d)" % (name, j, rec["p"], rec["i"])
        rgb5, cost = g.guided_candidates(rec["p"], rec["i"], r["K"])
        assert np.array_equal(rgb5, rec["cand"]) and np.array_equal(cost, rec["costs"]), what
        err, best = g.guided_step(rec["p"], rec["i"], r["K"])
        e2, b2, k2 = g.last_step()
        print("%s: best_k %d (model %d), error %.9f (model %.9f)" % (what, k2, rec["best_k"], err, rec["error"]))
        assert k2 == rec["best_k"] and np.array_equal(best, rec["rgb5"]) and np.array_equal(b2, rec["rgb5"]) and e2 == err and close(err, rec["error"]), what
        assert_state(g, rec, what)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GM.CASES))
def test_guided_sweep_equals_the_calls_one_by_one_and_the_model(S, O, name):
    r = GM.trajectory(O, name)
    g, twin = case_context(S, r), case_context(S, r)
    log, stats = g.guided_sweep(r["K"])
    slots = [(p, i) for p in range(r["C"]) for i in range(r["S"])] + ([(r["C"], 0)] if r["backdrop"] else [])
    assert len(log) == len(slots) and stats["calls"] == len(slots) and stats["scored"] == len(slots) * r["K"]
    for j, (p, i) in enumerate(slots):
        twin.guided_step(p, i, r["K"])
        e, b, k = twin.last_step()
        assert log[j][0] == e and log[j][1] == k and np.array_equal(log[j][2], b) and log[j][3] == int(k >= 0), (name, j, log[j], (e, b, k))
    assert stats["accepted"] == sum(x[3] for x in log) and 0 < stats["accepted"]
    assert np.array_equal(g.palette, twin.palette) and np.array_equal(g.palette_map, twin.palette_map) and g.error() == twin.error()
    assert g.last_step()[0] == twin.last_step()[0] and g.last_step()[2] == twin.last_step()[2]
    n = min(len(slots), len(r["recs"]))
    for j, rec in enumerate(r["recs"][:n]):
        assert (rec["p"], rec["i"]) == slots[j] and log[j][1] == rec["best_k"] and np.array_equal(log[j][2], rec["rgb5"]) and close(log[j][0], rec["error"]), (name, j)
    if n == len(slots):
        assert_state(g, r["recs"][n - 1], name + " after the sweep")
    # behind the sweep the context steps exactly as one whose palette was set to the same values
    fresh = S.OptimizedImage(r["img"], r["C"], r["S"], backdrop=r["backdrop"], **r["flags"])
    fresh.tile_palettes, fresh.palette = r["tp"], g.palette
    if r["backdrop"]:
        fresh.backdrop = g.backdrop
    fresh.optimize()
    for j, (p, i) in enumerate(slots[:3] + slots[-1:]):
        ea, ba = g.step(S.METHOD_RANDOM, p, i, 0, 5, j, 32)
        eb, bb = fresh.step(S.METHOD_RANDOM, p, i, 0, 5, j, 32)
        assert np.array_equal(ba, bb) and g.last_step()[2] == fresh.last_step()[2] and close(ea, eb), (name, j)
        assert np.array_equal(g.palette, fresh.palette) and np.array_equal(g.palette_map, fresh.palette_map)
    for x in (g, twin, fresh):
        x.close()


def refused(S, fn, code):
    with pytest.raises(S.SnesImageError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def all_refused(S, g, code):
    refused(S, lambda: g.guided_costs(0, 0), code)
    refused(S, lambda: g.guided_candidates(0, 0), code)
    refused(S, lambda: g.guided_step(0, 0), code)
    refused(S, lambda: g.guided_step_async(0, 0), code)
    refused(S, lambda: g.guided_sweep(), code)


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(S):
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    img = GM.image(16, 12)

    def started(**flags):
        g = S.OptimizedImage(img, 2, 3, **flags)
        g.initialize_tiles()
        g.recalculate_palettes()
        return g

    def state(g):
        return (g.error(), g.palette.tobytes(), g.palette_map.tobytes())

    # a NES context
    g = started(nes=True)
    before = state(g)
    all_refused(S, g, UNSUPPORTED)
    assert state(g) == before
    g.step(S.METHOD_NES, 0, 0)
    g.close()
    # lent to a set
    g = started()
    g.set_chunk(64)
    before = state(g)
    sp = S.SharedPalette([g])
    all_refused(S, g, ERR_STATE)
    sp.close()
    assert state(g) == before
    # between the phases of a split-phase step
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    all_refused(S, g, ERR_STATE)
    g.step_commit(buf.ptr)
    # a failed workspace allocation
    before = state(g)
    L.snesimage_debug_fail_alloc(0)
    try:
        assert "workspace" in refused(S, lambda: g.guided_costs(0, 0), ERR_HIP)
    finally:
        L.snesimage_debug_fail_alloc(-1)
    L.snesimage_debug_fail_alloc(1)
    try:
        refused(S, lambda: g.guided_sweep(), ERR_HIP)
    finally:
        L.snesimage_debug_fail_alloc(-1)
    assert state(g) == before
    twin = S.OptimizedImage(img, 2, 3)
    twin.tile_palettes, twin.palette = g.tile_palettes, g.palette
    twin.optimize()
    assert np.array_equal(g.guided_costs(1, 1), twin.guided_costs(1, 1))
    la, lb = g.guided_sweep(4)[0], twin.guided_sweep(4)[0]
    assert [(x[1], x[2].tolist()) for x in la] == [(x[1], x[2].tolist()) for x in lb] and np.array_equal(g.palette, twin.palette)
    # arguments
    refused(S, lambda: g.guided_step(2, 0), ERR_ARG)
    refused(S, lambda: g.guided_sweep(65), ERR_ARG)
    assert L.snesimage_guided_costs(g._c, 0, 0, None) == ERR_ARG and L.snesimage_guided_candidates(g._c, 0, 0, 4, None, None) == ERR_ARG
    g.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("proxy", ["redmean", "cielab"])
def test_the_member_table_follows_the_context(S, proxy):
    """The generator reaches a context's planes through a one-entry member table on the device (kernels_guide.hpp: GuideMember).
    The target moves when an ordered-dither table is set or cleared, the candidate list when a call needs more room than 64:
    the calls behind either equal those of a fresh context in the same state, whose table was written once."""
    img, table = GM.image(16, 14), OM.bayer(4, 64)

    def fresh_twin(g, table):
        t = S.OptimizedImage(img, 2, 3)
        t.guided_proxy = proxy
        if table is not None:
            t.set_ordered_dither(table)
        t.tile_palettes, t.palette = g.tile_palettes, g.palette
        t.optimize()
        return t

    g = S.OptimizedImage(img, 2, 3)
    g.guided_proxy = proxy
    g.initialize_tiles()
    g.recalculate_palettes()
    assert sorted(np.unique(g.tile_palettes).tolist()) == [0, 1], "one subpalette is unused: the case shows less"
    plain = g.guided_costs(0, 1)  # the member table exists
    g.set_ordered_dither(table)  # the target moves
    g.optimize()
    g.step(S.METHOD_RANDOM, 1, 0, 0, 1, 0, 256)  # the candidate list grows
    twin = fresh_twin(g, table)
    dithered = g.guided_costs(0, 1)
    assert (dithered != plain).any(), "the table changes no cost: the case shows nothing"  # (the step touched subpalette 1 only)
    assert_costs_equal(dithered, twin.guided_costs(0, 1), "slot (0, 1) behind the table and the long call")
    assert_costs_equal(g.guided_costs(1, 2), twin.guided_costs(1, 2), "slot (1, 2) behind the table and the long call")
    (ra, ca), (rb, cb) = g.guided_candidates(1, 1, 8), twin.guided_candidates(1, 1, 8)
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)
    la, lb = g.guided_sweep(4)[0], twin.guided_sweep(4)[0]
    assert [(x[1], x[2].tolist()) for x in la] == [(x[1], x[2].tolist()) for x in lb] and all(close(x[0], y[0]) for x, y in zip(la, lb))
    assert np.array_equal(g.palette, twin.palette) and np.array_equal(g.palette_map, twin.palette_map)
    g.set_ordered_dither(None)  # the target moves back
    g.optimize()
    twin.close()
    twin = fresh_twin(g, None)
    assert_costs_equal(g.guided_costs(0, 1), twin.guided_costs(0, 1), "slot (0, 1) behind the cleared table")
    g.close()
    twin.close()


def drive(S, g, calls, every, k, seed=1, fixed=False):
    """The CLI's loop call by call: scheduled calls of 64, one guided sweep behind every `every` sweeps of the palette.
    fixed: --backdrop-fixed, whose schedule and guided sweeps pass the backdrop slot by."""
    sched = S.schedule(g.sub_count, g.sub_size, calls + 1)
    sweeps = 0
    for j in range(calls):
        method, p, i, ch, step = sched[j]
        g.step(method, p, i, ch, seed, j, 64 if method == S.METHOD_RANDOM else 0)
        after = sched[j + 1][4]
        if after != step and after % every == 0:
            if fixed:
                for p, i in [(p, i) for p in range(g.sub_count) for i in range(g.sub_size)]:
                    g.guided_step(p, i, k)
            else:
                g.guided_sweep(k)
            sweeps += 1
    return sweeps


@pytest.mark.gpu
def test_cli_guided_sweeps_write_what_the_library_writes(tmp_path, S):
    """The CLI takes synth:SEED at 256 x 256 only; a small picture goes in as a raw RGBA file of the same generator."""
    img = GM.image(16, 13)
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    sched = S.schedule(2, 3, 64)
    ends = [j for j in range(63) if sched[j + 1][4] != sched[j][4]]
    calls = ends[1] + 3  # two sweeps of the palette end inside the run, and it stops in the middle of the third
    a, b = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    common = ["-c", "2", "-s", "3", "--seed", "1", "--guided", "1", "--guided-shortlist", "8", "--calls", str(calls)]
    r = run_cli(str(src), a, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("Guided sweep: 6 calls, ") == 2, r.stdout
    g = S.OptimizedImage(img, 2, 3)
    g.initialize_tiles()
    g.recalculate_palettes()
    assert drive(S, g, calls, 1, 8) == 2
    assert g.as_json() == open(a).read()
    g.close()
    r = run_cli(str(src), b, *common, "--window", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(b).read() == open(a).read() and r.stdout.count("Guided sweep: 6 calls, ") == 2
    plain = str(tmp_path / "p.json")
    assert run_cli(str(src), plain, "-c", "2", "-s", "3", "--seed", "1", "--calls", str(calls)).returncode == 0
    assert open(plain).read() != open(a).read(), "the guided sweeps changed nothing: the comparison shows nothing"


@pytest.mark.gpu
def test_cli_guided_sweeps_pass_a_fixed_backdrop_by(tmp_path, S):
    img = GM.image(16, 14)
    src = tmp_path / "in.rgba"
    src.write_bytes(img.tobytes())
    a, b = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    common = ["-c", "2", "-s", "3", "--seed", "1", "--backdrop-fixed", "1,2,30", "--guided", "1", "--guided-shortlist", "8", "--calls", "14"]
    r = run_cli(str(src), a, *common, "--window", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("Guided sweep: 6 calls, ") == 2, r.stdout
    g = S.OptimizedImage(img, 2, 3, backdrop=True)
    g.backdrop = [1, 2, 30]
    g.initialize_tiles()
    g.recalculate_palettes()
    assert drive(S, g, 14, 1, 8, fixed=True) == 2
    assert np.array_equal(g.backdrop, [1, 2, 30]) and g.as_json() == open(a).read()
    g.close()
    r = run_cli(str(src), b, *common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(b).read() == open(a).read()
