"""The CIELAB proxy on shared-palette sets (include/snesimage_hip.h: snesimage_shared_set_guided_proxy; SharedPalette.guided_proxy;
DESIGN 5f'').

The model is tests/guided_lab_model.py: the set's table is the integer sum of the members' CIELAB tables, everything else is
tests/set_guided_model.py.  Frames of 256 x 8 at (C, S) = (2, 4).  Costs and shortlists agree bit for bit, as do palettes, every
member's map and the decisions; errors within the project's 1e-11 relative.  tests/test_guided_lab_model.py shows on the CPU that
the trajectories (guided_lab_model.SET_CASES) hold the gap premise, accept and reject, and never meet the redmean shortlist."""
import numpy as np
import pytest

import guided_lab_model as LM
import guided_model as GM
import set_backdrop_model as SB

REL_ERR = 1e-11
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5
PERCEPTUAL = dict(perceptual=True)


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def close(a, b):
    return abs(a - b) <= REL_ERR * abs(b)


def make_set(S, imgs, Cn, Sz, flags=None, tiles=None, pal=None, B=None, proxy="cielab", chunk=64):
    """A set whose members hold the given tile palettes and regular entries; B: a backdrop set with that B."""
    ctxs = [S.OptimizedImage(f, Cn, Sz, backdrop=B is not None, **(flags or {})) for f in imgs]
    for j, c in enumerate(ctxs):
        c.set_chunk(chunk)
        if tiles is not None:
            c.tile_palettes = tiles[j]
        if pal is not None:
            c.palette = pal
        c.optimize()
    sp = S.SharedPalette(ctxs, backdrop=None if B is None else B)
    sp.guided_proxy = proxy
    return ctxs, sp


def model_set(S, m, proxy="cielab"):
    return make_set(S, m.imgs, m.C, m.S, m.flags, m.tiles, m.palette, m.B, proxy)


def close_all(sp, ctxs, m=None):
    sp.close()
    for c in ctxs:
        c.close()
    if m is not None:
        m.close()


def assert_costs_equal(got, want, what):
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.shape == want.shape == (32768,)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of 32768 costs differ, first at u = %d: %d against %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def state_of(sp, ctxs):
    return (sp.error(), [c.palette.tobytes() for c in ctxs], [c.tile_palettes.tobytes() for c in ctxs], [c.palette_map.tobytes() for c in ctxs])


@pytest.mark.gpu
@pytest.mark.parametrize("F", [2, 3])
def test_the_sets_table_is_the_integer_sum_of_the_members_tables(S, O, F):
    m = LM.SetModel(O, LM.frames(F, 8), 2, 4, PERCEPTUAL)
    ctxs, sp = model_set(S, m)
    assert sp.guided_proxy == "cielab" and all(c.guided_proxy == "redmean" for c in ctxs), "the set's setting is its own"
    before = state_of(sp, ctxs)
    for p, i in ((0, 1), (1, 3)):
        want = m.costs(p, i)
        members = [LM.costs(O, f, t, m.internal, 2, 4, p, i) for f, t in zip(m.imgs, m.tiles)]
        assert np.array_equal(want, np.sum(members, axis=0, dtype=np.uint64)) and all(x.any() for x in members)
        assert_costs_equal(sp.guided_costs(p, i), want, "%d x (256 x 8), slot (%d, %d)" % (F, p, i))
        cur = m.internal[p * 4 + i]
        for k in (1, 16, 64):
            rgb5, c = sp.guided_candidates(p, i, k)
            want_rgb5, want_c = GM.shortlist(want, cur, k)
            assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c), (F, p, i, k)
        assert not np.array_equal(GM.shortlist(want, cur, 16)[0], GM.shortlist(m.redmean_costs(p, i), cur, 16)[0])
    assert state_of(sp, ctxs) == before
    # redmean again: the table of the set's guided calls as they were
    sp.guided_proxy = "redmean"
    assert_costs_equal(sp.guided_costs(0, 1), m.redmean_costs(0, 1), "redmean behind cielab")
    assert all(c.guided_proxy == "redmean" for c in ctxs)
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_the_backdrop_slot_of_a_backdrop_set(S, O):
    imgs = LM.frames(2, 8)
    m = LM.SetModel(O, imgs, 2, 4, PERCEPTUAL, SB.stack_backdrop(O, imgs, PERCEPTUAL))
    ctxs, sp = model_set(S, m)
    assert np.array_equal(sp.backdrop, m.B) and np.array_equal(sp.palette, m.palette)
    for p, i, what in ((1, 1, "a regular slot"), (2, 0, "the tied slot")):
        want = m.costs(p, i)
        assert_costs_equal(sp.guided_costs(p, i), want, "backdrop set, " + what)
        rgb5, c = sp.guided_candidates(p, i, 16)
        want_rgb5, want_c = m.candidates(p, i, 16)
        assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c)
        cur = m.internal[m.entries(p, i)[0][0]]
        assert not np.array_equal(want_rgb5, GM.shortlist(m.redmean_costs(p, i), cur, 16)[0])
    without_b = np.sum([LM.costs(O, f, t, m.palette, 2, 4, 1, 1) for f, t in zip(m.imgs, m.tiles)], axis=0, dtype=np.uint64)
    assert (without_b != m.costs(1, 1)).any(), "B changes no floor: the case shows nothing"
    close_all(sp, ctxs, m)


@pytest.mark.gpu
def test_a_set_of_one_member_equals_that_context(S):
    img = LM.frames(1, 8)[0]
    g = S.OptimizedImage(img, 2, 4, perceptual=True)
    g.set_chunk(64)
    g.initialize_tiles()
    g.recalculate_palettes()
    g.guided_proxy = "cielab"
    own = [(g.guided_costs(p, i), g.guided_candidates(p, i, 16)) for p, i in ((0, 0), (1, 2))]
    twin = S.OptimizedImage(img, 2, 4, perceptual=True)
    twin.set_chunk(64)
    twin.tile_palettes, twin.palette = g.tile_palettes, g.palette
    twin.optimize()
    twin.guided_proxy = "cielab"
    g.guided_proxy = "redmean"  # the member's setting is not the set's
    sp = S.SharedPalette([g])
    assert sp.guided_proxy == "redmean"
    sp.guided_proxy = "cielab"
    assert g.guided_proxy == "redmean"
    for (p, i), (cost, (rgb5, c)) in zip(((0, 0), (1, 2)), own):
        assert_costs_equal(sp.guided_costs(p, i), cost, "a set of one, slot (%d, %d)" % (p, i))
        r2, c2 = sp.guided_candidates(p, i, 16)
        assert np.array_equal(r2, rgb5) and np.array_equal(c2, c)
    for p, i in ((0, 0), (1, 2), (0, 3)):
        e, best = sp.guided_step(p, i, 16)
        e2, best2 = twin.guided_step(p, i, 16)
        assert e == e2 and np.array_equal(best, best2) and sp.last_step()[1] == twin.last_step()[2]
        assert np.array_equal(g.palette, twin.palette) and np.array_equal(g.palette_map, twin.palette_map)
    close_all(sp, [g, twin])


def case_set(S, r):
    return make_set(S, r["imgs"], r["C"], r["S"], r["flags"], r["tiles"], r["pal0"], r["B0"])


def assert_state(sp, ctxs, rec, what):
    assert np.array_equal(sp.palette, rec["palette"]), what
    if rec["B"] is not None:
        assert np.array_equal(sp.backdrop, rec["B"]), what
    for c, pm in zip(ctxs, rec["pmaps"]):
        assert np.array_equal(c.palette, rec["palette"]) and np.array_equal(c.palette_map, pm), what
    assert close(sp.error(), rec["error"]), (what, sp.error(), rec["error"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.SET_CASES))
def test_guided_steps_follow_the_model(S, O, name):
    r = LM.set_trajectory(O, name)
    ctxs, sp = case_set(S, r)
    assert all(np.array_equal(c.palette_map, pm) and np.array_equal(c.tile_palettes, t) for c, pm, t in zip(ctxs, r["maps0"], r["tiles"])) and close(sp.error(), r["err0"])
    for j, rec in enumerate(r["recs"]):
        what = "%s call %d slot (%d, %d)" % (name, j, rec["p"], rec["i"])
        rgb5, cost = sp.guided_candidates(rec["p"], rec["i"], r["K"])
        assert np.array_equal(rgb5, rec["cand"]) and np.array_equal(cost, rec["costs"]), what
        err, best = sp.guided_step(rec["p"], rec["i"], r["K"])
        e2, k2, b2, ch2 = sp.last_step()
        print("%s: best_k %d (model %d), E %.9f (model %.9f)" % (what, k2, rec["best_k"], err, rec["error"]))
        assert k2 == rec["best_k"] and ch2 == rec["changed"] and np.array_equal(best, rec["rgb5"]) and np.array_equal(b2, rec["rgb5"]) and e2 == err and close(err, rec["error"]), what
        assert_state(sp, ctxs, rec, what)
    assert all(c.guided_proxy == "redmean" for c in ctxs)
    close_all(sp, ctxs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.SET_CASES))
def test_guided_sweep_follows_the_model(S, O, name):
    r = LM.set_trajectory(O, name)
    ctxs, sp = case_set(S, r)
    log, stats = sp.guided_sweep(r["K"])
    slots = [(p, i) for p in range(r["C"]) for i in range(r["S"])] + ([(r["C"], 0)] if r["backdrop"] else [])
    recs = r["recs"][:len(slots)]
    assert len(recs) == len(slots) == len(log) and stats["calls"] == len(slots) and stats["scored"] == len(slots) * r["K"]
    assert stats["accepted"] == sum(c["changed"] for c in recs) > 0
    for j, rec in enumerate(recs):
        assert (rec["p"], rec["i"]) == slots[j] and log[j][1] == rec["best_k"] and np.array_equal(log[j][2], rec["rgb5"]) and log[j][3] == rec["changed"] and close(log[j][0], rec["error"]), (name, j)
    assert_state(sp, ctxs, recs[-1], name + " after the sweep")
    close_all(sp, ctxs)


def refused(S, fn, code):
    with pytest.raises(S.SnesImageError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def set_proxy(x, name):
    x.guided_proxy = name


@pytest.mark.gpu
def test_refusals_leave_the_set_usable(S, O):
    from snesimage_amd import _ffi
    L = _ffi.load()
    r = LM.set_trajectory(O, "perceptual-f2-2x4")
    ctxs, sp = make_set(S, r["imgs"], r["C"], r["S"], r["flags"], r["tiles"], r["pal0"], None, "redmean")
    before = state_of(sp, ctxs)
    # a bad value, a null pointer
    for v in (2, 0xFFFFFFFF):
        assert L.snesimage_shared_set_guided_proxy(sp._s, v) == ERR_ARG
    assert L.snesimage_shared_get_guided_proxy(sp._s, None) == ERR_ARG and sp.guided_proxy == "redmean"
    with pytest.raises(ValueError):
        sp.guided_proxy = "lab"
    # a lent member's own setting stays refused
    refused(S, lambda: set_proxy(ctxs[0], "cielab"), ERR_STATE)
    # a failed allocation of the CIELAB list on a set that holds the redmean workspace: all or nothing
    sp.guided_costs(0, 0)
    sp.guided_proxy = "cielab"
    L.snesimage_debug_fail_alloc(0)
    try:
        assert "workspace" in refused(S, lambda: sp.guided_costs(0, 0), ERR_HIP)
    finally:
        L.snesimage_debug_fail_alloc(-1)
    assert sp.guided_proxy == "cielab" and state_of(sp, ctxs) == before
    # an NES set
    nctx = [S.OptimizedImage(f, 2, 3, nes=True) for f in r["imgs"]]
    for c in nctx:
        c.set_chunk(64)
    nsp = S.SharedPalette(nctx)
    nsp.initialize_tiles()
    nsp.recalculate_palettes()
    refused(S, lambda: set_proxy(nsp, "cielab"), UNSUPPORTED)
    assert nsp.guided_proxy == "redmean"
    nsp.step(S.METHOD_NES, 0, 0)
    close_all(nsp, nctx)
    # a member stepped outside the set: what every set call answers
    octx, osp = case_set(S, r)
    octx[1].step(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 16)
    refused(S, lambda: set_proxy(osp, "redmean"), ERR_STATE)
    assert osp.guided_proxy == "cielab"
    close_all(osp, octx)
    # after all of them a guided step still follows the model
    rec = r["recs"][0]
    err, best = sp.guided_step(rec["p"], rec["i"], r["K"])
    assert sp.last_step()[1] == rec["best_k"] and np.array_equal(best, rec["rgb5"]) and close(err, rec["error"])
    assert_state(sp, ctxs, rec, "behind the refusals")
    close_all(sp, ctxs)
