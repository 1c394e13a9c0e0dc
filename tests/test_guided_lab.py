"""The CIELAB proxy of guided calls (include/snesimage_hip.h: snesimage_set_guided_proxy; OptimizedImage.guided_proxy; DESIGN 5f'').

The model is tests/guided_lab_model.py: the definition over the CPU oracle's distance_cielab.  All 32,768 costs, shortlists,
palettes, maps and decisions agree bit for bit, errors within the project's 1e-11 relative.  tests/test_guided_lab_model.py shows
on the CPU that every picture and slot compared here has a CIELAB shortlist that differs from the redmean one, and that every
trajectory holds the gap premise and both accepts and rejects."""
import ctypes as C
import os

import numpy as np
import pytest

import guided_lab_model as LM
import guided_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_ERR = GM.REL_ERR
ERR_ARG, ERR_HIP, ERR_STATE, UNSUPPORTED = -1, -2, -3, -5


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def close(a, b):
    return abs(a - b) <= REL_ERR * abs(b)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_the_proxy_symbols():
    from snesimage_amd import _ffi
    text = open(os.path.join(ROOT, "include", "snesimage_hip.h")).read()
    bound = {n for n, _, _ in _ffi.SIGNATURES}
    lib = _ffi.load()
    for name in ("snesimage_set_guided_proxy", "snesimage_get_guided_proxy", "snesimage_shared_set_guided_proxy", "snesimage_shared_get_guided_proxy"):
        assert name + "(" in text and name in bound and getattr(lib, name) is not None
    assert "enum { SNES_GUIDE_REDMEAN = 0, SNES_GUIDE_CIELAB = 1 };" in text
    v = C.c_uint32(7)
    assert lib.snesimage_set_guided_proxy(None, 1) == ERR_ARG and lib.snesimage_get_guided_proxy(None, C.byref(v)) == ERR_ARG
    assert lib.snesimage_shared_set_guided_proxy(None, 1) == ERR_ARG and lib.snesimage_shared_get_guided_proxy(None, C.byref(v)) == ERR_ARG
    import snesimage_amd
    assert isinstance(snesimage_amd.OptimizedImage.guided_proxy, property) and isinstance(snesimage_amd.SharedPalette.guided_proxy, property)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

def context(S, m, proxy="cielab"):
    """A library context in the model's state."""
    g = S.OptimizedImage(m.img, m.C, m.S, backdrop=m.backdrop, **m.flags)
    if m.table is not None:
        g.set_ordered_dither(m.table)
    g.tile_palettes, g.palette = m.tile_palettes, m.palette
    if m.backdrop:
        g.backdrop = m.B
    g.optimize()
    g.guided_proxy = proxy
    return g


def assert_costs_equal(got, want, what):
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.shape == want.shape == (32768,)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of 32768 costs differ, first at u = %d: %d against %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def state(g):
    return (g.error(), g.palette.tobytes(), g.palette_map.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.TABLE_CASES))
def test_costs_and_shortlists_equal_the_model(S, O, name):
    """All 32,768 costs and the shortlists of 1, 16 and 64 with their costs, bit for bit: a population under one slice, ragged and
    whole slices, transparent tiles and pixels, a backdrop context's regular and tied slot, an ordered-dither target, and a
    context that is not perceptual."""
    m = LM.table_model(O, name)
    g = context(S, m)
    assert g.guided_proxy == "cielab"
    if name == "ordered":
        assert np.array_equal(g.target_rgba(), m.T) and not np.array_equal(m.T, m.img)
    if name == "transparent":
        assert (m.img[..., 3] == 0).sum() == 12 * 50 and (m.img[8:16, 104:144, 3] == 0).all()  # five whole tiles and parts of others
    before = state(g)
    for p, i in LM.TABLE_CASES[name][-1]:
        want = m.costs(p, i)
        assert_costs_equal(g.guided_costs(p, i), want, "%s slot (%d, %d)" % (name, p, i))
        cur = m.internal[m.entries(p, i)[0][0]]
        for k in (1, 16, 64):
            rgb5, c = g.guided_candidates(p, i, k)
            want_rgb5, want_c = GM.shortlist(want, cur, k)
            assert rgb5.shape == (k, 3) and np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c), (name, p, i, k)
            assert not any(np.array_equal(x, cur) for x in rgb5)
    assert state(g) == before, "the table and the shortlist changed the state"
    g.close()
    m.close()


@pytest.mark.gpu
def test_costs_of_a_one_entry_subpalette_have_no_floor(S, O):
    img, tp, pal = LM.no_floor_case()
    g = S.OptimizedImage(img, 2, 1, perceptual=True)
    g.tile_palettes, g.palette = tp, pal
    g.optimize()
    g.guided_proxy = "cielab"
    for p in (0, 1):
        want = LM.costs(O, img, tp, pal, 2, 1, p, 0)
        assert_costs_equal(g.guided_costs(p, 0), want, "2 x 1 slot (%d, 0)" % p)
        rgb5, c = g.guided_candidates(p, 0, 16)
        want_rgb5, want_c = GM.shortlist(want, pal[p], 16)
        assert np.array_equal(rgb5, want_rgb5) and np.array_equal(c, want_c)
    g.close()


def case_context(S, r, proxy="cielab"):
    g = S.OptimizedImage(r["img"], r["C"], r["S"], backdrop=r["backdrop"], **r["flags"])
    g.tile_palettes, g.palette = r["tp"], r["pal0"]
    if r["backdrop"]:
        g.backdrop = r["B0"]
    g.optimize()
    g.guided_proxy = proxy
    return g


def assert_state(g, rec, what):
    assert np.array_equal(g.palette, rec["palette"]), what
    if rec["B"] is not None:
        assert np.array_equal(g.backdrop, rec["B"]), what
    assert np.array_equal(g.palette_map, rec["pmap"]), what
    assert close(g.error(), rec["error"]), (what, g.error(), rec["error"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_guided_steps_follow_the_model(S, O, name):
    r = LM.trajectory(O, name)
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
@pytest.mark.parametrize("name", sorted(LM.CASES))
def test_two_guided_sweeps_follow_the_model(S, O, name):
    r = LM.trajectory(O, name)
    g = case_context(S, r)
    n = r["C"] * r["S"]
    assert len(r["recs"]) == 2 * n
    for rnd in range(2):
        log, stats = g.guided_sweep(r["K"])
        recs = r["recs"][rnd * n:(rnd + 1) * n]
        assert len(log) == n and stats["calls"] == n and stats["scored"] == n * r["K"] and stats["accepted"] == sum(c["changed"] for c in recs)
        for j, rec in enumerate(recs):
            assert log[j][1] == rec["best_k"] and np.array_equal(log[j][2], rec["rgb5"]) and log[j][3] == rec["changed"] and close(log[j][0], rec["error"]), (name, rnd, j)
        assert_state(g, recs[-1], "%s after sweep %d" % (name, rnd))
    g.close()


@pytest.mark.gpu
def test_redmean_again_is_todays_table_and_a_fresh_context_answers_redmean(S, O):
    m = LM.table_model(O, "ragged")
    fresh = context(S, m, "redmean")
    assert S.OptimizedImage(m.img, 2, 4).guided_proxy == "redmean"
    g = context(S, m, "cielab")
    lab = g.guided_costs(0, 1)
    assert_costs_equal(lab, m.costs(0, 1), "cielab")
    g.guided_proxy = "redmean"
    assert g.guided_proxy == "redmean"
    want = m.redmean_costs(0, 1)
    assert (want != lab).any()
    assert_costs_equal(g.guided_costs(0, 1), want, "redmean behind cielab")
    assert_costs_equal(fresh.guided_costs(0, 1), want, "redmean on a context that never saw cielab")
    for k in (1, 16, 64):
        a, b = g.guided_candidates(0, 1, k), fresh.guided_candidates(0, 1, k)
        w = GM.shortlist(want, m.internal[1], k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], w[0]) and np.array_equal(a[1], w[1])
    g.guided_proxy = "cielab"  # and back: the CIELAB list is still there
    assert_costs_equal(g.guided_costs(0, 1), m.costs(0, 1), "cielab again")
    with pytest.raises(ValueError):
        g.guided_proxy = "lab"
    assert g.guided_proxy == "cielab"
    g.close()
    fresh.close()
    m.close()


def refused(S, fn, code):
    with pytest.raises(S.SnesImageError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def set_proxy(g, name):
    g.guided_proxy = name


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(S, O):
    from hipmem import DeviceArray
    from snesimage_amd import _ffi
    L = _ffi.load()
    m = LM.table_model(O, "one-slice")
    # a NES context
    n = S.OptimizedImage(GM.image(16, 12), 2, 3, nes=True)
    n.initialize_tiles()
    n.recalculate_palettes()
    before = state(n)
    refused(S, lambda: set_proxy(n, "cielab"), UNSUPPORTED)
    assert n.guided_proxy == "redmean" and state(n) == before
    n.step(S.METHOD_NES, 0, 0)
    n.close()
    # a bad value
    g = context(S, m, "redmean")
    before = state(g)
    for v in (2, 0xFFFFFFFF):
        assert L.snesimage_set_guided_proxy(g._c, v) == ERR_ARG
    assert L.snesimage_get_guided_proxy(g._c, None) == ERR_ARG and g.guided_proxy == "redmean"
    # lent to a set
    g.set_chunk(64)
    sp = S.SharedPalette([g])
    refused(S, lambda: set_proxy(g, "cielab"), ERR_STATE)
    assert g.guided_proxy == "redmean"
    sp.close()
    # between the phases of a split-phase step
    buf = DeviceArray(64, np.float64, fill=0)
    g.step_begin(S.METHOD_RANDOM, 0, 0, 0, 1, 0, 64, 0, 1, buf.ptr)
    refused(S, lambda: set_proxy(g, "cielab"), ERR_STATE)
    assert g.guided_proxy == "redmean"
    g.step_commit(buf.ptr)
    # a failed allocation of the CIELAB list, on a context that holds the redmean workspace and on one that holds none: all or nothing
    g.palette = m.palette
    g.optimize()
    assert_costs_equal(g.guided_costs(1, 0), m.redmean_costs(1, 0), "redmean behind the refusals")
    g.guided_proxy = "cielab"
    twin = context(S, m, "cielab")
    for x in (g, twin):
        L.snesimage_debug_fail_alloc(0)
        try:
            assert "workspace" in refused(S, lambda: x.guided_costs(1, 0), ERR_HIP)
        finally:
            L.snesimage_debug_fail_alloc(-1)
        assert x.guided_proxy == "cielab"
        assert_costs_equal(x.guided_costs(1, 0), m.costs(1, 0), "cielab behind the refusals")
    assert state(g) == state(twin)
    g.close()
    twin.close()
    m.close()
