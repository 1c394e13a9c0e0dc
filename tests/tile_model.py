"""The model of objective-scored tile moves (include/snesimage_hip.h: "tile call", "tile sweep") over the unchanged CPU
oracle: tile_palettes setter + optimize() + error() per candidate, ascending subpalette, strict <."""
import numpy as np

REL_ERR = 1e-11
MIN_GAP = 1e-9  # premise of the comparisons: a candidate equals its incumbent exactly or differs by more than this (relative)


def make_pair(S, O, img, count, size, flags, slots=0, reassign=False):
    """A product context and an oracle in the same state: k-means start (a random state where k-means refuses the geometry), then `slots` scheduled calls, then reassign_tiles."""
    g = S.OptimizedImage(img, count, size, **flags)
    o = O.OracleImage(img, count, size, **flags)
    try:
        g.initialize_tiles()
        g.recalculate_palettes()
        o.initialize_tiles()
        o.recalculate_palettes()
    except S.SnesImageError as e:  # one-colour subpalettes: the k-means precondition 2 <= k < n fails (the reference panics there)
        assert e.code == -4
        rng = np.random.default_rng(count * 16 + size)
        tp = np.zeros(1024, np.uint8)
        ntile = 32 * (img.shape[0] // 8)
        tp[:ntile] = rng.integers(0, count, ntile)
        pal = rng.integers(0, 32, (count * size, 3), dtype=np.uint8)
        for x in (g, o):
            x.tile_palettes = tp
            x.palette = pal
            x.optimize()
    if slots:
        run_slots_both(S, g, o, count, size, 0, slots, bool(flags.get("nes")))
    if reassign:
        assert g.reassign_tiles() == o.reassign_tiles()
    assert np.array_equal(g.tile_palettes, o.tile_palettes) and np.array_equal(g.palette_map, o.palette_map)
    return g, o


def run_slots_both(S, g, o, count, size, first, n, nes=False, seed=5, n_random=8):
    """Calls first .. first + n - 1 of the reference's schedule on both (few random candidates: the oracle scores them one by one)."""
    sched = S.schedule(count, size, first + n + 1, nes)
    m, p, i, ch, st = sched[first]
    g.run_slots(n, seed=seed, first_step_id=first, state=(p, i, ch, st), n_random=n_random)
    for j in range(first, first + n):
        m, p, i, ch, _ = sched[j]
        o.step(m, p, i, ch, seed, j, n_random if m == 0 else 0)
    assert np.array_equal(g.palette, o.palette) and np.array_equal(g.palette_map, o.palette_map)


def model_candidate(o, tile, sub):
    """error() and palette_map of the oracle's state with `tile` drawn from `sub`; the oracle is left as it was."""
    tp, pm = o.tile_palettes, o.palette_map
    tp2 = tp.copy()
    tp2[tile] = sub
    o.tile_palettes = tp2
    o.optimize()
    e, m = o.error(), o.palette_map
    o.tile_palettes = tp
    o.palette_map = pm
    return e, m


def check_gap(e, inc):
    gap = abs(e - inc) / inc
    assert gap == 0.0 or gap > MIN_GAP, "the input breaks the premise: candidate %r against incumbent %r (gap %.3e)" % (e, inc, gap)


def model_tile_call(o, tile, sub_count, inc):
    """One tile call on the oracle -> (incumbent error after, the tile's subpalette after, changed)."""
    cur = int(o.tile_palettes[tile])
    best, best_k, best_map = inc, -1, None
    for k in range(sub_count):
        if k == cur:
            continue
        e, m = model_candidate(o, tile, k)
        check_gap(e, inc)
        if e < best:
            best, best_k, best_map = e, k, m
    if best_k >= 0:
        tp = o.tile_palettes.copy()
        tp[tile] = best_k
        o.tile_palettes = tp
        o.palette_map = best_map
    return best, (best_k if best_k >= 0 else cur), int(best_k >= 0)


def model_tile_sweep(o, first_tile, n_tiles, sub_count, inc=None):
    """-> list of (error, sub, changed), one per tile."""
    inc = o.error() if inc is None else inc
    log = []
    for t in range(first_tile, first_tile + n_tiles):
        inc, sub, ch = model_tile_call(o, t, sub_count, inc)
        log.append((inc, sub, ch))
    return log


def assert_log_matches(log, want):
    assert len(log) == len(want)
    for j, (r, (e, sub, ch)) in enumerate(zip(log, want)):
        assert int(r["sub"]) == sub and int(r["changed"]) == ch, (j, r, (e, sub, ch))
        assert abs(float(r["error"]) - e) <= REL_ERR * abs(e), (j, float(r["error"]), e)
