"""The oracle's restatement of `error()` (lib.rs:503-548) against an independent binary64 model (tests/ssim2_model.py), stage
by stage, and the HIP path's whole score against that model.

Oracle and kernels were written from the same appendix, so a mistake of that appendix's reading passes every oracle-versus-
kernel test.  The model is a second reading: numpy, binary64, the blur's taps from the filter design instead of a recurrence.
The whole score is a blunt instrument (two neighbouring weights exchanged move it by 6e-8), so the comparison is made where
binary32 and binary64 agree to about 1e-6: XYB planes, blurred planes, pooled statistics, the score as a function of given
statistics, and only then the whole.

BARS.  Each bar is 4 x the largest value the oracle-versus-model comparison gave over the whole case table (PICTURES x HEIGHTS
x RECONSTRUCTIONS, measured on the CPU, never on the GPU); binary32 rounding varies with content by about that factor between
cases, and a planted mistake sits 100 x or more above (test_planted_errors_are_seen asserts 10 x the bar).  The measured value
stands beside each constant; DESIGN section 2 carries the same table.
"""
import numpy as np
import pytest

import adversarial_images as A
import ssim2_model as M

# stage: (measured maximum over the case table, bar = 4 x measured)
XYB_ABS = (7.49e-7, 3.0e-6)    # stage 1: positive XYB planes of every scale, maximum absolute difference
TAPS_ABS = (1.36e-7, 5.5e-7)    # stage 2: taps of the design against the oracle's FIR (binary32 taps)
BLUR_ABS = (4.05e-6, 1.62e-5)    # stage 2: recursive blur (the product's) against the model, planes in [0, 1.3]
BLUR_FIR_ABS = (9.91e-7, 4.0e-6)  # stage 2: the oracle's FIR mode against the model
STATS_FIR_REL = (6.01e-3, 2.4e-2)  # stage 3: statistics, oracle in FIR mode, relative (see stats_rel)
STATS_REC_REL = (1.12e-2, 4.5e-2)  # stage 3: statistics, oracle in recursive mode (the product's), coarse reconstructions
SCORE_REL = (1.5e-15, 6.0e-15)   # stage 4: error from the ORACLE's statistics, binary64 on both sides
WHOLE_REL = (2.86e-4, 1.15e-3)   # stage 5: whole error, oracle in recursive mode, where FIR and recursive agree within PREMISE
PREMISE = 2e-4                # stage 5 runs where the recursion's binary32 noise is below this (asserted)
TEETH = 10.0                  # a planted mistake must reach TEETH x bar on some stage of some case

# A pooled statistic is a mean of per-pixel values 1 - (a ratio near 1) formed in binary32, so whatever its size it carries an
# absolute error of the order of 2^-24 = 6e-8 per pixel; a relative difference is asked for values above STATS_FLOOR only,
# smaller ones are measured against the floor.  (Where the model gives exactly 0 the oracle must too: no floor there.)
STATS_FLOOR = 1e-4

HEIGHTS = (8, 24, 40, 56, 72, 136, 256)
ROWS = {8: (8, 4), 24: (24, 12, 6), 40: (40, 20, 10, 5), 56: (56, 28, 14, 7), 72: (72, 36, 18, 9, 5), 136: (136, 68, 34, 17, 9, 5),
        256: (256, 128, 64, 32, 16, 8)}
PICTURES = ("synth", "two_tone", "lab_extremes", "alpha_mix")
RECONSTRUCTIONS = ("levels8", "levels4", "levels2", "noise2")
COARSE = ("levels4", "levels2")  # the reconstructions stage 5 is asserted on


def picture(name, h):
    if name == "synth":
        from snesimage_amd.synth import synth_image
        return synth_image(0x5EED0100 + h, 256, h, 0)
    if name == "alpha_mix":
        return A.alpha_mix(max(h, 16))[:h].copy()  # alpha_mix marks single pixels of tile row 1
    return getattr(A, name)(h)


def reconstruction(src, kind):
    """What as_rgba() could return for `src`: each channel quantised to 8, 4 or 2 levels, or moved by a value in -2 .. 2;
    transparent pixels black with alpha 0 (lib.rs:550-577)."""
    rgb = src[..., :3].astype(np.int64)
    if kind == "noise2":
        rgb = np.clip(rgb + np.random.default_rng(src.shape[0]).integers(-2, 3, rgb.shape), 0, 255)
    else:
        n = int(kind[6:]) - 1
        rgb = (2 * rgb * n + 255) // 510 * 255 // n  # round to the nearest of n + 1 levels, then back to 8 bits (floor)
    out = np.zeros_like(src)
    out[..., :3] = rgb
    out[..., 3] = 255
    out[src[..., 3] == 0] = 0
    return out


def rel(a, b):
    return abs(a - b) / abs(b)


def planes_abs(got, want):
    """Maximum absolute difference of two pyramids; infinite where the number of scales or a scale's size differs."""
    if len(got) != len(want) or any(a.shape != b.shape for a, b in zip(got, want)):
        return float("inf")
    return max(float(np.max(np.abs(a - b))) for a, b in zip(got, want))


def stats_rel(oracle, model):
    """Largest |oracle - model| / max(|model|, STATS_FLOOR); infinite where the shapes differ or where the model's value is
    exactly 0 and the oracle's is not."""
    oracle, model = np.asarray(oracle), np.asarray(model)
    if oracle.shape != model.shape or np.any((model == 0.0) & (oracle != 0.0)) or not np.all(np.isfinite(model)):
        return float("inf")
    return float(np.max(np.abs(oracle - model) / np.maximum(np.abs(model), STATS_FLOOR)))


class Case:
    """One (picture, height, reconstruction): the oracle's stage outputs, kept for every test of this module."""

    def __init__(self, O, name, h, kind, src, src_planes):
        self.id, self.kind, self.h = "%s-%d-%s" % (name, h, kind), kind, h
        self.src, self.dst = src, reconstruction(src, kind)
        self.o_src = src_planes
        self.o_dst = O.xyb_pyramid(self.dst)
        self.o_stats = {mode: O.scale_stats(self.src, self.dst, mode) for mode in (0, 1)}  # 0 recursive, 1 FIR
        self.o_error = {mode: 100.0 - O.ssimulacra2_rgba(self.src, self.dst, mode) for mode in (0, 1)}

    def measure(self, model):
        """{stage: value} of `model` (the model proper, or one with a planted mistake) against the oracle."""
        m_src, m_dst = model.pyramid(self.src), model.pyramid(self.dst)
        out = {"xyb": max(planes_abs(self.o_src, m_src), planes_abs(self.o_dst, m_dst))}
        out["score"] = rel(100.0 - model.score_from_stats(self.o_stats[0]), self.o_error[0])
        if len(m_src) != len(self.o_src):
            out["stats_fir"] = out["stats_rec"] = out["whole"] = float("inf")
            return out
        m_stats = np.array([model.scale_stats(a, b) for a, b in zip(m_src, m_dst)])
        out["stats_fir"] = stats_rel(self.o_stats[1], m_stats)
        out["stats_rec"] = stats_rel(self.o_stats[0], m_stats)
        out["whole"] = rel(100.0 - model.score_from_stats(m_stats), self.o_error[0])
        out["zeros"] = int(np.sum(m_stats == 0.0))
        return out

    @property
    def premise(self):
        return rel(self.o_error[1], self.o_error[0])


@pytest.fixture(scope="module")
def table(O):
    cases = []
    for h in HEIGHTS:
        for name in PICTURES:
            src = picture(name, h)
            planes = O.xyb_pyramid(src)
            assert tuple(p.shape[1] for p in planes) == ROWS[h] and planes[-1].shape[2] == 256 >> (len(planes) - 1)
            cases += [Case(O, name, h, kind, src, planes) for kind in RECONSTRUCTIONS]
    return cases


@pytest.fixture(scope="module")
def measured(table):
    """The model proper against the oracle on every case, printed (run with -s to see the figures the bars come from)."""
    model = M.Model()
    out = [(c, c.measure(model)) for c in table]
    for key in ("xyb", "stats_fir", "stats_rec", "score", "whole"):
        for label, kinds in (("coarse", COARSE), ("near-exact", ("levels8", "noise2"))):
            c, m = max(((c, m) for c, m in out if c.kind in kinds), key=lambda cm: cm[1][key])
            print("%-9s %-10s max %.3e at %s" % (key, label, m[key], c.id))
    for label, kinds in (("coarse", COARSE), ("near-exact", ("levels8", "noise2"))):
        sel = [c for c, _ in out if c.kind in kinds]
        print("%-10s FIR against recursive: max %.3e; error() %.1f .. %.1f" % (
            label, max(c.premise for c in sel), min(c.o_error[0] for c in sel), max(c.o_error[0] for c in sel)))
    return out


# ---- stage 2 first: it needs no picture ---------------------------------------------------------------------------------------
def blur_shapes():
    shapes = {(8, 8)}
    for rows in ROWS.values():
        shapes |= {(r, 256 >> s) for s, r in enumerate(rows)}
    return sorted(shapes)


def border_split(diff):
    """(largest difference in the first and last four rows and columns, largest elsewhere)."""
    inner = diff[4:-4, 4:-4]
    edge = diff.copy()
    edge[4:-4, 4:-4] = 0.0
    return float(edge.max()), float(inner.max()) if inner.size else 0.0


def test_blur_taps_follow_the_design(O):
    """The taps of the truncated-cosine design at sigma = 1.5, radius 5: they sum to 1, their second moment is sigma^2, they
    differ from a sampled Gaussian by 1.8e-3 to 1.9e-3 (so the two cannot be mistaken), and the oracle's FIR is these taps."""
    taps = M.blur_taps()
    n = np.arange(-4, 5)
    assert taps.size == 9 and np.allclose(taps, taps[::-1], rtol=0, atol=1e-16)
    assert abs(taps.sum() - 1.0) < 1e-14 and abs((taps * n * n).sum() - 1.5 ** 2) < 1e-13
    gauss = M.Model("true_gaussian").blur_taps()
    assert 1.5e-3 < np.max(np.abs(gauss - taps)) < 2.5e-3
    fir = O.blur_constants()[2].astype(np.float64)
    d = float(np.max(np.abs(fir - taps)))
    print("taps: oracle FIR against the design %.3e" % d)
    assert d <= TAPS_ABS[1]


def test_blur_matches_the_zero_padded_fir_borders_included(O, table):
    """O.blur_plane (recursive, and the FIR mode) against blur(): random planes in [0, 1] at every plane shape the heights
    produce and 8 x 8, and the real planes img, img^2 and img1 * img2 of one case at each of its scales."""
    rng = np.random.default_rng(0x2B1)
    planes = [rng.random(shape).astype(np.float32) for shape in blur_shapes()]
    case = next(c for c in table if c.id == "lab_extremes-136-levels4")
    for a, b in zip(case.o_src, case.o_dst):
        planes += [a[1], a[1] * a[1], a[0] * b[0], a[2] * b[2]]
    worst = {0: [0.0, 0.0], 1: [0.0, 0.0]}
    for p in planes:
        want = M.blur(p)
        for mode in (0, 1):
            edge, inner = border_split(np.abs(O.blur_plane(p, mode) - want))
            worst[mode] = [max(worst[mode][0], edge), max(worst[mode][1], inner)]
    print("blur: recursive borders %.3e interior %.3e; FIR mode borders %.3e interior %.3e" % (*worst[0], *worst[1]))
    assert max(worst[0]) <= BLUR_ABS[1]
    assert max(worst[1]) <= BLUR_FIR_ABS[1]


# ---- stages 1, 3, 4, 5 -----------------------------------------------------------------------------------------------------------
def test_xyb_pyramid(measured):
    assert max(m["xyb"] for _, m in measured) <= XYB_ABS[1]


def test_statistics_per_scale(measured):
    """The 18 statistics of every scale, against the oracle in FIR mode and in recursive mode (the product's).  sigma - mu^2
    is a difference of binary32 values near 0.3 divided by something as small as C2 = 0.0009, so a statistic carries the
    planes' 1e-6 several hundred times over, and more as the pictures approach each other: asserted on the reconstructions
    stage 5 is asserted on, printed for the others.  two_tone provides statistics that are exactly 0 in the model (stats_rel
    is infinite where the oracle's is not 0 there)."""
    coarse = [m for c, m in measured if c.kind in COARSE]
    assert max(m["stats_fir"] for m in coarse) <= STATS_FIR_REL[1]
    assert max(m["stats_rec"] for m in coarse) <= STATS_REC_REL[1]
    assert all(np.isfinite(m["stats_rec"]) and np.isfinite(m["stats_fir"]) for _, m in measured)
    assert sum(m["zeros"] for c, m in measured if c.id.startswith("two_tone") and c.kind in COARSE) > 0


def test_score_from_the_oracles_statistics(measured):
    """2, 3, 4, 5 and 6 scales: the weights are consumed contiguously over the scales present."""
    assert {len(c.o_stats[0]) for c, _ in measured} == {2, 3, 4, 5, 6}
    assert max(m["score"] for _, m in measured) <= SCORE_REL[1]


def test_whole_error(measured):
    coarse = [(c, m) for c, m in measured if c.kind in COARSE]
    assert len(coarse) == len(HEIGHTS) * len(PICTURES) * len(COARSE)
    for c, m in coarse:
        assert c.premise <= PREMISE, (c.id, c.premise)
        assert m["whole"] <= WHOLE_REL[1], (c.id, m["whole"])


# ---- teeth ------------------------------------------------------------------------------------------------------------------------
BARS = {"xyb": XYB_ABS[1], "stats_fir": STATS_FIR_REL[1], "score": SCORE_REL[1], "whole": WHOLE_REL[1]}


def seen(values, coarse):
    """The stage on which {stage: value} reaches TEETH x its bar, or None; stages 3 and 5 count where they are asserted."""
    return next((k for k, bar in BARS.items() if values[k] >= TEETH * bar and (coarse or k in ("xyb", "score"))), None)


def test_planted_errors_are_seen(O, table):
    """Every mistake of ssim2_model.PLANTS, planted in the MODEL one at a time, moves some stage on some case to 10 x that
    stage's bar or more; so does each exchange of two neighbouring non-zero weights, at stage 4."""
    rng = np.random.default_rng(0x7EE7)
    plane = rng.random((9, 32)).astype(np.float32)
    where = {}
    for plant in M.PLANTS:
        model = M.Model(plant)
        if float(np.max(np.abs(O.blur_plane(plane, 0) - model.blur(plane)))) >= TEETH * BLUR_ABS[1]:
            where[plant] = ("blur", "9x32")
            continue
        for c in table:  # ordered by height: the cheap cases first
            if c.h > 136:
                break
            stage = seen(c.measure(model), c.kind in COARSE)
            if stage:
                where[plant] = (stage, c.id)
                break
    print("planted:", where)
    assert sorted(where) == sorted(M.PLANTS), sorted(set(M.PLANTS) - set(where))
    nonzero = np.flatnonzero(M.WEIGHTS)
    swaps = list(zip(nonzero[:-1], nonzero[1:]))
    assert len(swaps) == 51
    six = [c for c in table if c.h == 256]
    least = []
    for swap in swaps:
        model = M.Model(weight_swap=swap)
        least.append(max(rel(100.0 - model.score_from_stats(c.o_stats[0]), c.o_error[0]) for c in six))
    print("weight swaps: the least visible moves stage 4 by %.3e" % min(least))
    assert min(least) >= TEETH * SCORE_REL[1]


# ---- GPU: the HIP path's whole error against the model -----------------------------------------------------------------------------
GEOMETRIES = ((2, 3), (4, 7))
GPU_CASES = [(h, g) for h in HEIGHTS[:-1] for g in GEOMETRIES] + [(256, (4, 7))]
SLOT = (1, 2)


def coarse_palette(count, size, h):
    """5-bit entries from {0, 10, 21, 31}: far enough from any picture that FIR and recursive blur agree (the premise)."""
    levels = np.array([0, 10, 21, 31], np.uint8)
    return levels[np.random.default_rng(1000 * count + h).integers(0, 4, (count * size, 3))]


def rebuild(src, tile_palettes, palette, size, pmap):
    """as_rgba() in numpy (lib.rs:550-577): the 5 -> 8-bit expansion v * 8 + v / 4 of the entry each pixel's map value
    selects in its tile's subpalette; pixels whose source alpha is 0 stay (0, 0, 0, 0)."""
    h = src.shape[0]
    y, x = np.mgrid[0:h, 0:256]
    entry = tile_palettes[(y // 8) * 32 + x // 8].astype(np.int64) * size + pmap
    p5 = palette.astype(np.int64)[entry]
    out = np.zeros_like(src)
    out[..., :3] = p5 * 8 + p5 // 4
    out[..., 3] = 255
    out[src[..., 3] == 0] = 0
    return out


def model_error(src_planes, dst):
    stats = np.array([M.scale_stats(a, b) for a, b in zip(src_planes, M.pyramid(dst))])
    return 100.0 - M.score_from_stats(stats)


@pytest.mark.gpu
@pytest.mark.parametrize("h,geometry", GPU_CASES, ids=["%d-%dx%d" % (h, c, s) for h, (c, s) in GPU_CASES])
def test_gpu_error_and_candidates_against_the_model(O, h, geometry, monkeypatch):
    """error() of a hand-set state, and score_candidates of 8 colours (the incumbent, black and white among them) on the
    group-sparse path and on the dense one, against the model on (source, reconstruction rebuilt from the returned map)."""
    import snesimage_amd as S
    from hipmem import DeviceArray
    count, size = geometry
    sp, si = SLOT
    src = picture("alpha_mix" if count == 4 else "synth", h)
    src_planes = M.pyramid(src)
    tiles, pal = A.hand_tiles(count), coarse_palette(count, size, h)
    cand = S.random_candidates(11, h + count, 8)
    cand[0], cand[1], cand[2] = pal[sp * size + si], (0, 0, 0), (31, 31, 31)

    def premise(dst):
        return rel(100.0 - O.ssimulacra2_rgba(src, dst, 1), 100.0 - O.ssimulacra2_rgba(src, dst, 0))

    got = {}
    for path, env in (("sparse", "1"), ("dense", "0")):
        monkeypatch.setenv("SNES_SPARSE", env)
        g = S.OptimizedImage(src, count, size)
        g.tile_palettes, g.palette = tiles, pal
        g.optimize()
        if path == "sparse":
            dst = g.as_rgba()
            assert np.array_equal(dst, rebuild(src, tiles, pal, size, g.palette_map))
            assert premise(dst) <= PREMISE
            e_gpu, e_model = g.error(), model_error(src_planes, dst)
            print("error() %.6f, model %.6f, rel %.3e" % (e_gpu, e_model, rel(e_gpu, e_model)))
            assert rel(e_gpu, e_model) <= WHOLE_REL[1]
        d_c, d_e = DeviceArray.from_numpy(cand), DeviceArray(8, np.float64, fill=0)
        d_m = DeviceArray((8, h, 256), np.uint8, fill=255)
        if path == "sparse":  # asking for maps takes the dense path: the errors from the sparse one, the maps from the remap alone
            errors = g.score_candidates(sp, si, cand)
            g.remap_candidates_device(sp, si, d_c.ptr, 8, d_m.ptr)
        else:
            g.score_candidates_device(sp, si, d_c.ptr, 8, d_e.ptr, d_m.ptr)
        g.sync()
        got[path] = (errors if path == "sparse" else d_e.numpy(), d_m.numpy())
        for d in (d_c, d_e, d_m):
            d.free()
        g.close()
    assert np.array_equal(got["sparse"][1], got["dense"][1])
    for k in range(8):
        p = pal.copy()
        p[sp * size + si] = cand[k]
        dst = rebuild(src, tiles, p, size, got["dense"][1][k])
        assert premise(dst) <= PREMISE, k
        e_model = model_error(src_planes, dst)
        for path in ("sparse", "dense"):
            r = rel(got[path][0][k], e_model)
            print("candidate %d %s: %.6f, model %.6f, rel %.3e" % (k, path, got[path][0][k], e_model, r))
            assert r <= WHOLE_REL[1], (k, path)
