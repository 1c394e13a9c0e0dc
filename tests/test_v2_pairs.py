"""At scale 0 a wave of the candidates' wide V pass sweeps TWO candidates in the channels whose class forms no SSIM map, and
fetches the source's a1 and r1 once for both ("Two candidates per wave").

Nothing a caller sees may move: every GPU comparison here is `array_equal` on the float64 errors of a context with the pairs on
(the default) and of one with SNES_V2_PAIR=0, which launches the single body on the grid it always had.

What the lists are chosen for:
  * partners are neighbours in the launch's order; without an order (lists up to 512) they are neighbours in the list, and
    their first changed groups lie anywhere in the picture.  Both then resume from B's checkpoint record min(gsA, gsB), and the
    later one sweeps B's own planes up to its first group: the equalities on the unordered lists pin the invariant that such a
    sweep reproduces B's record bit for bit;
  * a colour that wins no pixel, the slot's incumbent and a repeated colour give waves where neither partner, or only one, has
    an own group; an odd count leaves a last candidate without a partner;
  * SNES_DEBUG_POISON=1 fills the call's candidate storage with NaN bytes first: a paired wave that read a plane of a partner
    that the call did not write would show as a changed or non-finite error.
The image is that of tests/test_one_plane_h.py (a colour family per 64-column block), 256 wide.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP, SI = 0, 14
FAMILY = np.array([[200, 40, 40], [40, 200, 40], [40, 40, 200], [200, 200, 40]], np.int64)  # RGB8 centre per 64-column block
NOTHING, BLOCK0, BLOCK3 = (0, 0, 0), (22, 7, 7), (23, 27, 7)  # raw 5-bit candidates
HEIGHTS = (256, 64, 224)
REL_ERR = 1e-11  # the bar of tests/test_gpu_parity.py
OFF = {"SNES_V2_PAIR": "0"}


def image(h, seed=0):
    rng = np.random.default_rng(0x2E60 + h + 1000 * seed)
    out = np.zeros((h, 256, 4), np.uint8)
    base = FAMILY[np.arange(256) // 64][None, :, :]
    out[..., :3] = np.clip(base + rng.integers(-24, 25, (h, 256, 3)), 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def palette():
    """Subpalette 0 holds three or four entries per family; the other subpalettes are unused by the tiles."""
    pal = np.random.default_rng(77).integers(0, 32, (8 * 15, 3)).astype(np.uint8)
    c5 = FAMILY // 8
    rows = []
    for f in range(4):
        for d in ((0, 0, 0), (2, 0, 0), (0, 2, 0), (2, 2, 0)):
            rows.append(c5[f] + np.array(d))
    pal[:15] = np.array(rows[:15], np.uint8)
    return pal


def the_list(n, seed=5, si=SI):
    """n candidates around the four families; from four candidates on, one that wins nothing, one that wins in block 0, one
    that wins only in block 3, the incumbent and a repeated colour sit at fixed places."""
    rng = np.random.default_rng(seed)
    cand = np.clip((FAMILY // 8)[rng.integers(0, 4, n)] + rng.integers(-5, 6, (n, 3)), 0, 31).astype(np.uint8)
    if n >= 8:
        cand[1], cand[2], cand[n // 2], cand[n - 2] = NOTHING, BLOCK0, BLOCK3, palette()[SP * 15 + si]
        cand[3] = cand[n - 1] = (24, 26, 4)
    return cand


# ---- no GPU: the pyramids under test have a channel that pairs ---------------------------------------------------------------------
def header_weights():
    text = open(os.path.join(ROOT, "include", "ssimulacra2_constants.h")).read()
    body = re.search(r"#define SSIM2_WEIGHTS \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    return [float(v) for v in body.split(",")]


ACC_OF = [0, 2, 4, 1, 3, 5]  # weight order {ssim1, art1, det1, ssim4, art4, det4} -> bit of the pooling sum
SSIM_BITS, EDGE_BITS = 0x03, 0x3C


def sum_mask(w, ns, ch, s):
    return sum(1 << ACC_OF[e] for e in range(6) if w[(ch * ns + s) * 6 + e] != 0.0)


def scales_of(w_px, h_px):
    """The number of scales of a w x h image: ssimulacra2 tests the size before it downscales, and the downscale rounds up."""
    n, w, h = 1, w_px, h_px
    while n < 6 and not (w < 8 or h < 8):
        w, h, n = w // 2, (h + 1) // 2, n + 1
    return n


def pairing_channels(w, ns):
    """kSumMasks and the class rule of kernels.hpp restated: the instantiated masks are the distinct masks of the three widest
    scales of a six-scale pyramid and the full mask, a block runs the smallest that holds its own; a channel of scale 0 pairs
    where that one has no SSIM sum (and an edge sum)."""
    classes = []
    for ch in range(3):
        for s in range(3):
            m = sum_mask(w, 6, ch, s)
            if m not in classes:
                classes.append(m)
    classes.append(0x3F)
    out = set()
    for ch in range(3):
        need = sum_mask(w, ns, ch, 0)
        run = min((m for m in classes if m & need == need), key=lambda m: bin(m).count("1"))
        if not run & SSIM_BITS and run & EDGE_BITS:
            out.add("XYB"[ch])
    return out


def test_the_pyramids_under_test_have_a_pairing_channel():
    w = header_weights()
    assert len(w) == 108
    assert scales_of(256, 256) == 6 and scales_of(256, 224) == 6 and scales_of(256, 64) == 5
    assert pairing_channels(w, scales_of(256, 256)) == {"X", "B"}
    assert pairing_channels(w, scales_of(256, 224)) == {"X", "B"}
    assert pairing_channels(w, scales_of(256, 64)) == {"X"}


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


class env:
    """The switches are read when a context is created: set for as long as the variant's contexts are being made."""

    def __init__(self, monkeypatch, extra):
        self.mp, self.vars = monkeypatch, dict(extra)

    def __enter__(self):
        for k, v in self.vars.items():
            self.mp.setenv(k, v)

    def __exit__(self, *a):
        for k in self.vars:
            self.mp.delenv(k)


def context(S, h, **flags):
    g = S.OptimizedImage(image(h), 8, 15, **flags)
    g.tile_palettes = np.zeros(1024, np.uint8)
    g.palette = palette()
    g.optimize()
    return g


def scored(S, h, monkeypatch, switches, calls, **flags):
    """The errors of the calls (slot index, list), scored one after the other on one fresh context under the switches."""
    with env(monkeypatch, switches):
        g = context(S, h, **flags)
    out = [g.score_candidates(SP, si, c) for si, c in calls]
    g.close()
    return out


def on_equals_off(S, h, monkeypatch, calls, extra=None, **flags):
    extra = extra or {}
    on = scored(S, h, monkeypatch, extra, calls, **flags)
    off = scored(S, h, monkeypatch, dict(extra, **OFF), calls, **flags)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.dtype == np.float64 and a.shape == (len(calls[i][1]),) and np.all(np.isfinite(a)), i
        assert np.array_equal(a, b), (i, int(np.sum(a != b)))
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("h2q", [{}, {"SNES_H2Q_MAX": "0"}], ids=["quad-h", "long-h"])
def test_heights(S, h, h2q, monkeypatch):
    """Six scales (X and B pair), five (X alone) and a pyramid of odd heights; behind either H pass of a short list."""
    w = header_weights()
    if not pairing_channels(w, scales_of(256, h)):
        pytest.fail("every pyramid here is expected to pair; a table that changes this needs a test of the unpaired grid")
    on = on_equals_off(S, h, monkeypatch, [(SI, the_list(64, 5)), (SI, the_list(64, 9)), (SI, the_list(64, 9)[:5])], h2q)
    assert len(set(on[0].tolist())) >= 4  # nothing won, block 0, block 3 and the incumbent are four different images at least


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 64, 513, 1025])
def test_list_lengths(S, n, monkeypatch):
    """One, a pair, a pair and a single; 64 as listed (no order: partners start far apart); 513 in the V pass's order with an odd
    count; 1,025 with scale 0 on the side stream."""
    calls = [(SI, the_list(n, 20 + n))]
    if n <= 3:
        calls += [(SI, np.array([BLOCK0, BLOCK3, NOTHING][:n], np.uint8)), (SI, np.array([BLOCK3, NOTHING, BLOCK0][:n], np.uint8))]
    on_equals_off(S, 256, monkeypatch, calls)


@pytest.mark.gpu
def test_duplicates_and_candidates_without_a_group(S, monkeypatch):
    """Dedup on (repeated colours have no items: their waves take B's sums beside a live partner); the incumbent and colours that
    win nothing, next to each other and next to winners."""
    dup = the_list(64, 31)
    dup[10:20] = dup[0:10]
    dup[21], dup[22], dup[23] = NOTHING, palette()[SP * 15 + SI], NOTHING
    dup[40], dup[41] = BLOCK3, NOTHING
    dup[42], dup[43] = NOTHING, BLOCK0
    on = on_equals_off(S, 256, monkeypatch, [(SI, dup), (SI, np.array([NOTHING, NOTHING, NOTHING], np.uint8))], {"SNES_DEDUP_MIN": "8"})
    assert np.array_equal(on[0][10:20], on[0][0:10]) and on[0][21] == on[0][23] == on[0][1]
    assert np.all(on[1] == on[0][21])


@pytest.mark.gpu
def test_two_candidate_lists_on_many_slots(S, monkeypatch):
    """40 random pairs on the fifteen slots of the subpalette, on one context each way: partners whose first groups differ by
    anything up to the whole picture."""
    rng = np.random.default_rng(0x9A1)
    calls = []
    for i in range(40):
        pair = np.clip((FAMILY // 8)[rng.integers(0, 4, 2)] + rng.integers(-6, 7, (2, 3)), 0, 31).astype(np.uint8)
        calls.append((i % 15, pair))
    on = on_equals_off(S, 256, monkeypatch, calls)
    assert sum(1 for e in on if e[0] != e[1]) >= 8  # (a premise on the lists: pairs that do differ from each other)


@pytest.mark.gpu
def test_poisoned_storage(S, monkeypatch):
    calls = [(SI, the_list(67, 11)), (SI, the_list(3, 4)), (SI, the_list(1100, 13))]
    ref = scored(S, 256, monkeypatch, OFF, calls)
    got = scored(S, 256, monkeypatch, {"SNES_DEBUG_POISON": "1"}, calls)
    for a, b in zip(ref, got):
        assert np.all(np.isfinite(b)) and np.array_equal(a, b)


@pytest.mark.gpu
def test_against_the_oracle(S, O):
    cand = the_list(9, 17)
    g = context(S, 64)
    o = O.OracleImage(image(64), 8, 15)
    o.tile_palettes = np.zeros(1024, np.uint8)
    o.palette = palette()
    o.optimize()
    eg, eo = g.score_candidates(SP, SI, cand), o.score_candidates(SP, SI, cand)
    g.close()
    o.close()
    assert float(np.max(np.abs(eg - eo) / np.maximum(np.abs(eo), 1e-300))) < REL_ERR


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{"perceptual": True}, {"dither": True}], ids=["perceptual", "dither"])
def test_other_distances(S, flags, monkeypatch):
    on_equals_off(S, 256, monkeypatch, [(SI, the_list(67, 41))], **flags)
