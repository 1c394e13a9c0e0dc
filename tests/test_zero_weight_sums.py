"""The candidates' wide V pass forms only the pooling sums whose weight in the score is not zero.

Nothing a caller sees may move: every GPU comparison here is on the raw bytes of the float64 errors (and of the committed
palettes), default against SNES_WEIGHT_MASK=0 (all six sums of every channel and scale, the path as it was) and against the
dense path (SNES_SPARSE=0), which never had a mask.

The image is 256 wide and 32 or 64 high.  At height 32 the pyramid is 256x32, 128x16 and 64x8 — three scales, all of them wide,
so the score walks the weights of (channel, scale) with a stride of three scales and not six: the masks of such an image are
not those of the table in DESIGN 4a, and the test would fail at once if the kernel took them from it.  Height 64 has four
scales, the last one narrow (the general body, which forms every sum).

The image has one colour family per 64-column block and every tile uses subpalette 0, so what a candidate of slot (0, 14) wins
is decided by its colour: `kinds()` checks, on the remap itself, that the list holds a colour that wins nothing, one that wins
pixels in column block 0 (all four waves of a channel pair sweep), one that wins only in block 3 (three of the four waves take
B's sums), the incumbent and a repeated colour.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP, SI = 0, 14  # the slot the lists are scored on
FAMILY = np.array([[200, 40, 40], [40, 200, 40], [40, 40, 200], [200, 200, 40]], np.int64)  # RGB8 centre per 64-column block
NOTHING, BLOCK0, BLOCK3 = (0, 0, 0), (22, 7, 7), (23, 27, 7)  # raw 5-bit candidates (kinds() checks what they win)


# ---- no GPU: the header's zero pattern is the one DESIGN 4a prints ------------------------------------------------------------
SUMS = ["ssim1", "art1", "det1", "ssim4", "art4", "det4"]  # the order of the six weights of one (channel, scale)


def header_weights():
    text = open(os.path.join(ROOT, "include", "ssimulacra2_constants.h")).read()
    body = re.search(r"#define SSIM2_WEIGHTS \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    return [float(v) for v in body.split(",")]


def design_table():
    """{channel: [set of sums per scale]} from the table of DESIGN 4a that follows the line naming SSIM2_WEIGHTS."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = text.index("<!-- zero-weight table -->")
    rows = {}
    for line in text[at:].splitlines()[1:]:
        if not line.startswith("|"):
            if rows:
                break
            continue
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if cells[0] in ("X", "Y", "B"):
            rows[cells[0]] = [set() if c in ("—", "-", "") else set(c.split()) for c in cells[1:]]
    return rows


def test_design_table_is_the_headers_zero_pattern():
    w = header_weights()
    assert len(w) == 108
    assert sum(1 for v in w if v == 0.0) == 56
    table = design_table()
    assert sorted(table) == ["B", "X", "Y"]
    for ch, name in enumerate("XYB"):
        assert len(table[name]) == 6
        for s in range(6):
            need = {SUMS[e] for e in range(6) if w[(ch * 6 + s) * 6 + e] != 0.0}
            assert table[name][s] <= set(SUMS), (name, s, table[name][s])
            assert table[name][s] == need, (name, s, sorted(table[name][s]), sorted(need))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


def image(h):
    rng = np.random.default_rng(0x2E60 + h)
    out = np.zeros((h, 256, 4), np.uint8)
    base = FAMILY[np.arange(256) // 64][None, :, :]
    out[..., :3] = np.clip(base + rng.integers(-24, 25, (h, 256, 3)), 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def palette():
    """Subpalette 0: three or four entries per family, the centre and neighbours on ONE side of it (a candidate on the other
    side then wins pixels); slot 14 is a colour of family 3.  The other subpalettes are unused by the tiles."""
    pal = np.random.default_rng(77).integers(0, 32, (8 * 15, 3)).astype(np.uint8)
    c5 = FAMILY // 8
    rows = []
    for f in range(4):
        for d in ((0, 0, 0), (2, 0, 0), (0, 2, 0), (2, 2, 0)):
            rows.append(c5[f] + np.array(d))
    pal[:15] = np.array(rows[:15], np.uint8)  # entries 12, 13, 14: family 3
    return pal


def context(S, h, monkeypatch, env=None, pal=None, **flags):
    """A context with every tile on subpalette 0, created with `env` in the environment (the switches are read at creation)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    g = S.OptimizedImage(image(h), 8, 15, **flags)
    for k in (env or {}):
        monkeypatch.delenv(k)
    g.tile_palettes = np.zeros(1024, np.uint8)
    g.palette = palette() if pal is None else pal
    g.optimize()
    return g


def the_list(n, seed=5):
    """n candidates: random colours, with the five kinds of the docstring at fixed places (the repeat twice, far apart)."""
    rng = np.random.default_rng(seed)  # colours around the four families, so that most of them win pixels somewhere
    cand = np.clip((FAMILY // 8)[rng.integers(0, 4, n)] + rng.integers(-5, 6, (n, 3)), 0, 31).astype(np.uint8)
    cand[1], cand[2], cand[n // 2], cand[n - 2] = NOTHING, BLOCK0, BLOCK3, palette()[SP * 15 + SI]
    cand[3] = cand[n - 1] = (24, 26, 4)
    return cand


@pytest.fixture(scope="module")
def kinds(S):
    """What NOTHING, BLOCK0 and BLOCK3 win at either height, read off the remap with the colour in the slot."""
    mp = pytest.MonkeyPatch()
    out = {}
    for h in (32, 64):
        for c in (NOTHING, BLOCK0, BLOCK3):
            pal = palette()
            pal[SP * 15 + SI] = c
            g = context(S, h, mp, pal=pal)
            won = np.argwhere(g.palette_map == SI)
            out[h, c] = sorted({int(x) // 64 for _, x in won})
            g.close()
    mp.undo()
    return out


def three_ways(S, h, n, monkeypatch, **flags):
    cand = the_list(n)
    res = []
    for env in (None, {"SNES_WEIGHT_MASK": "0"}, {"SNES_SPARSE": "0"}):
        g = context(S, h, monkeypatch, env, **flags)
        res.append(g.score_candidates(SP, SI, cand))
        g.close()
    masked, full, dense = res
    assert masked.dtype == np.float64 and np.all(np.isfinite(masked))
    assert masked.tobytes() == full.tobytes(), int(np.sum(masked != full))
    assert masked.tobytes() == dense.tobytes(), int(np.sum(masked != dense))
    assert masked[3] == masked[n - 1]  # the repeated colour
    return masked


@pytest.mark.gpu
@pytest.mark.parametrize("h", [32, 64])
def test_the_lists_hold_what_they_are_meant_to(kinds, h):
    assert kinds[h, NOTHING] == []
    assert 0 in kinds[h, BLOCK0]
    assert kinds[h, BLOCK3] == [3]


@pytest.mark.gpu
@pytest.mark.parametrize("h", [32, 64])
@pytest.mark.parametrize("n", [64, 600, 1024], ids=["h2q-64", "h2-600", "two-streams-dedup-1024"])
def test_masked_equals_full_equals_dense(S, h, n, monkeypatch):
    e = three_ways(S, h, n, monkeypatch)
    assert len(set(e.tolist())) >= 4  # nothing won, block 0, block 3 and the incumbent are four different images at least


@pytest.mark.gpu
@pytest.mark.parametrize("h", [32, 64])
@pytest.mark.parametrize("flags", [{"perceptual": True}, {"dither": True}], ids=["perceptual", "dither"])
def test_perceptual_and_dither_share_the_scorer(S, h, flags, monkeypatch):
    three_ways(S, h, 600, monkeypatch, **flags)


@pytest.mark.gpu
@pytest.mark.parametrize("h", [32, 64])
def test_no_stale_sums_between_calls(S, h, monkeypatch):
    """The 1,024-list on one slot, then a 64-list on another slot of the same context: the second call reuses the storage of
    the first's candidates 0..63, and a sum that the masked body did not form must not be what the first call left there."""
    used, fresh = context(S, h, monkeypatch), context(S, h, monkeypatch)
    used.score_candidates(SP, SI, the_list(1024))
    short = the_list(64, seed=9)
    a, b = used.score_candidates(SP, 3, short), fresh.score_candidates(SP, 3, short)
    assert a.tobytes() == b.tobytes(), int(np.sum(a != b))
    used.close()
    fresh.close()


@pytest.mark.gpu
def test_slot_window_equals_call_by_call_under_both_settings(S, monkeypatch):
    """Twelve scheduled calls at height 32 in one window (the kb_* shells) against twelve single calls, with and without the
    mask: the errors after every call and the committed palette and map, as bytes."""
    sched = S.schedule(8, 15, 12)
    runs = {}
    for name, env in (("masked", None), ("full", {"SNES_WEIGHT_MASK": "0"})):
        win, one = context(S, 32, monkeypatch, env), context(S, 32, monkeypatch, env)
        log, _, _ = win.run_slots(12, seed=1, first_step_id=0, state=(0, 0, 0, 0), window=12)
        errs = []
        for j, (method, p, idx, ch, _) in enumerate(sched):
            e, best = one.step(method, p, idx, ch, 1, j, 0)
            errs.append(e)
            assert np.array_equal(best, log[j][2]), (name, j)
        e_win, e_one = np.array([r[0] for r in log], np.float64), np.array(errs, np.float64)
        assert e_win.tobytes() == e_one.tobytes(), (name, e_win, e_one)
        assert win.palette.tobytes() == one.palette.tobytes() and win.palette_map.tobytes() == one.palette_map.tobytes(), name
        runs[name] = (e_win.tobytes(), win.palette.tobytes(), win.palette_map.tobytes())
        win.close()
        one.close()
    assert runs["masked"] == runs["full"]
