"""At scale 0 the candidates' long H pass writes only mu2 and the XYB plane of the channels whose V class forms no SSIM map
("One-plane H items").

Nothing a caller sees may move: every GPU comparison here is on the raw bytes of the float64 errors (and of the committed
palettes), the default against SNES_H_PLANES=0 (three planes everywhere), against SNES_WEIGHT_MASK=0 (every sum, three planes)
and against the dense path (SNES_SPARSE=0).  SNES_DEBUG_POISON=1 fills a call's candidate storage with NaN bytes before the
call writes it: a read of a plane the H pass left out then shows as a changed or non-finite error instead of hiding behind
a stale finite value with a zero weight.  SNES_H2Q_MAX=0 everywhere, so that short lists take the long body under test.

The image is 256 wide and 32 or 256 high: three scales (X alone is SSIM-free at scale 0 — a table written for six scales
fails here) and six (X and B).  It is the one-colour-family-per-64-column-block image of tests/test_zero_weight_sums.py, so
that the first column block of a changed group is decided by the candidate's colour; `triples()` counts, on the remap of the
CPU oracle, the triples every (scale 0, first block) list of the H pass holds, and the premises below check that the lists
reach every kind of wave: all mixed, a ragged tail, pure waves of each class, and a start from a checkpoint.

The V pass's classes without an SSIM map fetch their map inputs an iteration ahead (sparse_v2_body, PRE); the V kernels run in
every comparison here, so the same equalities cover that: a single candidate and a list of 67 are among them.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP, SI = 0, 14  # the slot the lists are scored on
FAMILY = np.array([[200, 40, 40], [40, 200, 40], [40, 40, 200], [200, 200, 40]], np.int64)  # RGB8 centre per 64-column block
NOTHING, BLOCK0, BLOCK3 = (0, 0, 0), (22, 7, 7), (23, 27, 7)  # raw 5-bit candidates
HEIGHTS = (32, 256)
H2Q = {"SNES_H2Q_MAX": "0"}
VARIANTS = {
    "default": {},
    "three-planes": {"SNES_H_PLANES": "0"},
    "full-sums": {"SNES_WEIGHT_MASK": "0"},
    "dense": {"SNES_SPARSE": "0"},
    "default-poison": {"SNES_DEBUG_POISON": "1"},
    "three-planes-poison": {"SNES_H_PLANES": "0", "SNES_DEBUG_POISON": "1"},
}


def image(h, seed=0):
    rng = np.random.default_rng(0x2E60 + h + 1000 * seed)
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


def the_list(n, seed=5):
    """n candidates: random colours around the four families, with a colour that wins nothing, one that wins in block 0, one
    that wins only in block 3, the incumbent and a repeated colour at fixed places."""
    rng = np.random.default_rng(seed)
    cand = np.clip((FAMILY // 8)[rng.integers(0, 4, n)] + rng.integers(-5, 6, (n, 3)), 0, 31).astype(np.uint8)
    cand[1], cand[2], cand[n // 2], cand[n - 2] = NOTHING, BLOCK0, BLOCK3, palette()[SP * 15 + SI]
    cand[3] = cand[n - 1] = (24, 26, 4)
    return cand


# the three lists of every comparison, scored one after the other on ONE context (the storage of a call lies under the next)
def lists():
    return [the_list(64, 5), the_list(64, 9), the_list(64, 9)[:4]]


# ---- no GPU: the premises ---------------------------------------------------------------------------------------------------------
def header_weights():
    text = open(os.path.join(ROOT, "include", "ssimulacra2_constants.h")).read()
    body = re.search(r"#define SSIM2_WEIGHTS \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    return [float(v) for v in body.split(",")]


ACC_OF = [0, 2, 4, 1, 3, 5]  # weight order {ssim1, art1, det1, ssim4, art4, det4} -> bit of the pooling sum
SSIM_BITS = 0x03


def sum_mask(w, ns, ch, s):
    return sum(1 << ACC_OF[e] for e in range(6) if w[(ch * ns + s) * 6 + e] != 0.0)


def ssim_free_channels(w, ns):
    """Channels whose V block of scale 0 runs an instantiation without the SSIM map: the rule of kernels.hpp restated — the
    instantiated masks are the distinct masks of the three widest scales of a six-scale pyramid and the full mask, a block
    takes the smallest instantiated mask that holds its own."""
    classes = []
    for ch in range(3):
        for s in range(3):
            m = sum_mask(w, 6, ch, s)
            if m not in classes:
                classes.append(m)
    classes.append(0x3F)
    free = set()
    for ch in range(3):
        need = sum_mask(w, ns, ch, 0)
        run = min((m for m in classes if m & need == need), key=lambda m: bin(m).count("1"))
        if not run & SSIM_BITS:
            free.add("XYB"[ch])
    return free


def test_ssim_free_channels_of_scale_0_follow_the_number_of_scales():
    w = header_weights()
    assert len(w) == 108
    assert ssim_free_channels(w, 6) == {"X", "B"}  # 256 x 256
    for ns in (3, 4, 5):                           # 256 x 32, 256 x 64, 256 x 128
        assert ssim_free_channels(w, ns) == {"X"}, ns


def triples(h, cand):
    """Triples per first column block in the scale-0 lists of the H pass for `cand` on slot (SP, SI): one per (candidate,
    changed 4-row group), listed under the block of the group's leftmost won column less the filter's reach of four."""
    from oracle import oracle_py as O
    o = O.OracleImage(image(h), 8, 15)
    o.tile_palettes = np.zeros(1024, np.uint8)
    n = [0, 0, 0, 0]
    for c in cand:
        pal = palette()
        pal[SP * 15 + SI] = c
        o.palette = pal
        o.optimize()
        won = o.palette_map == SI
        for g in range(h // 4):
            xs = np.nonzero(won[4 * g:4 * g + 4].any(axis=0))[0]
            if len(xs):
                n[min(max(int(xs[0]) - 4, 0) >> 6, 3)] += 1
    o.close()
    return n


def test_the_lists_reach_every_kind_of_wave():
    counts = [n for h in HEIGHTS for cand in lists() for n in triples(h, cand)]
    assert any(0 < n < 6 for n in counts)              # 3 n < 16: the list's only wave holds all three channels
    assert any(n > 0 and (3 * n) % 16 for n in counts)  # a last wave with lanes that have no item
    assert any(n >= 33 for n in counts)                # pure waves of every class and both boundary waves
    for h in HEIGHTS:
        assert all(triples(h, cand)[3] > 0 for cand in lists()[:2]), h  # a start from B's checkpoint of block 3 (gs > 0)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


class env:
    """The switches are read when a context is created (the slot contexts of a window copy their parent's): set for as long as
    the variant's contexts live."""

    def __init__(self, monkeypatch, extra):
        self.mp, self.vars = monkeypatch, dict(H2Q, **extra)

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


def scored(S, h, monkeypatch, variant, cands, **flags):
    """The errors of the lists, scored one after the other on one fresh context of the variant."""
    with env(monkeypatch, VARIANTS[variant]):
        g = context(S, h, **flags)
        out = [g.score_candidates(SP, SI, c) for c in cands]
        g.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("flags", [{}, {"perceptual": True}, {"dither": True}], ids=["rgb", "perceptual", "dither"])
def test_one_plane_equals_three_planes_full_sums_and_dense(S, h, flags, monkeypatch):
    cands = lists()
    ref = scored(S, h, monkeypatch, "default", cands, **flags)
    for e, c in zip(ref, cands):
        assert e.dtype == np.float64 and e.shape == (len(c),) and np.all(np.isfinite(e))
    assert len(set(ref[0].tolist())) >= 4  # nothing won, block 0, block 3 and the incumbent are four different images at least
    for variant in VARIANTS:
        if variant == "default":
            continue
        got = scored(S, h, monkeypatch, variant, cands, **flags)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert np.all(np.isfinite(b)), (variant, i)
            assert a.tobytes() == b.tobytes(), (variant, i, int(np.sum(a != b)))


@pytest.mark.gpu
def test_one_candidate_and_a_ragged_list(S, monkeypatch):
    """A single candidate, and 67 (neither the items nor the pairs fill their last blocks), at six scales."""
    cands = [the_list(64, 5)[2:3], the_list(67, 11)]
    ref = scored(S, 256, monkeypatch, "default", cands)
    for variant in ("three-planes", "default-poison", "dense"):
        got = scored(S, 256, monkeypatch, variant, cands)
        for a, b in zip(ref, got):
            assert np.all(np.isfinite(b)) and a.tobytes() == b.tobytes(), variant


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
def test_a_long_call_with_the_two_stream_head(S, h, monkeypatch):
    """1,100 candidates: scale 0's H pass ahead on its own stream (grid-stride waves of both forms), duplicate colours."""
    cands = [the_list(1100, 13)]
    ref = scored(S, h, monkeypatch, "default", cands)
    for variant in ("default-poison", "three-planes", "full-sums"):
        got = scored(S, h, monkeypatch, variant, cands)
        assert np.all(np.isfinite(got[0])) and ref[0].tobytes() == got[0].tobytes(), variant


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
def test_slot_window_of_seven(S, h, monkeypatch):
    """Seven scheduled calls in one window (the kb_* shells through sparse_h2_dispatch; the slot contexts take the switches
    from their parent) against the same seven calls one by one, under every switch: errors, best colours, palette, map.  The
    single calls are the path the tests above hold against the dense one, so a window that read a plane its H pass left out,
    or that lost a switch on the way to its slot contexts and then met a poisoned store, differs from them."""
    sched = S.schedule(8, 15, 7)
    runs = {}
    for variant in ("default", "three-planes", "full-sums", "default-poison", "three-planes-poison"):
        with env(monkeypatch, VARIANTS[variant]):
            win, one = context(S, h), context(S, h)
            log, _, _ = win.run_slots(7, seed=1, first_step_id=0, state=(0, 0, 0, 0), window=7)
            errs = []
            for j, (method, p, idx, ch, _) in enumerate(sched):
                e, best = one.step(method, p, idx, ch, 1, j, 0)
                errs.append(e)
                assert np.array_equal(best, log[j][2]), (variant, j)
            e_win, e_one = np.array([r[0] for r in log], np.float64), np.array(errs, np.float64)
            assert np.all(np.isfinite(e_win)) and np.all(np.isfinite(e_one)), variant
            assert e_win.tobytes() == e_one.tobytes(), (variant, e_win, e_one)
            assert win.palette.tobytes() == one.palette.tobytes() and win.palette_map.tobytes() == one.palette_map.tobytes(), variant
            runs[variant] = (e_win.tobytes(), b"".join(np.asarray(r[2]).tobytes() for r in log), win.palette.tobytes(), win.palette_map.tobytes())
            win.close()
            one.close()
    for variant in runs:
        assert runs["default"] == runs[variant], variant


@pytest.mark.gpu
def test_image_batch_of_two(S, monkeypatch):
    """Two images through one launch per stage (kb_sparse_h2), five scheduled calls."""
    from snesimage_amd.throughput import ImageBatch
    runs = {}
    for variant in ("default", "three-planes", "default-poison"):
        with env(monkeypatch, VARIANTS[variant]):
            b = ImageBatch([(0, image(32)), (1, image(32, seed=1))], 8, 15, candidates=64, batched=True, groups=1)
            for m in b.images:
                m.tile_palettes = np.zeros(1024, np.uint8)
                m.palette = palette()
                m.optimize()
            b._open_batch()
            b.run(5)
            runs[variant] = b"".join(m.palette.tobytes() + m.palette_map.tobytes() for m in b.images)
            errs = np.asarray(b.errors(), np.float64)
            assert np.all(np.isfinite(errs)), variant
            runs[variant] += errs.tobytes()
            b.close()
    assert runs["default"] == runs["three-planes"]
    assert runs["default"] == runs["default-poison"]
