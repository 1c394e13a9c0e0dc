"""The candidates' long H pass in a kernel per form ("One kernel per form"; SNES_H_FORMS).

Which code shares a kernel is all that changes: no operation, operand or order.  So every comparison here is on the raw bytes
of the float64 errors (and of the committed palettes), SNES_H_FORMS=0 — the kernels that hold every form — against each single
bit and the full mask, and the full mask against the dense path, a poisoned store, three planes everywhere and every sum.

SNES_H2Q_MAX=0 and SNES_H0_MIN=16 everywhere unless a variant says otherwise: lists of 16 candidates and more then take the
two-stream head (scale 0's lists ahead: k_sparse_h2_one + k_sparse_h2_full, or k_sparse_h2_um, or k_sparse_h2; the other wide
scales behind the downscale: k_sparse_h2_from), a single candidate takes one launch for every scale.

The images, the palette and the lists' colours are those of tests/test_one_plane_h.py, restated: 256 x 32 (three scales: X alone
is one-plane at scale 0, and no scale is narrow) and 256 x 256 (six scales: X and B), one colour family per 64-column block, so
that a candidate wins in block 0 only, in block 3 only, or nowhere.
"""
import numpy as np
import pytest

SP, SI = 0, 14  # the slot the lists are scored on
FAMILY = np.array([[200, 40, 40], [40, 200, 40], [40, 40, 200], [200, 200, 40]], np.int64)  # RGB8 centre per 64-column block
NOTHING, BLOCK0, BLOCK3 = (0, 0, 0), (22, 7, 7), (23, 27, 7)  # raw 5-bit candidates
HEIGHTS = (32, 256)
FLAGS = [{}, {"perceptual": True}, {"dither": True}]  # dither: the map input of scale 0 (UM = true)
FLAG_IDS = ["rgb", "perceptual", "dither"]
BASE = {"SNES_H2Q_MAX": "0", "SNES_H0_MIN": "16"}
FULL = {"SNES_H_FORMS": "7"}
REFERENCE = "forms-0"
VARIANTS = {  # None: the variable is not set
    REFERENCE: {"SNES_H_FORMS": "0"},
    "forms-1": {"SNES_H_FORMS": "1"},
    "forms-2": {"SNES_H_FORMS": "2"},
    "forms-4": {"SNES_H_FORMS": "4"},
    "forms-7": FULL,
    "one-launch": dict(FULL, SNES_H0_MIN=None),      # every scale in one launch
    "grid-16": dict(FULL, SNES_H0_GRID="16"),        # each kernel strides over its own waves many times
    "dense": {"SNES_SPARSE": "0"},
    "poison": dict(FULL, SNES_DEBUG_POISON="1"),
    "three-planes": dict(FULL, SNES_H_PLANES="0"),   # the full form everywhere
    "full-sums": dict(FULL, SNES_WEIGHT_MASK="0"),   # the full form everywhere
}


def image(h, seed=0):
    rng = np.random.default_rng(0x2E60 + h + 1000 * seed)
    out = np.zeros((h, 256, 4), np.uint8)
    base = FAMILY[np.arange(256) // 64][None, :, :]
    out[..., :3] = np.clip(base + rng.integers(-24, 25, (h, 256, 3)), 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def palette():
    """Subpalette 0: three or four entries per family, the centre and neighbours on one side of it (a candidate on the other
    side then wins pixels); slot 14 is a colour of family 3."""
    pal = np.random.default_rng(77).integers(0, 32, (8 * 15, 3)).astype(np.uint8)
    c5 = FAMILY // 8
    rows = []
    for f in range(4):
        for d in ((0, 0, 0), (2, 0, 0), (0, 2, 0), (2, 2, 0)):
            rows.append(c5[f] + np.array(d))
    pal[:15] = np.array(rows[:15], np.uint8)
    return pal


def the_list(n, seed):
    """n candidates around the four families, with one that wins nothing, one that wins in block 0, one that wins only in block
    3, the incumbent and a repeated colour at fixed places."""
    rng = np.random.default_rng(seed)
    cand = np.clip((FAMILY // 8)[rng.integers(0, 4, n)] + rng.integers(-5, 6, (n, 3)), 0, 31).astype(np.uint8)
    cand[1], cand[2], cand[n // 2], cand[n - 2] = NOTHING, BLOCK0, BLOCK3, palette()[SP * 15 + SI]
    cand[3] = cand[n - 1] = (24, 26, 4)
    return cand


def lists():
    """Scored one after the other on one context: 1 candidate; 64; 67 (items and pairs leave ragged last waves, and a third of
    the items is no multiple of 16: both boundary waves mix classes); 64 that win nothing (every item count is 0: every kernel
    of the family returns); 64 again, over the storage the others left."""
    return [the_list(64, 5)[2:3], the_list(64, 5), the_list(67, 11), np.array([NOTHING] * 64, np.uint8), the_list(64, 9)]


@pytest.fixture(scope="module")
def S():
    import snesimage_amd
    return snesimage_amd


class env:
    """The switches are read when a context is created (the slot contexts of a window copy their parent's): set for as long as
    the variant's contexts live."""

    def __init__(self, monkeypatch, extra):
        self.mp, self.vars = monkeypatch, dict(BASE, **extra)

    def __enter__(self):
        for k, v in self.vars.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, v)

    def __exit__(self, *a):
        for k in self.vars:
            self.mp.delenv(k, raising=False)


def context(S, h, **flags):
    g = S.OptimizedImage(image(h), 8, 15, **flags)
    g.tile_palettes = np.zeros(1024, np.uint8)
    g.palette = palette()
    g.optimize()
    return g


def scored(S, h, monkeypatch, variant, flags):
    with env(monkeypatch, VARIANTS[variant]):
        g = context(S, h, **flags)
        out = [g.score_candidates(SP, SI, c) for c in lists()]
        g.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_every_mask_gives_the_bytes_of_the_bundled_kernels(S, h, flags, monkeypatch):
    ref = scored(S, h, monkeypatch, REFERENCE, flags)
    for e, c in zip(ref, lists()):
        assert e.dtype == np.float64 and e.shape == (len(c),) and np.all(np.isfinite(e))
    assert len(set(ref[1].tolist())) >= 4  # nothing won, block 0, block 3 and the incumbent are four different images at least
    assert len(set(ref[3].tolist())) == 1  # the list that wins nothing: B, 64 times
    for variant in VARIANTS:
        if variant == REFERENCE:
            continue
        got = scored(S, h, monkeypatch, variant, flags)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert b.dtype == np.float64 and np.all(np.isfinite(b)), (variant, i)
            assert a.tobytes() == b.tobytes(), (variant, i, int(np.sum(a != b)))


@pytest.mark.gpu
@pytest.mark.parametrize("h", HEIGHTS)
def test_slot_window_of_seven(S, h, monkeypatch):
    """Seven scheduled calls in one window (the batched shells: kb_sparse_h2_from behind the downscale under the full mask,
    kb_sparse_h2_lists under 0; the slot contexts take the switch from their parent) against the same calls one by one."""
    sched = S.schedule(8, 15, 7)
    runs = {}
    for variant in ("forms-7", REFERENCE):
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
    assert runs["forms-7"] == runs[REFERENCE]


@pytest.mark.gpu
def test_image_batch_of_two(S, monkeypatch):
    """Two images through one launch per stage, five scheduled calls."""
    from snesimage_amd.throughput import ImageBatch
    runs = {}
    for variant in ("forms-7", REFERENCE):
        with env(monkeypatch, VARIANTS[variant]):
            b = ImageBatch([(0, image(32)), (1, image(32, seed=1))], 8, 15, candidates=64, batched=True, groups=1)
            for m in b.images:
                m.tile_palettes = np.zeros(1024, np.uint8)
                m.palette = palette()
                m.optimize()
            b._open_batch()
            b.run(5)
            errs = np.asarray(b.errors(), np.float64)
            assert np.all(np.isfinite(errs)), variant
            runs[variant] = b"".join(m.palette.tobytes() + m.palette_map.tobytes() for m in b.images) + errs.tobytes()
            b.close()
    assert runs["forms-7"] == runs[REFERENCE]
