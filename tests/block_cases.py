"""The case table of the palette-block tests: the smallest shapes at which the block kernels can still go wrong, and the
builders both test files share.  Every row must leave at least one block mixed under the per-tile oracle (checked on the CPU by
test_blocks_model.py): otherwise the constraint binds on nothing and the row proves nothing."""
import numpy as np

import block_model as BM

#        id                  h   count size bw bh  flags                               image
CASES = [
    ("16_2x2",              16,  4,    3,   2, 2, {},                                  "synth"),   # one block row
    ("16_2x1",              16,  4,    3,   2, 1, {},                                  "synth"),   # 128 pixels: half of the remap's 256 threads, rows of 16
    ("32_2x2_alpha",        32,  4,    7,   2, 2, {},                                  "alpha"),
    ("32_4x2_perceptual",   32,  2,    3,   4, 2, {"perceptual": True},                "synth"),   # with the next: bw / bh exchanged
    ("32_2x4",              32,  4,    3,   2, 4, {},                                  "synth"),
    ("48_2x2",              48,  4,    3,   2, 2, {},                                  "synth"),   # three block rows, an odd count
    ("64_8x8",              64,  2,    3,   8, 8, {},                                  "synth"),   # four blocks: the 4,096-pixel candidate
    ("32_2x2_dither",       32,  4,    3,   2, 2, {"dither": True},                    "synth"),
    ("32_2x2_dither_perc",  32,  4,    3,   2, 2, {"dither": True, "perceptual": True}, "synth"),
    ("32_2x2_nes",          32,  4,    3,   2, 2, {"nes": True},                       "synth"),
    ("32_2x2_backdrop",     32,  4,    3,   2, 2, {"backdrop": True},                  "synth"),
    ("32_2x2_holes",        32,  4,    3,   2, 2, {},                                  "holes"),
    ("224_2x4",             224, 4,    3,   2, 4, {},                                  "synth"),   # seven block rows; a handful of pairs only
]
CASE_IDS = [c[0] for c in CASES]
HOLE_BLOCKS = {"transparent": 1, "black": 2, "one_tile": 3}  # the blocks the "holes" image changes


def case(name):
    return next(c for c in CASES if c[0] == name)


def image(kind, h, bw=2, bh=2):
    from snesimage_amd.synth import synth_image
    if kind == "alpha":
        return np.ascontiguousarray(synth_image(0x5EED0001, variant=1)[:h])
    img = np.ascontiguousarray(synth_image()[:h]).copy()
    if kind == "holes":  # one whole block at alpha 0, one whole block black, one block with a single opaque tile
        def area(b):
            nbx = 32 // bw
            return slice((b // nbx) * bh * 8, (b // nbx + 1) * bh * 8), slice((b % nbx) * bw * 8, (b % nbx + 1) * bw * 8)
        ys, xs = area(HOLE_BLOCKS["transparent"])
        img[ys, xs, 3] = 0
        ys, xs = area(HOLE_BLOCKS["black"])
        img[ys, xs, :3] = 0
        ys, xs = area(HOLE_BLOCKS["one_tile"])
        keep = img[ys.start:ys.start + 8, xs.start:xs.start + 8, 3].copy()
        img[ys, xs, 3] = 0
        img[ys.start:ys.start + 8, xs.start:xs.start + 8, 3] = keep
    return img


def oracle_flags(flags):
    return {k: v for k, v in flags.items() if k != "backdrop"}


def mean_backdrop(O, img, flags):
    from backdrop_model import mean_backdrop as mb
    return mb(img, O, bool(flags.get("nes")), bool(flags.get("perceptual")))


def expand(pal, B, count, size):
    """The palette of the oracle's expanded context (count, size + 1): column `size` holds the backdrop colour B."""
    out = np.zeros((count, size + 1, 3), np.uint8)
    out[:, :size] = np.asarray(pal, np.uint8).reshape(count, size, 3)
    out[:, size] = B
    return out.reshape(-1, 3)


def model_start(O, img, count, size, bw, bh, flags, recalc=True):
    """The oracle in the state the blocked initialiser (and recalculate_palettes) leaves: the blocked model at bw x bh, the
    oracle's own initialiser at 1 x 1.  A backdrop case returns the oracle on the expanded geometry (backdrop_model.py)."""
    of = oracle_flags(flags)
    o = O.OracleImage(img, count, size, **of)
    if bw * bh == 1:
        o.initialize_tiles()
    else:
        BM.model_initialize_tiles(O, o, img, bw, bh, bool(of.get("perceptual")), bool(of.get("nes")))
    if recalc:
        o.recalculate_palettes()
    if not flags.get("backdrop"):
        return o
    x = O.OracleImage(img, count, size + 1, **of)
    x.tile_palettes = o.tile_palettes
    x.palette = expand(o.palette, mean_backdrop(O, img, flags), count, size)
    x.optimize()
    o.close()
    return x


def regular(o, count, size, flags):
    """The regular entries of the model's palette (all of them unless the case is a backdrop case)."""
    if not flags.get("backdrop"):
        return o.palette
    return o.palette.reshape(count, size + 1, 3)[:, :size].reshape(-1, 3).copy()
