"""A second family of 256 x h RGBA8 test images, beside the gradient-plus-noise family of snesimage_amd/synth.py: the
content real inputs are made of (pixel art, sprites with cut-out alpha, flat areas) and the branches it reaches —
duplicate leading k-means points (NaN centres), subpalettes left without tiles, the tile-mean filter, alpha other than
0 / 255 and transparent borders, massive ties, neutral / blue-violet / near-black Lab colours, the dither clamp.
Pure numpy and deterministic; tests/test_adversarial_content.py pins every image's sha256."""
import numpy as np

W = 256

# flat colours of pixel_art: black, white, dark blue (L + a + b < 0), primaries, greys 1 apart, near black, near white
K = [(0, 0, 0), (255, 255, 255), (0, 0, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (128, 128, 128), (127, 127, 127), (8, 8, 8),
     (248, 248, 248), (0, 0, 40), (255, 255, 0)]


def _grid(h):
    if h % 8 or h <= 0:
        raise ValueError("h must be a positive multiple of 8")
    y, x = np.mgrid[0:h, 0:W]
    return y, x


def _opaque(h, r, g, b):
    out = np.zeros((h, W, 4), np.uint8)
    for c, v in enumerate((r, g, b)):
        v = np.asarray(v)
        assert v.min() >= 0 and v.max() <= 255
        out[..., c] = v
    out[..., 3] = 255
    return out


def pixel_art(h=32):
    """Opaque; tile (tx, ty): left 4 columns K[(5 tx + 7 ty) % 12], right 4 columns K[(3 tx + ty + 1) % 12]."""
    y, x = _grid(h)
    tx, ty = x // 8, y // 8
    k = np.where(x % 8 < 4, (5 * tx + 7 * ty) % 12, (3 * tx + ty + 1) % 12)
    rgb = np.array(K, np.uint8)[k]
    return _opaque(h, rgb[..., 0], rgb[..., 1], rgb[..., 2])


def alpha_mix(h=32):
    """The gradient image with alpha from {0, 1, 127, 128, 254, 255}, a transparent border, two tiles with a single
    opaque pixel (the tile's first, alpha 200; the tile's last, alpha 1) and a run of fully transparent tiles."""
    from snesimage_amd.synth import synth_image
    y, x = _grid(h)
    out = synth_image(0x5EED0040, W, h, 0)
    out[..., 3] = np.array([0, 1, 127, 128, 254, 255, 255, 255], np.uint8)[(7 * x + 13 * y + (x * y) % 5) % 8]
    out[0, :, 3] = out[h - 1, :, 3] = 0
    out[:, 0, 3] = out[:, W - 1, 3] = 0
    out[8:16, 8:16, 3] = 0      # tile (1, 1)
    out[8, 8, 3] = 200
    out[8:16, 16:24, 3] = 0     # tile (2, 1)
    out[15, 23, 3] = 1
    out[16:24, 64:128, 3] = 0
    return out


def two_tone(h=32):
    """Opaque; a 1-pixel black / white checkerboard, flat 128 in columns 128..191, white every third column in 192..255."""
    y, x = _grid(h)
    v = ((x + y) & 1) * 255
    v = np.where((x >= 128) & (x < 192), 128, v)
    v = np.where(x >= 192, (x % 3 == 0) * 255, v)
    return _opaque(h, v, v, v)


def lab_extremes(h=32):
    """Opaque; four bands of h / 4 rows: neutral ramp, blue-violet (x, x // 2, 255), near black, (255 - x, 37 y, x)."""
    y, x = _grid(h)
    band = y // (h // 4)
    chans = []
    for c, (violet, last) in enumerate(((x, 255 - x), (x // 2, (37 * y) % 256), (np.full_like(x, 255), x))):
        chans.append(np.select([band == 0, band == 1, band == 2], [x, violet, (x + 3 * c) % 8], last))
    return _opaque(h, *chans)


def flat_tiles(h=32):
    """pixel_art with whole tiles of one dark colour.  pixel_art itself never has a one-colour tile: equal left and right
    indices, 5 tx + 7 ty = 3 tx + ty + 1 (mod 12), mean 2 tx + 6 ty - 1 = 0 (mod 12), and the left side is odd.  The
    tile-mean filter `sum > 0` drops exactly one-colour black (and, with Lab sums, dark-blue) tiles.  Row 0 of tiles:
    tile 3 black, tile 5 (0, 0, 128), tile 7 (0, 0, 40); and the last tile black."""
    out = pixel_art(h)
    for tx, ty, rgb in ((3, 0, (0, 0, 0)), (5, 0, (0, 0, 128)), (7, 0, (0, 0, 40)), (31, h // 8 - 1, (0, 0, 0))):
        out[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8, :3] = rgb
    return out


IMAGES = {"pixel_art": pixel_art, "alpha_mix": alpha_mix, "two_tone": two_tone, "lab_extremes": lab_extremes}


def hand_tiles(count):
    """1,024 tile palettes ((tx // 2 + ty) % count) laid out as ty * 32 + tx: a start where the k-means initialisers refuse."""
    t = np.arange(1024)
    return (((t % 32) // 2 + t // 32) % count).astype(np.uint8)
