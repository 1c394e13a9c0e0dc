"""Inputs shared by the CPU and the GPU tests of the native import: a hand-made set of native bytes for a 256 x 16 picture with a
fully and a partly transparent tile, the mutations that make the import refuse them — with the tile and the reason the contract
names — and the foreign re-encoding of a state (shuffled, duplicated and unused cells, bases, priority bits, another flip for a
symmetric cell, garbage where CGRAM is not read).  Nothing here calls the library or the oracle."""
import numpy as np

import native_model as N
import native_import_model as I

S, C = 2, 2                   # the geometry of the refusal cases: 2bpp, two rows
CLEAR_TILE, HALF_TILE = 5, 6  # tile 5 is fully transparent, the left half of tile 6 is
LAYOUT = N.layout(2, char_base=4, palette_base=2)


def refusal_image():
    from snesimage_amd.synth import synth_image
    img = synth_image(0x5EED0F00, 256, 16)
    img[0:8, 40:48, 3] = 0
    img[0:8, 48:52, 3] = 0
    return img


def refusal_bytes():
    """-> (cgram, chr, words): cell 0 all 1, cell 1 all 0, cell 2 zero on its left half and 2 on its right, cell 3 all 3 (> S).
    Every tile draws cell 0 from row t % 2, tile 5 cell 1 and tile 6 cell 2: a state a plain (C, S) context accepts."""
    cells = np.zeros((4, 8, 8), np.uint8)
    cells[0] = 1
    cells[2][:, 4:] = 2
    cells[3] = 3
    chr_ = b"".join(N.encode_cell(c.reshape(64), 2).tobytes() for c in cells)
    words = np.array([N.map_word(0, LAYOUT["char_base"], t % 2, LAYOUT["palette_base"], 0, 0, 0, 2) for t in range(64)], np.uint16)
    words[CLEAR_TILE] = N.map_word(1, LAYOUT["char_base"], 1, LAYOUT["palette_base"], 0, 0, 0, 2)
    words[HALF_TILE] = N.map_word(2, LAYOUT["char_base"], 0, LAYOUT["palette_base"], 0, 0, 0, 2)
    cg = np.random.default_rng(7).integers(0, 65536, 256).astype("<u2")
    return cg.tobytes(), chr_, words


def with_cell(word, cell):
    return (int(word) & ~1023) | (LAYOUT["char_base"] + cell)


def with_field(word, field):
    return (int(word) & ~(7 << 10)) | (field << 10)


def refusal_cases():
    """[(name, words, chr, backdrop contexts too?, (tile, reason) on a plain context, the same on a backdrop context or None if
    it is accepted there)]"""
    cgram, chr_, base = refusal_bytes()
    out = []

    def case(name, edits, plain, backdrop="same", chr_bytes=chr_):
        w = base.copy()
        for t, v in edits.items():
            w[t] = v
        out.append((name, w, chr_bytes, plain, plain if backdrop == "same" else backdrop))

    case("below", {9: (int(base[9]) & ~1023) | 3}, (9, I.BELOW))
    case("past", {9: with_cell(base[9], 4)}, (9, I.PAST))
    case("palette_high", {9: with_field(base[9], 4)}, (9, I.PALETTE))
    case("palette_low", {9: with_field(base[9], 1)}, (9, I.PALETTE))
    case("value", {9: with_cell(base[9], 3)}, (9, I.VALUE))
    case("opaque_zero", {9: with_cell(base[9], 1)}, (9, I.OPAQUE_ZERO), None)
    case("clear_value", {CLEAR_TILE: with_cell(base[CLEAR_TILE], 0)}, (CLEAR_TILE, I.CLEAR_VALUE))
    case("lowest_tile", {20: with_field(base[20], 7), 9: with_cell(base[9], 3)}, (9, I.VALUE))                       # the tile orders, not the reason
    case("lowest_reason", {HALF_TILE: int(base[HALF_TILE]) | 0x4000}, (HALF_TILE, I.OPAQUE_ZERO), (HALF_TILE, I.CLEAR_VALUE))  # hflip: both halves are wrong
    case("number_before_field", {9: with_field(with_cell(base[9], 4), 7), 30: (int(base[30]) & ~1023) | 0}, (9, I.PAST))
    case("ragged", {}, (None, I.CHR), chr_bytes=chr_[:-1])
    return cgram, out


def foreign(chars, rep, flip, tile_palettes, palette_u16, backdrop, bpp, seed=0):
    """A state re-encoded as a foreign tool might: CHR shuffled with one cell duplicated (both copies in use when the class has
    two tiles) and one cell nobody uses, char_base 256 and palette_base 2, the priority bit set in every third word, a symmetric
    cell drawn with another flip, garbage in every CGRAM word the geometry does not name and — with a backdrop — in the rows'
    first words.  -> (cgram, chr, words, layout)"""
    rng = np.random.default_rng(seed)
    chars, rep, flip = np.asarray(chars, np.uint8), np.asarray(rep, np.int64), np.asarray(flip, np.int64)
    Cn, Sn = np.shape(palette_u16)
    lay = N.layout(bpp, char_base=256, palette_base=0 if bpp == 8 else 2)
    reps = [t for t in range(len(chars)) if rep[t] == t]
    cells = [chars[t] for t in reps] + [chars[reps[0]], rng.integers(0, Sn + 1, 64).astype(np.uint8)]  # + a duplicate of class 0, + an unused cell
    order = rng.permutation(len(cells))
    at = {int(c): i for i, c in enumerate(order)}  # cell c sits at position at[c]
    chr_ = b"".join(N.encode_cell(cells[c], bpp).tobytes() for c in order)
    words = np.zeros(len(chars), np.uint16)
    seen_first = False
    for t in range(len(chars)):
        cls = reps.index(int(rep[t]))
        cell, f = cls, int(flip[t])
        if cls == 0 and seen_first:
            cell = len(reps)  # later tiles of class 0 draw the duplicate
        seen_first = seen_first or cls == 0
        c8 = cells[cell].reshape(8, 8)
        if np.array_equal(c8, c8[:, ::-1]):
            f ^= 1  # a cell equal to its mirror image: the other flip draws the same
        if np.array_equal(c8, c8[::-1, :]):
            f ^= 2
        words[t] = N.map_word(at[cell], lay["char_base"], int(tile_palettes[t]), lay["palette_base"], 1 if t % 3 == 0 else 0, f & 1, f >> 1, bpp)
    cg = rng.integers(0, 65536, 256).astype(np.uint16)  # garbage everywhere, bit 15 included ...
    pal = np.asarray(palette_u16, np.uint16)
    for p in range(Cn):  # ... but in the words that are read
        start = 0 if bpp == 8 else (lay["palette_base"] + p) << bpp
        cg[start + 1:start + 1 + Sn] = pal[p] | (rng.integers(0, 2, Sn).astype(np.uint16) << 15)
    if backdrop is not None:
        cg[0] = int(backdrop[0]) | int(backdrop[1]) << 5 | int(backdrop[2]) << 10
    return cg.astype("<u2").tobytes(), chr_, words, lay
