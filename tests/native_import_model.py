"""The model of the native import (include/snesimage_hip.h: "Native import") in numpy, written from the contract: `parse`
reads CGRAM, CHR and MAP bytes into a state — palette, backdrop colour, tile palettes, map — or names the lowest offending tile
and its reason.  It calls neither the library nor the oracle and borrows only native_model's helpers."""
import numpy as np

from native_model import auto_bpp

# the reasons, in the order in which one tile's reasons are reported
CHR, BELOW, PAST, PALETTE, VALUE, OPAQUE_ZERO, CLEAR_VALUE = 0, 1, 2, 3, 4, 5, 6
# what the library's message says for each
REASON_TEXT = {CHR: "chr_bytes", BELOW: "below char_base", PAST: "past the", PALETTE: "selects palette", VALUE: "value above", OPAQUE_ZERO: "SNES_BACKDROP",
               CLEAR_VALUE: "transparent"}


def cell_values(chr_, bpp):
    """chr bytes -> (cells, 8, 8) character values [cell, y, x]: plane pair k, row y: byte 16k + 2y is plane 2k, byte 16k + 2y + 1
    plane 2k + 1; bit 7 - x of a plane byte is that plane's bit at column x."""
    cells = np.frombuffer(bytes(chr_), np.uint8).reshape(-1, 8 * bpp).astype(np.int64)
    out = np.zeros((len(cells), 8, 8), np.int64)
    for k in range(bpp // 2):
        for y in range(8):
            for x in range(8):
                out[:, y, x] |= ((cells[:, 16 * k + 2 * y] >> (7 - x)) & 1) << (2 * k)
                out[:, y, x] |= ((cells[:, 16 * k + 2 * y + 1] >> (7 - x)) & 1) << (2 * k + 1)
    return out


def parse(cgram, chr_, words, lay, S, C, backdrop, alpha):
    """-> (palette_rgb5 uint8[C * S, 3], B (three 5-bit values, or None without a backdrop), tile_palettes uint8[n], map) or
    (tile, reason).  words: one per tile of one image, or of every member of a set one after another; alpha: the source alpha,
    [h, 256] or [F, h, 256]; map has alpha's shape.  lay: native_model.layout (bpp 0 = the smallest depth that holds S; the
    priority is not read).  The layout is taken as valid: its refusals are the export's."""
    bpp = lay["bpp"] or auto_bpp(S)
    cb, pb = lay["char_base"], lay["palette_base"]
    chr_ = bytes(chr_)
    if len(chr_) == 0 or len(chr_) % (8 * bpp) or len(chr_) // (8 * bpp) > 1024:
        return None, CHR
    cells = cell_values(chr_, bpp)
    words = np.asarray(words, np.int64).reshape(-1)
    alpha = np.asarray(alpha)
    single = alpha.ndim == 2
    al = alpha[None] if single else alpha
    F, h = al.shape[0], al.shape[1]
    ntile = 32 * (h // 8)
    assert len(words) == F * ntile
    tps = np.zeros(len(words), np.uint8)
    maps = np.zeros(al.shape, np.uint8)
    for g, w in enumerate(words.tolist()):
        m, t = divmod(g, ntile)
        n = (w & 1023) - cb
        reasons = []
        if n < 0:
            reasons.append(BELOW)
        elif n >= len(cells):
            reasons.append(PAST)
        p = 0
        if bpp != 8:
            p = ((w >> 10) & 7) - pb
            if not 0 <= p < C:
                reasons.append(PALETTE)
        if reasons:  # (a tile whose number is refused is not decoded further; the palette field is judged before the pixels)
            return g, min(reasons)
        v = cells[n]
        if w & 0x4000:
            v = v[:, ::-1]
        if w & 0x8000:
            v = v[::-1, :]
        y0, x0 = (t // 32) * 8, (t % 32) * 8
        clear = al[m, y0:y0 + 8, x0:x0 + 8] == 0
        if (v > S).any():
            return g, VALUE
        if not backdrop and ((v == 0) & ~clear).any():
            return g, OPAQUE_ZERO
        if ((v != 0) & clear).any():
            return g, CLEAR_VALUE
        tps[g] = p
        maps[m, y0:y0 + 8, x0:x0 + 8] = np.where(v >= 1, v - 1, np.where(clear, 0, S))
    cg = np.frombuffer(bytes(cgram), "<u2").astype(np.int64) & 0x7FFF
    pal = np.zeros((C, S, 3), np.uint8)
    for p in range(C):
        start = 0 if bpp == 8 else (pb + p) << bpp
        ws = cg[start + 1:start + 1 + S]
        pal[p] = np.stack([ws & 31, (ws >> 5) & 31, (ws >> 10) & 31], axis=-1)
    B = np.array([cg[0] & 31, (cg[0] >> 5) & 31, (cg[0] >> 10) & 31], np.uint8) if backdrop else None
    return pal.reshape(C * S, 3), B, tps, (maps[0] if single else maps)
