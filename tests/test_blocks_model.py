"""The premises of the palette-block tests, on the CPU: the model (tests/block_model.py) equals the oracle where a block is a
tile, every row of the case table binds the constraint on something, the model's own results are tied, blocks without colour keep
their entry, and a model with bw and bh exchanged is seen."""
import numpy as np
import pytest

import block_cases as BC
import block_model as BM


@pytest.mark.parametrize("flags", [{}, {"perceptual": True}, {"nes": True}], ids=["plain", "perceptual", "nes"])
def test_model_at_1x1_is_the_oracle(O, flags):
    """Initialiser and reassignment of the model at 1 x 1 against oracle.initialize_tiles() / reassign_tiles(): table, palette and
    map bit for bit, the number of tiles moved equal."""
    img = BC.image("alpha", 32)
    count, size = 4, 3
    a, b = O.OracleImage(img, count, size, **flags), O.OracleImage(img, count, size, **flags)
    a.initialize_tiles()
    BM.model_initialize_tiles(O, b, img, 1, 1, bool(flags.get("perceptual")), bool(flags.get("nes")))
    for step in range(2):
        assert np.array_equal(a.tile_palettes, b.tile_palettes) and np.array_equal(a.palette, b.palette) and np.array_equal(a.palette_map, b.palette_map)
        if step == 0:
            a.recalculate_palettes()
            b.recalculate_palettes()
            moved = a.reassign_tiles()
            assert moved > 0 and BM.model_reassign(O, b, img, 1, 1, bool(flags.get("perceptual"))) == moved
    a.close()
    b.close()


@pytest.mark.parametrize("name,h,count,size,bw,bh,flags,kind", BC.CASES, ids=BC.CASE_IDS)
def test_every_case_binds_the_constraint_and_the_model_is_tied(O, name, h, count, size, bw, bh, flags, kind):
    """The per-tile oracle leaves at least one block mixed after the initialiser and after the reassignment (else the row
    proves nothing); the model's own results are tied, and its reassignment moves whole blocks."""
    img = BC.image(kind, h, bw, bh)
    perc = bool(flags.get("perceptual"))
    o = BC.model_start(O, img, count, size, 1, 1, flags)
    assert len(BM.mixed_blocks(o.tile_palettes, h, bw, bh)) >= 1, "per-tile initialiser: no mixed block"
    o.reassign_tiles()
    assert len(BM.mixed_blocks(o.tile_palettes, h, bw, bh)) >= 1, "per-tile reassignment: no mixed block"
    o.close()
    m = BC.model_start(O, img, count, size, bw, bh, flags)
    assert BM.is_tied(m.tile_palettes, h, bw, bh)
    assert len(set(m.tile_palettes[:32 * (h // 8)].tolist())) > 1
    moved = BM.model_reassign(O, m, img, bw, bh, perc)
    assert moved % (bw * bh) == 0 and BM.is_tied(m.tile_palettes, h, bw, bh)
    m.close()


def test_blocks_without_colour_keep_their_entry(O):
    """The transparent and the black block are left out of the k-means points and keep what they had (here 3); the block with
    one opaque tile is clustered as a whole.  The reassignment passes the transparent block by."""
    _, h, count, size, bw, bh, flags, kind = BC.case("32_2x2_holes")
    img = BC.image(kind, h, bw, bh)
    o = O.OracleImage(img, count, size)
    tp = np.zeros(1024, np.uint8)
    tp[:32 * (h // 8)] = 3
    o.tile_palettes = tp
    BM.model_initialize_tiles(O, o, img, bw, bh)
    after = o.tile_palettes
    for key in ("transparent", "black"):
        assert (after[BM.block_tiles(BC.HOLE_BLOCKS[key], bw, bh)] == 3).all(), key
    one = after[BM.block_tiles(BC.HOLE_BLOCKS["one_tile"], bw, bh)]
    assert len(set(one.tolist())) == 1 and BM.is_tied(after, h, bw, bh)
    o.recalculate_palettes()
    BM.model_reassign(O, o, img, bw, bh)
    assert (o.tile_palettes[BM.block_tiles(BC.HOLE_BLOCKS["transparent"], bw, bh)] == 3).all()
    o.close()


def test_hand_written_2x2_case(O):
    """A 256 x 16 strip of sixteen 16 x 16 squares, red and blue in turn, and one 8 x 8 tile of blue square 5 painted red.
    k-means over the 2 x 2 blocks with k = 2 starts from blocks 0 (red) and 1 (blue): every red square lands in cluster 0,
    every blue one in cluster 1, and square 5 — three quarters blue — goes to cluster 1 as a whole, its red tile included."""
    img = np.zeros((16, 256, 4), np.uint8)
    img[..., 3] = 255
    red, blue = (200, 16, 16), (16, 16, 200)
    for b in range(16):
        img[:, b * 16:(b + 1) * 16, :3] = red if b % 2 == 0 else blue
    img[:8, 5 * 16:5 * 16 + 8, :3] = red
    o = O.OracleImage(img, 2, 3)
    BM.model_initialize_tiles(O, o, img, 2, 2)
    want = np.array([[0, 0, 1, 1] * 8, [0, 0, 1, 1] * 8], np.uint8)  # rows of tiles 0 and 1, written out
    assert np.array_equal(o.tile_palettes[:64].reshape(2, 32), want), o.tile_palettes[:64].reshape(2, 32)
    assert BM.block_tiles(5, 2, 2) == [10, 11, 42, 43] and BM.n_blocks(16, 2, 2) == 16
    pal = o.palette.reshape(2, 3, 3)
    assert (pal[0] == (25, 2, 2)).all() and pal[1, 0, 2] > pal[1, 0, 0]  # red / 8 exactly; the other one is bluish
    o.close()


def test_a_model_with_bw_and_bh_exchanged_is_seen(O):
    _, h, count, size, bw, bh, flags, kind = BC.case("32_4x2_perceptual")
    img = BC.image(kind, h, bw, bh)
    a = BC.model_start(O, img, count, size, bw, bh, flags)
    b = BC.model_start(O, img, count, size, bh, bw, flags)
    assert not np.array_equal(a.tile_palettes, b.tile_palettes)
    assert BM.is_tied(a.tile_palettes, h, bw, bh) and not BM.is_tied(b.tile_palettes, h, bw, bh)
    assert BM.block_tiles(1, 4, 2) != BM.block_tiles(1, 2, 4)
    a.close()
    b.close()
