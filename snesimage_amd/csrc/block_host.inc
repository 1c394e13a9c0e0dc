// snesimage_amd/csrc/block_host.inc — palette blocks: snesimage_set_palette_blocks / _get_palette_blocks, the blocked k-means
// initialiser and proxy reassignment, and the block moves decided by the objective: snesimage_score_block_moves,
// snesimage_block_step, snesimage_block_sweep (definition: include/snesimage_hip.h; kernels: kernels_tile.hpp).
//
// A tile move is the move of a 1 x 1 block, so both run through one host code (tile_host.inc: move_score_list, tile_sweep_impl)
// and one kernel family (k_move_*, k_unit_*): the block entry points hand in the context's BlockGeom, the tile entry points
// tile_geom.  The blocked initialiser is kmeans_initialize_tiles (kmeans_host.inc) and the blocked reassignment
// snesimage_reassign_tiles (capi.hip), on the context's geometry too.  Included by capi.hip behind tile_host.inc.

extern "C" {

int32_t snesimage_set_palette_blocks(snesimage_ctx *c, uint32_t bw, uint32_t bh) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    auto ok = [](uint32_t v) { return v == 1 || v == 2 || v == 4 || v == 8; };
    if (!ok(bw) || !ok(bh)) return fail(SNES_ERR_ARG, "palette blocks are 1, 2, 4 or 8 tiles wide and high");
    if ((c->H / 8) % bh) return fail(SNES_ERR_ARG, "the block height " + std::to_string(bh) + " does not divide the image's " + std::to_string(c->H / 8) + " rows of tiles");
    if (c->pend || c->win_pend) return fail(SNES_ERR_STATE, "a split-phase step is pending: commit it first");
    if (c->owner || c->group) return fail(SNES_ERR_STATE, "the context is lent to a batch, a set or a group, whose members choose a subpalette per tile: destroy that first");
    if (bw * bh > 1) {
        CHECK(set_device(c));
        std::vector<uint8_t> tp(1024);
        HIPCHK(hipMemcpyAsync(tp.data(), c->d_tile_pal, 1024, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const int b = untied_block(tp.data(), c->H, bw, bh);
        if (b >= 0) return fail(SNES_ERR_STATE, "tile_palettes is not constant over block " + std::to_string(b) + " of " + std::to_string(bw) + " x " + std::to_string(bh) +
                                                " palette blocks: set a table that is (snesimage_set_tile_palettes), or call snesimage_set_palette_blocks before snesimage_initialize_tiles");
    }
    c->pb_w = bw; c->pb_h = bh;
    return SNES_OK;
}

int32_t snesimage_get_palette_blocks(snesimage_ctx *c, uint32_t *bw, uint32_t *bh) {
    if (!c || !bw || !bh) return fail(SNES_ERR_ARG, "null pointer");
    *bw = c->pb_w; *bh = c->pb_h;
    return SNES_OK;
}

int32_t snesimage_score_block_moves(snesimage_ctx *c, const uint16_t *blocks, const uint8_t *subs, uint32_t n, double *errors, uint8_t *maps_out) {
    CHECK(tile_check(c));
    return move_score_list(c, blocks, subs, n, errors, maps_out, block_geom(c), "block");
}

int32_t snesimage_block_step(snesimage_ctx *c, uint32_t block, snesimage_tile_result *out) {
    snesimage_tile_result r{};
    if (!c) return fail(SNES_ERR_ARG, "null context");
    CHECK(tile_sweep_impl(c, block, 1, 1, &r, nullptr, block_geom(c), "block"));
    if (out) *out = r;
    return SNES_OK;
}

int32_t snesimage_block_sweep(snesimage_ctx *c, uint32_t first_block, uint32_t n_blocks, uint32_t window, snesimage_tile_result *log, snesimage_run_stats *stats) {
    if (!c) return fail(SNES_ERR_ARG, "null context");
    return tile_sweep_impl(c, first_block, n_blocks, window, log, stats, block_geom(c), "block");
}

} // extern "C"
