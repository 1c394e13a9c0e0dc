// snesimage_amd/csrc/kmeans_host.inc — host sequencing of the k-means initialisers
// (initialize_tiles lib.rs:79-189, recalculate_palette(s) lib.rs:330-415).  Included by capi.hip
// after `struct snesimage_ctx`.  The arithmetic (tile sums, Lab, distances, centre sums, the
// convergence test) runs in the kernels of kernels_opt.hpp; the host only builds the point
// order the reference defines, checks cogset's precondition and converts centres to colours.

namespace {

// palette 0.7.6: Lab<D65,f64> -> Xyz -> LinSrgb -> Srgb<f64> (clamped) -> Srgb<u8> (lib.rs:141-142, 369-371)
void host_lab_to_srgb8(const double *lab, uint8_t *rgb) {
    const double y = (lab[0] + PALETTE_LAB_L_OFFSET_D) / PALETTE_LAB_L_SCALE_D, x = y + (lab[1] / PALETTE_LAB_A_SCALE_D), z = y - (lab[2] / PALETTE_LAB_B_SCALE_D); // include/ssimulacra2_constants.h
    const double epsilon = PALETTE_LAB_EPS_ROOT_D, kappa = PALETTE_LAB_KAPPA_INV_D, delta = PALETTE_LAB_DELTA_D;
    auto conv = [&](double c) { return c > epsilon ? c * c * c : (c - delta) * kappa; };
    const double X = conv(x) * PALETTE_D65_X_D, Y = conv(y) * PALETTE_D65_Y_D, Z = conv(z) * PALETTE_D65_Z_D;
    const double lin[3] = {(X * PALETTE_RGB_RX) + (Y * PALETTE_RGB_RY) + (Z * PALETTE_RGB_RZ), (X * PALETTE_RGB_GX) + (Y * PALETTE_RGB_GY) + (Z * PALETTE_RGB_GZ),
                           (X * PALETTE_RGB_BX) + (Y * PALETTE_RGB_BY) + (Z * PALETTE_RGB_BZ)};
    for (int i = 0; i < 3; i++) {
        double v = lin[i];
        double e = v <= PALETTE_SRGB_ENCODE_THRESHOLD_D ? PALETTE_SRGB_LINEAR_DIV_D * v : PALETTE_SRGB_SCALE_D * std::pow(v, 1.0 / PALETTE_SRGB_GAMMA_D) - PALETTE_SRGB_OFFSET_D;
        if (!(e >= 0.0)) e = 0.0;
        if (e > 1.0) e = 1.0;
        rgb[i] = (uint8_t)std::nearbyint(e * 255.0);
    }
}
// Rust `f64 as u8`: saturating, NaN -> 0
uint8_t host_f64_as_u8(double v) { if (!(v == v) || v <= 0.0) return 0; if (v >= 255.0) return 255; return (uint8_t)v; }

// SnesColor::new_nes_only, lib.rs:640-660
void host_new_nes_only(const uint8_t *raw, bool cielab, const float *lab_eotf, uint8_t *out) {
    const uint32_t color = rgb5_to_rgb8(raw[0], raw[1], raw[2]);
    uint8_t best[3] = {kNesTableHost[0][0], kNesTableHost[0][1], kNesTableHost[0][2]};
    double best_error = 1.7976931348623157e308;
    for (uint32_t i = 0; i < kNesColorCount; i++) {
        const uint32_t nc = rgb5_to_rgb8(kNesTableHost[i][0], kNesTableHost[i][1], kNesTableHost[i][2]);
        double error;
        if (cielab) {
            Lab a = linear_to_lab(lab_eotf[color & 0xff], lab_eotf[(color >> 8) & 0xff], lab_eotf[(color >> 16) & 0xff]);
            Lab b = linear_to_lab(lab_eotf[nc & 0xff], lab_eotf[(nc >> 8) & 0xff], lab_eotf[(nc >> 16) & 0xff]);
            error = (double)ciede2000(a, b);
        } else error = std::sqrt((double)red_mean_key(color, nc) / 512.0); // monotone in the reference's distance; only the order matters
        if (error < best_error) { best[0] = kNesTableHost[i][0]; best[1] = kNesTableHost[i][1]; best[2] = kNesTableHost[i][2]; best_error = error; }
    }
    out[0] = best[0]; out[1] = best[1]; out[2] = best[2];
}

// centre -> SnesColor (lib.rs:140-171 == 369-401)
void host_centre_to_color(const snesimage_ctx *c, const double *centre, uint8_t *out) {
    uint8_t raw[3];
    if (c->perceptual) {
        uint8_t rgb[3];
        host_lab_to_srgb8(centre, rgb);
        raw[0] = rgb[0] / 8; raw[1] = rgb[1] / 8; raw[2] = rgb[2] / 8;
    } else {
        for (int i = 0; i < 3; i++) raw[i] = host_f64_as_u8(std::round(centre[i] / 8.0));
    }
    if (c->nes) host_new_nes_only(raw, c->perceptual, c->h_lab_eotf, out);
    else { out[0] = raw[0]; out[1] = raw[1]; out[2] = raw[2]; }
}

int32_t kmeans_reserve(snesimage_ctx *c, size_t npts, int nprob, int k) {
    KmeansWork &w = c->km;
    if (w.cap_pts >= npts && w.cap_prob >= nprob && w.cap_k >= k) return SNES_OK;
    // grow-only, sized for the image once: every problem set of this context fits (points <= pixels, problems <= subpalettes)
    if (npts < c->npx) npts = c->npx;
    if (nprob < (int)c->sub_count) nprob = (int)c->sub_count;
    if (k < (int)c->sub_size) k = (int)c->sub_size;
    if (k < (int)c->sub_count) k = (int)c->sub_count;
    kmeans_free(w);
    HIPCHK(hipMalloc(&w.pts, sizeof(double) * 3 * npts));
    HIPCHK(hipMalloc(&w.assign, sizeof(uint32_t) * npts));
    HIPCHK(hipMalloc(&w.centres, sizeof(double) * 3 * (size_t)nprob * k));
    HIPCHK(hipMalloc(&w.rounds, sizeof(int) * nprob));
    HIPCHK(hipMalloc(&w.d_n, sizeof(int) * nprob));
    HIPCHK(hipMalloc(&w.d_off, sizeof(long long) * nprob));
    HIPCHK(hipMalloc(&w.d_sums, sizeof(float) * 3 * 1024));
    HIPCHK(hipMalloc(&w.d_counts, sizeof(int) * 1024));
    HIPCHK(hipMalloc(&w.d_index, sizeof(uint32_t) * npts));
    w.cap_pts = npts; w.cap_prob = nprob; w.cap_k = k; w.cap_meta = nprob; w.cap_tile = 1024; w.cap_index = npts;
    return SNES_OK;
}

// Points already in c->km.pts (problem p occupies [off[p], off[p]+n[p])).  cogset: centres start as
// the first k points; at most 100 (update_centres, update_assignments) rounds.  One launch, one block per problem.
int32_t kmeans_run(snesimage_ctx *c, const std::vector<int> &n, const std::vector<long long> &off, int k, std::vector<double> &centres, std::vector<uint32_t> *assign0) {
    const int nprob = (int)n.size();
    for (int p = 0; p < nprob; p++)
        if (!(2 <= k && k < n[p])) return fail(SNES_ERR_KMEANS, "k-means precondition 2 <= k < n violated (the reference panics here)");
    if (k > 253) return fail(SNES_ERR_ARG, "k-means: at most 253 centres");
    KmeansWork &w = c->km;
    if (w.cap_meta < nprob) return fail(SNES_ERR_STATE, "k-means: workspace not reserved");
    int *d_n = w.d_n; long long *d_off = w.d_off;
    auto cleanup = [&]() {};
    auto body = [&]() -> int32_t {
        HIPCHK(hipMemcpyAsync(d_n, n.data(), sizeof(int) * nprob, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_off, off.data(), sizeof(long long) * nprob, hipMemcpyHostToDevice, c->stream));
        for (int p = 0; p < nprob; p++)
            HIPCHK(hipMemcpyAsync(w.centres + 3 * (size_t)p * k, w.pts + 3 * off[p], sizeof(double) * 3 * k, hipMemcpyDeviceToDevice, c->stream));
        KmParams P{};
        P.pts = w.pts; P.assign = w.assign; P.centres = w.centres; P.rounds = w.rounds; P.n = d_n; P.off = d_off; P.k = k;
        hipLaunchKernelGGL(k_kmeans, dim3(nprob), dim3(1024), 0, c->stream, P);
        HIPCHK(hipGetLastError());
        centres.resize(3 * (size_t)nprob * k);
        HIPCHK(hipMemcpyAsync(centres.data(), w.centres, sizeof(double) * centres.size(), hipMemcpyDeviceToHost, c->stream));
        if (assign0) { assign0->resize(n[0]); HIPCHK(hipMemcpyAsync(assign0->data(), w.assign + off[0], sizeof(uint32_t) * n[0], hipMemcpyDeviceToHost, c->stream)); }
        HIPCHK(hipStreamSynchronize(c->stream));
        return SNES_OK;
    };
    int32_t rc = body();
    cleanup();
    return rc;
}

// lib.rs:330-405 for every subpalette in `which` (batched); colours written to the device palette
int32_t kmeans_recalculate(snesimage_ctx *c, const std::vector<uint32_t> &which) {
    if (c->perceptual) CHECK(ensure_source(c)); // per-pixel Lab
    std::vector<uint8_t> tp(1024);
    HIPCHK(hipMemcpyAsync(tp.data(), c->d_tile_pal, 1024, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint32_t wt = c->W / 8, ht = c->H / 8;
    std::vector<uint32_t> index;
    std::vector<int> n; std::vector<long long> off;
    for (uint32_t palette : which) {
        off.push_back((long long)index.size());
        for (uint32_t tile = 0; tile < 1024; tile++) {
            if (tp[tile] != palette) continue;
            const uint32_t tx = tile % wt, ty = tile / wt;
            if (ty >= ht) continue;
            for (uint32_t x = 0; x < 8; x++)
                for (uint32_t y = 0; y < 8; y++) {
                    const uint32_t px = (ty * 8 + y) * c->W + tx * 8 + x;
                    if (c->h_orig[4 * (size_t)px + 3] > 0) index.push_back(px);
                }
        }
        n.push_back((int)((long long)index.size() - off.back()));
    }
    const int k = (int)c->user_size; // (a backdrop context: the regular entries; B is not an initialiser's to move)
    for (size_t p = 0; p < n.size(); p++)
        if (!(2 <= k && k < n[p])) return fail(SNES_ERR_KMEANS, "k-means precondition 2 <= k < n violated (the reference panics here)");
    CHECK(kmeans_reserve(c, index.size() ? index.size() : 1, (int)which.size(), k));
    uint32_t *d_index = c->km.d_index; // (at most one entry per pixel)
    int32_t rc = SNES_OK;
    std::vector<double> centres;
    auto body = [&]() -> int32_t {
        HIPCHK(hipMemcpyAsync(d_index, index.data(), sizeof(uint32_t) * index.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_gather_points, dim3((unsigned)((index.size() + 255) / 256)), dim3(256), 0, c->stream, c->d_orig, c->d_labpx, d_index, (long long)index.size(), c->perceptual ? 1 : 0,
                           c->km.pts);
        HIPCHK(hipGetLastError());
        CHECK(kmeans_run(c, n, off, k, centres, nullptr));
        return SNES_OK;
    };
    rc = body();
    if (rc != SNES_OK) return rc;
    std::vector<uint8_t> col(3 * (size_t)c->ncol);
    HIPCHK(hipMemcpyAsync(col.data(), c->d_colors, col.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t p = 0; p < which.size(); p++)
        for (int i = 0; i < k; i++) host_centre_to_color(c, &centres[3 * (p * k + i)], &col[3 * ((size_t)which[p] * c->sub_size + i)]);
    HIPCHK(hipMemcpyAsync(c->d_colors, col.data(), col.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tables_valid = false; c->pack_valid = false; c->inc_valid = false; c->map_synced = false; c->epoch++; c->epoch_by_commit = false;
    return SNES_OK;
}

int32_t kmeans_recalculate_palettes(snesimage_ctx *c) { // lib.rs:407-415
    std::vector<uint32_t> which;
    for (uint32_t p = 0; p < c->sub_count; p++) which.push_back(p);
    CHECK(kmeans_recalculate(c, which));
    CHECK(do_optimize(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

// On a context with palette blocks (snesimage_set_palette_blocks) the block stands in the tile's place: sums over the block's
// pixels, points in block order (bx outer, by inner), every tile of a clustered block assigned.  At 1 x 1 a block is a tile.
int32_t kmeans_initialize_tiles(snesimage_ctx *c) { // lib.rs:79-189
    if (c->sub_count == 1) {
        CHECK(kmeans_recalculate(c, std::vector<uint32_t>{0}));
        CHECK(do_optimize(c));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SNES_OK;
    }
    if (c->perceptual) CHECK(ensure_source(c));
    const BlockGeom g = block_geom(c);
    const uint32_t wt = g.nbx, ht = g.nblock / g.nbx, ntile = g.nblock; // the units that are clustered: tiles, or blocks of them
    CHECK(kmeans_reserve(c, 1, 1, (int)c->sub_count));
    float *d_sums = c->km.d_sums; int *d_counts = c->km.d_counts; // (ntile <= 1,024)
    std::vector<float> sums(3 * (size_t)ntile); std::vector<int> counts(ntile);
    auto body0 = [&]() -> int32_t {
        hipLaunchKernelGGL(k_unit_sums, dim3((ntile + 63) / 64), dim3(64), 0, c->stream, (const uint8_t *)c->d_orig, (const float *)c->d_labpx, (int)c->W, (int)c->H, c->perceptual ? 1 : 0, g.lbw, g.lbh,
                           d_sums, d_counts);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sums.data(), d_sums, sizeof(float) * sums.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SNES_OK;
    };
    int32_t rc = body0();
    if (rc != SNES_OK) return rc;
    std::vector<double> means; std::vector<uint32_t> map;
    for (uint32_t tx = 0; tx < wt; tx++)
        for (uint32_t ty = 0; ty < ht; ty++) {
            const uint32_t index = ty * wt + tx;
            const float *s = &sums[3 * (size_t)index];
            if (s[0] + s[1] + s[2] > 0.0f) { // lib.rs:118
                for (int i = 0; i < 3; i++) means.push_back((double)s[i] / (double)counts[index]);
                map.push_back(index);
            }
        }
    const int k = (int)c->sub_count;
    std::vector<int> n{(int)map.size()}; std::vector<long long> off{0};
    if (!(2 <= k && k < n[0])) return fail(SNES_ERR_KMEANS, "k-means precondition 2 <= k < n violated (the reference panics here)");
    CHECK(kmeans_reserve(c, map.size(), 1, k));
    HIPCHK(hipMemcpyAsync(c->km.pts, means.data(), sizeof(double) * means.size(), hipMemcpyHostToDevice, c->stream));
    std::vector<double> centres; std::vector<uint32_t> assign;
    CHECK(kmeans_run(c, n, off, k, centres, &assign));
    std::vector<uint8_t> tp(1024);
    HIPCHK(hipMemcpyAsync(tp.data(), c->d_tile_pal, 1024, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < map.size(); t++) block_fill(g, tp.data(), map[t], (uint8_t)assign[t]); // lib.rs:133-138 (a unit left out keeps what it had)
    std::vector<uint8_t> col(3 * (size_t)c->ncol);
    if (c->backdrop) { HIPCHK(hipMemcpyAsync(col.data(), c->d_colors, col.size(), hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); } // (B stays)
    for (int i = 0; i < k; i++) {
        uint8_t color[3];
        host_centre_to_color(c, &centres[3 * (size_t)i], color);
        for (uint32_t j = 0; j < c->user_size; j++) memcpy(&col[3 * ((size_t)i * c->sub_size + j)], color, 3); // lib.rs:181-183
    }
    HIPCHK(hipMemcpyAsync(c->d_tile_pal, tp.data(), 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_colors, col.data(), col.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tables_valid = false; c->pack_valid = false; c->inc_valid = false; c->map_synced = false; c->epoch++; c->epoch_by_commit = false;
    CHECK(do_optimize(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SNES_OK;
}

} // namespace
