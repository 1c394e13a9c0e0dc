"""A plain binary64 restatement of `error()` (lib.rs:503-577: SSIMULACRA2 of the source against `as_rgba()`), written from
SURVEY Appendix A and the published algorithm, NOT from oracle/snes_oracle.cpp: vectorised numpy, no fused multiply-add, no
operation order to preserve and no binary32 anywhere.  tests/test_ssim2_model.py holds the oracle to it stage by stage.

Constants come from include/ssimulacra2_constants.h (the one place), read as decimal text into binary64.

Every function is usable alone.  `Model(plant=NAME)` is the same arithmetic with ONE deliberate mistake (PLANTS): the tests
use it to show that each mistake would be seen.  The module-level functions are those of `Model()`, the model proper.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANTS = (
    "odd_row_dropped",        # downscale: an odd last row (or column) left out instead of clamped
    "odd_row_zero",           # ... or averaged with zeros
    "downscale_encoded",      # 2x2 mean of the encoded values, transfer function afterwards
    "size_test_after",        # the scale loop tests the size after it has downscaled
    "border_replicate",       # blur: edge-replicated borders instead of zero padding
    "border_renormalised",    # blur: divided by the weight inside the picture
    "true_gaussian",          # blur: a normalised sampled Gaussian at sigma instead of the truncated cosines
    "no_b_minus_y",           # make_positive_xyb: B + 0.55 instead of (B - Y) + 0.55
    "x_scale_offset_swapped", # make_positive_xyb: 0.42 X + 14
    "no_c2_in_denominator",   # ssim_map: C2 in the numerator only
    "two_norm",               # pooling: a 2-norm where the 4-norm belongs
    "artifact_detail_swapped",  # edge_diff_map: the two halves exchanged
    "weights_six_scale_index",  # score: weight (c * 6 + s) * 6 ... when there are fewer than six scales
)


def header_constants():
    """{name: float or [float]} of every numeric #define of include/ssimulacra2_constants.h."""
    text = open(os.path.join(ROOT, "include", "ssimulacra2_constants.h")).read()
    out = {}
    body = re.search(r"#define SSIM2_WEIGHTS \{(.*?)\}", text, re.S).group(1).replace("\\", " ")
    out["SSIM2_WEIGHTS"] = [float(v) for v in body.split(",")]
    for name, value in re.findall(r"^#define (\w+) \(?(-?[0-9][0-9.eE+-]*)f?\)?\s*$", text, re.M):
        out[name] = float(value)
    return out


K = header_constants()
WEIGHTS = np.array(K["SSIM2_WEIGHTS"], np.float64)
assert WEIGHTS.size == 108
NUM_SCALES, MIN_SIDE = int(K["SSIM2_NUM_SCALES"]), int(K["SSIM2_MIN_SIDE"])


def _design_taps(sigma, big_n):
    """Charalampidis, "Recursive implementation of the Gaussian filter using truncated cosine functions" (2016), k = 3 terms:
    h[n] = sum_k beta_k cos(omega_k n) for |n| < N, omega_k = (2k - 1) pi / (2N), zero elsewhere (cos(omega_k N) = 0).
    The Gaussian's own cosine-series coefficients are rho_k = exp(-sigma^2 omega_k^2 / 2) / N; beta is rho moved, by the
    smallest change, onto the two conditions the design imposes: the taps sum to 1 and their second moment is sigma^2.
    Both conditions are formed here by summing over the taps, not from the paper's closed forms."""
    n = np.arange(-(big_n - 1), big_n, dtype=np.float64)
    omega = (2.0 * np.arange(1, 4) - 1.0) * np.pi / (2.0 * big_n)
    cosines = np.cos(np.outer(omega, n))                     # (3, 2N - 1)
    cond = np.stack([cosines.sum(axis=1), (cosines * n * n).sum(axis=1)])  # rows: sum of taps, second moment
    want = np.array([1.0, sigma * sigma])
    rho = np.exp(-0.5 * sigma * sigma * omega * omega) / big_n
    beta = rho + cond.T @ np.linalg.solve(cond @ cond.T, want - cond @ rho)
    return beta @ cosines


class Model:
    def __init__(self, plant=None, weight_swap=None):
        if plant is not None and plant not in PLANTS:
            raise ValueError(plant)
        self.plant = plant
        self.weights = WEIGHTS.copy()
        if weight_swap is not None:
            i, j = weight_swap
            self.weights[[i, j]] = self.weights[[j, i]]

    # ---- transfer function, downscale, colour space ---------------------------------------------------------------------------
    def eotf(self, u8):
        """sRGB decoding of 8-bit values (any shape): x / 12.92 below the threshold, ((x + 0.055) / 1.055) ^ 2.4 above."""
        x = np.asarray(u8, np.float64) / 255.0
        return self._eotf_unit(x)

    def _eotf_unit(self, x):
        hi = ((x + K["SSIM2_SRGB_OFFSET"]) / K["SSIM2_SRGB_SCALE"]) ** K["SSIM2_SRGB_GAMMA"]
        return np.where(x < K["SSIM2_SRGB_THRESHOLD"], x / K["SSIM2_SRGB_LINEAR_DIV"], hi)

    def downscale(self, lin):
        """(h, w, 3) -> (ceil(h / 2), ceil(w / 2), 3): the mean of each 2 x 2 block, the last row / column repeated when odd."""
        h, w = lin.shape[:2]
        if self.plant == "odd_row_dropped":
            lin = lin[:h - (h & 1), :w - (w & 1)]
        else:
            lin = np.pad(lin, ((0, h & 1), (0, w & 1), (0, 0)), mode="constant" if self.plant == "odd_row_zero" else "edge")
        h, w = lin.shape[:2]
        return lin.reshape(h // 2, 2, w // 2, 2, 3).mean(axis=(1, 3))

    def positive_xyb(self, lin):
        """(h, w, 3) linear RGB -> (3, h, w) planes X, Y, B of yuvxyb's linear_rgb_to_xyb followed by make_positive_xyb."""
        m00, m02, m10, m12 = K["SSIM2_OPSIN_M00"], K["SSIM2_OPSIN_M02"], K["SSIM2_OPSIN_M10"], K["SSIM2_OPSIN_M12"]
        m20, m21 = K["SSIM2_OPSIN_M20"], K["SSIM2_OPSIN_M21"]
        opsin = np.array([[m00, 1.0 - m02 - m00, m02], [m10, 1.0 - m12 - m10, m12], [m20, m21, 1.0 - m20 - m21]])
        mixed = np.maximum(np.asarray(lin, np.float64) @ opsin.T + K["SSIM2_OPSIN_BIAS"], 0.0)
        l, m, s = np.moveaxis(np.cbrt(mixed) - K["SSIM2_OPSIN_BIAS_CBRT"], -1, 0)
        x, y, b = 0.5 * (l - m), 0.5 * (l + m), s
        pb = (b if self.plant == "no_b_minus_y" else b - y) + K["SSIM2_POS_B_OFFSET"]
        if self.plant == "x_scale_offset_swapped":
            px = K["SSIM2_POS_X_OFFSET"] * x + K["SSIM2_POS_X_SCALE"]
        else:
            px = K["SSIM2_POS_X_SCALE"] * x + K["SSIM2_POS_X_OFFSET"]
        return np.stack([px, y + K["SSIM2_POS_Y_OFFSET"], pb])

    # ---- blur --------------------------------------------------------------------------------------------------------------------
    def blur_taps(self):
        """The 2N - 1 taps h[-(N - 1) .. N - 1], N = round(3.2795 sigma + 0.2546)."""
        sigma = K["SSIM2_BLUR_SIGMA"]
        big_n = int(np.floor(K["SSIM2_BLUR_RADIUS_A"] * sigma + K["SSIM2_BLUR_RADIUS_B"] + 0.5))
        if self.plant == "true_gaussian":
            n = np.arange(-(big_n - 1), big_n, dtype=np.float64)
            g = np.exp(-0.5 * n * n / (sigma * sigma))
            return g / g.sum()
        return _design_taps(sigma, big_n)

    def blur(self, plane):
        """Separable FIR of one (h, w) plane; what lies outside the plane counts as zero."""
        taps = self.blur_taps()
        out = self._fir(np.asarray(plane, np.float64), taps)
        if self.plant == "border_renormalised":
            out = out / self._fir(np.ones_like(out), taps)
        return out

    def _fir(self, a, taps):
        r = taps.size // 2
        mode = "edge" if self.plant == "border_replicate" else "constant"
        for axis in (1, 0):
            p = np.pad(a, [(r, r) if ax == axis else (0, 0) for ax in (0, 1)], mode=mode)
            n = a.shape[axis]
            a = sum(taps[j] * np.take(p, np.arange(j, j + n), axis=axis) for j in range(taps.size))
        return a

    # ---- maps and pooling -----------------------------------------------------------------------------------------------------------
    def scale_stats(self, src_xyb, dst_xyb):
        """18 values of one scale from two (3, h, w) sets of planes: per channel mean(d) and mean(d^4)^(1/4) of the SSIM map
        (6 values), then per channel the same two norms of artifact and of detail_lost (12 values: a1, a4, d1, d4)."""
        c2 = K["SSIM2_C2"]
        ssim, edge = [], []
        for i1, i2 in zip(np.asarray(src_xyb, np.float64), np.asarray(dst_xyb, np.float64)):
            mu1, mu2 = self.blur(i1), self.blur(i2)
            s11, s22, s12 = self.blur(i1 * i1), self.blur(i2 * i2), self.blur(i1 * i2)
            num_m = 1.0 - (mu1 - mu2) ** 2
            num_s = 2.0 * (s12 - mu1 * mu2) + c2
            den_s = (s11 - mu1 * mu1) + (s22 - mu2 * mu2) + (0.0 if self.plant == "no_c2_in_denominator" else c2)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.nan_to_num(np.maximum(1.0 - num_m * num_s / den_s, 0.0), nan=0.0, posinf=np.inf)
            ssim += [self._norm1(d), self._norm4(d)]
            d1 = (1.0 + np.abs(i2 - mu2)) / (1.0 + np.abs(i1 - mu1)) - 1.0
            artifact, detail_lost = np.maximum(d1, 0.0), np.maximum(-d1, 0.0)
            if self.plant == "artifact_detail_swapped":
                artifact, detail_lost = detail_lost, artifact
            edge += [self._norm1(artifact), self._norm4(artifact), self._norm1(detail_lost), self._norm4(detail_lost)]
        return np.array(ssim + edge)

    @staticmethod
    def _norm1(d):
        return float(np.mean(d))

    def _norm4(self, d):
        if self.plant == "two_norm":
            return float(np.sqrt(np.mean(d * d)))
        return float(np.mean(d ** 4) ** 0.25)

    def score_from_stats(self, stats):
        """Msssim::score of (scales, 18) statistics: the weights are consumed one after the other in the order channel ->
        scale present -> norm, three per step (ssim, artifact, detail_lost); then the cubic and the power."""
        stats = np.asarray(stats, np.float64).reshape(-1, 18)
        total, i = 0.0, 0
        for c in range(3):
            for s in range(stats.shape[0]):
                for n in range(2):
                    if self.plant == "weights_six_scale_index":
                        i = ((c * NUM_SCALES + s) * 2 + n) * 3
                    terms = (stats[s, c * 2 + n], stats[s, 6 + c * 4 + n], stats[s, 6 + c * 4 + n + 2])
                    for t in terms:
                        total += self.weights[i] * abs(t)
                        i += 1
        total *= K["SSIM2_SCORE_SCALE"]
        total = K["SSIM2_SCORE_C1"] * total + K["SSIM2_SCORE_C2"] * total ** 2 + K["SSIM2_SCORE_C3"] * total ** 3
        if total > 0.0:
            return K["SSIM2_SCORE_MAX"] + K["SSIM2_SCORE_GAIN"] * total ** K["SSIM2_SCORE_EXP"]
        return K["SSIM2_SCORE_MAX"]

    # ---- the whole -------------------------------------------------------------------------------------------------------------------
    def pyramid(self, rgba):
        """[(3, h_s, w_s)]: the positive XYB planes of every scale of an (h, w, 4) or (h, w, 3) 8-bit picture; alpha is ignored.
        At most six scales; a scale is made only from a picture that is at least 8 x 8 (tested BEFORE halving, so the last
        scale may be smaller)."""
        rgb = np.asarray(rgba)[..., :3]
        encoded = rgb.astype(np.float64) / 255.0
        lin = self.eotf(rgb)
        out = []
        for scale in range(NUM_SCALES):
            h, w = lin.shape[:2]
            if self.plant != "size_test_after" and (w < MIN_SIDE or h < MIN_SIDE):
                break
            if scale > 0:
                if self.plant == "downscale_encoded":
                    encoded = self.downscale(encoded)
                    lin = self._eotf_unit(encoded)
                else:
                    lin = self.downscale(lin)
            if self.plant == "size_test_after" and (lin.shape[1] < MIN_SIDE or lin.shape[0] < MIN_SIDE):
                break
            out.append(self.positive_xyb(lin))
        return out

    def stats(self, src_rgba, dst_rgba):
        return np.array([self.scale_stats(a, b) for a, b in zip(self.pyramid(src_rgba), self.pyramid(dst_rgba))])

    def error(self, src_rgba, dst_rgba):
        """lib.rs:547: 100 - SSIMULACRA2(source, reconstruction).  `dst_rgba` is what as_rgba() returns: transparent pixels
        are already black there, while the source keeps its RGB."""
        return 100.0 - self.score_from_stats(self.stats(src_rgba, dst_rgba))


_M = Model()
eotf, downscale, positive_xyb, blur_taps, blur = _M.eotf, _M.downscale, _M.positive_xyb, _M.blur_taps, _M.blur
scale_stats, score_from_stats, pyramid, stats, error = _M.scale_stats, _M.score_from_stats, _M.pyramid, _M.stats, _M.error
