/*
 * pt_denoise_temporal.h — a temporal stage in front of the a-trous filter of pt_denoise.h: the two
 * SVGF stages (Schied et al. 2017) a progressive path tracer with a spatial filter is expected to
 * have.  History is reprojected through camera changes, and a per-pixel variance estimate tells the
 * spatial filter how hard to smooth.  Like the denoiser it reads the accumulated image and never
 * writes it.
 *
 *   pt_denoise_temporal   k_reproject (once per capture), k_temporal_integrate, then the a-trous
 *                         levels of pt_denoise.h with a variance-normalised colour term
 *
 * Colours are in the filter's domain: c0(p) = image(p) / samples, divided by max(albedo, 1e-3) at
 * hit pixels when demodulate_albedo is set.  L(c) = 0.2126 r + 0.7152 g + 0.0722 b.
 *
 * State.  HISTORY: the integrated colour, moments and sample count of the last pt_denoise_temporal
 * call, with the feature planes and the camera that call ran under.  The feature planes are double
 * buffered: a pt_gbuffer_capture that would overwrite planes the history refers to writes the other
 * set.  BASE: the history reprojected into the current capture's pixel grid, computed once per
 * capture by the first pt_denoise_temporal call after it (with that call's max_history,
 * normal_cos_min and plane_tol).  Later calls under the same capture reuse the base and recompute
 * the integration from base + current image, so repeating a call counts nothing twice.  pt_init,
 * pt_free, pt_temporal_reset and a change of demodulate_albedo between calls drop the history.
 *
 * Stage 1, reprojection.  A pixel p with hit flag 1 has X = position(p), n = normal(p), t and
 * material m.  With the history's camera (position P, view, right, up, pixelLength, resolution):
 * v = X - P, d = v.view; no history for p if d <= 1e-6;
 *   u = -(v.right) / (d plx) + resx / 2 - 0.5,   w = -(v.up) / (d ply) + resy / 2 - 0.5
 * (the inverse of the camera ray's pixel point for a pinhole at P: the aperture offset and the
 * sub-pixel jitter of the history's samples are ignored).  x0 = floor(u), fx = u - x0, likewise
 * y0, fy; the four taps q = (x0 + i, y0 + j) carry the bilinear weights.  A tap is valid iff it is
 * inside the image, the history's hit flag at q is 1 and its material equals m,
 * n.n_hist(q) >= normal_cos_min, |(x_hist(q) - X).n| <= plane_tol t, and the history colour at q is
 * finite with a count > 0.  W = sum of the valid weights.  W < 1e-3: p has no history (colour,
 * moments and N_base are 0).  Otherwise base colour, mu1 and mu2 are the W-normalised sums and
 * N_base = min(normalised sum of counts, max_history).  Miss pixels and calls without history have
 * N_base = 0.
 *
 * Stage 2, integration and variance.  N = N_base + samples, a = samples / N,
 * colour = (1 - a) base + a c0; mu1 and mu2 are blended likewise with L(c0) and L(c0)^2.  A
 * non-finite c0 leaves the base value with N = N_base; if N_base is 0 too the pixel is stored as
 * 0 0 0 | 0, the filter's mark of a non-finite colour.  variance = max(0, mu2 - mu1^2) where
 * N_base >= variance_history_min; elsewhere the spatial estimate mean(L^2) - mean(L)^2, clamped at
 * 0, of c0 over the 7 x 7 window around p, clipped to the image and restricted to finite pixels
 * with p's hit flag and material (0 when there is none).
 *
 * Stage 3, the a-trous levels of pt_denoise.h, from the integrated colour.  Level l's colour
 * exponent is |c(p) - c(q)|^2 / (sv_l^2 (variance(p) + 1e-6)), sv_l = sigma_variance 2^-l
 * (sigma_color is checked but not used).  Everything else is as pt_denoise defines it: normal and
 * position terms, hit-flag and non-finite rules, tap order, albedo multiplied back, outputs.
 * The integrated planes, not the filtered output, become the history.
 *
 * One unsharded device context only, and not in naive mesh mode (PT_E_UNSUPPORTED), as pt_denoise.
 * PT_E_UNSUPPORTED as well after a through-capture with max_specular > 0
 * (include/pt/pt_gbuffer_through.h): the reprojection projects the recorded position through the
 * pinhole camera, which is wrong for a surface seen in a mirror or through glass.
 * Memory: one more set of three feature planes and four float4 planes (base and integrated colour
 * and moments; the history lives in the integrated planes until the next capture's reprojection
 * has read it), allocated at the first call and freed by pt_free.
 */
#ifndef PT_DENOISE_TEMPORAL_H
#define PT_DENOISE_TEMPORAL_H

#include <stdint.h>

#include "pt/pt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_temporal_params {
    int32_t max_history;          /* default 32: cap on the history's sample count */
    float   normal_cos_min;       /* default 0.9 */
    float   plane_tol;            /* default 0.02 (relative to the pixel's t) */
    int32_t variance_history_min; /* default 4: below it the variance is estimated spatially */
    float   sigma_variance;       /* default 4.0: colour sigma in standard deviations, halves every level */
} pt_temporal_params;

void    pt_temporal_default_params(pt_temporal_params*);

/* Drop all history. */
int32_t pt_temporal_reset(void);

/* Reproject (first call after a capture), integrate, filter.  Outputs as pt_denoise's; p / t NULL:
 * the defaults.  Errors: the codes and conditions of pt_denoise, and PT_E_INVALID for
 * max_history < 1, normal_cos_min outside [-1, 1], plane_tol or sigma_variance not positive and
 * finite, variance_history_min < 0. */
int32_t pt_denoise_temporal(const pt_denoise_params* p, const pt_temporal_params* t, int32_t samples,
                            pt_uchar4* pbo_device, float* host_out);

/* Host copies of the last call's planes; any pointer may be NULL; 4 floats per pixel each:
 *   base_color = reprojected history rgb | N_base      base_moments = mu1, mu2, 0, 0
 *   color      = integrated rgb | N                    moments      = mu1, mu2, variance, 0
 * PT_E_STATE before the first pt_denoise_temporal call. */
int32_t pt_temporal_get(float* base_color, float* base_moments, float* color, float* moments, int64_t n_pixels);

/* Tools (tools/denoise_probe.py): with pt_debug_denoise_timing enabled, the last call's kernel
 * times from HIP events on the context's stream: reprojection (0 when the base was reused),
 * integration + variance, and the a-trous levels together.  Any pointer may be NULL. */
int32_t pt_debug_temporal_times(float* reproject_ms, float* integrate_ms, float* levels_ms);

#ifdef __cplusplus
}
#endif
#endif /* PT_DENOISE_TEMPORAL_H */
