/*
 * pt_denoise_regress.h — blockwise feature regression (after BMFR, Koskela et al. 2019): a second
 * spatial filter beside the a-trous wavelet of pt_denoise.h.  In every image block the noisy colour
 * is fitted by ridge-regularised least squares as a linear function of the noise-free guides a
 * capture already holds (normal, position), and the fit is the output: a radiance gradient along a
 * wall is a linear function of the position features and survives, and a non-finite pixel is filled
 * from its block's fit.  A framework addition like pt_denoise: it reads the accumulated image and
 * the planes of the last pt_gbuffer_capture or pt_gbuffer_capture_through (any K) and writes
 * neither.
 *
 *   pt_denoise_regress   k_regress_fit (one launch, one workgroup per block) + k_regress_apply
 *
 * Colour.  c0(p) = image(p) / samples; with demodulate_albedo, hit pixels hold
 * c0 / max(albedo, 1e-3) per channel, as in pt_denoise.h.
 *
 * Pixel classes.  A surface pixel has hit flag 1 and a material of emittance 0.  A sample is a
 * surface pixel whose c0 is finite in all three channels.  Every other pixel (a miss or an emitter)
 * passes through: out(p) = c0(p) if all three channels are finite, else 0, and then the albedo back
 * where it was divided out.
 *
 * Blocks are 32 x 32 pixels on a 16-pixel stride.  Block (i, j), i = 0 .. ceil(W / 16),
 * j = 0 .. ceil(H / 16), covers x in [16 i - 16, 16 i + 16), y in [16 j - 16, 16 j + 16), clipped
 * to the image: every pixel lies in four blocks.  n is the block's number of samples, lo and hi the
 * per-axis minimum and maximum of the samples' positions, xs = (x - lo) / (hi - lo) per axis (0 on
 * an axis where hi = lo), and the feature row of a pixel is
 *
 *   f = (1, n.x, n.y, n.z, xs.x, xs.y, xs.z, xs.x^2, xs.y^2, xs.z^2)
 *
 * Fit, per block with n >= 1: beta (10 x 3) solves (F^T F + ridge n D) beta = F^T C over the
 * block's samples, D = diag(0, 1, ..., 1): the constant column is not penalised, and the matrix is
 * positive definite for every n >= 1.  A block with n = 0 has no fit.
 *
 * Output at a surface pixel p = (x, y): over the blocks b = (i, j) that contain p and have a fit, in
 * (j, i) ascending order, with w_b = (1 - |x - (16 i - 1/2)| / 16) (1 - |y - (16 j - 1/2)| / 16),
 *
 *   out(p) = sum w_b max(0, f_b(p) . beta_b) / sum w_b      (0 when no such block has a fit)
 *
 * f_b(p) is formed with block b's lo and hi; at a surface pixel that is no sample xs may lie outside
 * [0, 1].  The albedo is multiplied back where it was divided out.  Non-finite inputs never reach
 * the output: the factorisation keeps every pivot at or above its exact lower bound (n for the
 * constant, ridge n for the others) whatever float32 rounding does to it at a very small ridge, and
 * a fitted value that is not finite counts as 0.  No atomics on floating-point data and a fixed
 * order: two calls give the same bytes.
 *
 * Contexts, errors and outputs are those of pt_denoise: one unsharded device context, not in naive
 * mesh mode (PT_E_UNSUPPORTED); PT_E_STATE without a valid capture; all work on the context's own
 * stream, a speculated next frame is neither cancelled nor disturbed.  The block table is allocated
 * at the first call and freed by pt_free; the result uses the colour buffers of pt_denoise.
 */
#ifndef PT_DENOISE_REGRESS_H
#define PT_DENOISE_REGRESS_H

#include <stdint.h>

#include "pt/pathtrace_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_REGRESS_BLOCK_FLOATS 37   /* pt_regress_get: n | lo.xyz | hi.xyz | beta[10][3] */

typedef struct pt_regress_params {
    float   ridge;             /* default 1e-3; > 0 and finite */
    int32_t demodulate_albedo; /* default 1, as pt_denoise */
} pt_regress_params;

void    pt_regress_default_params(pt_regress_params*);

/* Fit and blend (accumulated image / samples), guided by the captured planes.
 *   host_out[w*h*3] = the regressed mean radiance                          (or NULL)
 *   pbo_device      = sendImageToPBO of the result with iteration 1        (or NULL)
 * p NULL: the defaults.  Never writes the accumulated image.  Returns when the result is complete.
 * PT_E_INVALID: samples < 1, a ridge that is <= 0 or not finite. */
int32_t pt_denoise_regress(const pt_regress_params* p, int32_t samples, pt_uchar4* pbo_device, float* host_out);

/* Host copy of the last call's per-block fit, for tests and tools: PT_REGRESS_BLOCK_FLOATS floats per
 * block, blocks in (j, i) row-major order, (ceil(H/16) + 1) x (ceil(W/16) + 1) of them: n | lo.xyz |
 * hi.xyz | 10 x 3 coefficients (feature-major).  A block with n = 0 holds zeros.  PT_E_STATE before
 * the first call; PT_E_INVALID with room for fewer blocks than the image has. */
int32_t pt_regress_get(float* blocks, int64_t n_blocks);

/* Tools (tools/denoise_probe.py --regress): with pt_debug_denoise_timing enabled, the last call's
 * kernel times from HIP events on the context's stream.  Either pointer may be NULL. */
int32_t pt_debug_regress_times(float* fit_ms, float* apply_ms);

#ifdef __cplusplus
}
#endif
#endif /* PT_DENOISE_REGRESS_H */
