/*
 * pt_denoise.h — an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) for the few-spp
 * images of an interactive session, guided by a first-hit feature buffer (normal, position,
 * albedo).  A framework addition beside the reference's boundary: it runs after the wavefront,
 * reads the accumulated image and never writes it, so nothing the path tracer computes changes.
 *
 *   pt_gbuffer_capture   k_gbuffer: generateRayFromCamera(iteration) + computeIntersections for
 *                        every pixel -- the production camera, primitive, BVH and finish_hit code
 *   pt_denoise           k_atrous, one launch per level (tap step 1, 2, 4, ...)
 *
 * The filter.  c0(p) = image(p) / samples; with demodulate_albedo, hit pixels hold
 * c0 / max(albedo, 1e-3) per channel (miss pixels are left as they are).  Level l = 0..levels-1
 * has tap step s = 2^l and taps q = p + s (i, j), i, j in -2..2, in row-major (j, i) order; taps
 * outside the image are skipped.  With h = {1/16, 1/4, 3/8, 1/4, 1/16} and sc_l = sigma_color 2^-l
 *
 *   w = h[i] h[j] exp(-|c(p) - c(q)|^2 / sc_l^2) exp(-|n(p) - n(q)|^2 / sigma_normal^2)
 *                 exp(-|x(p) - x(q)|^2 / sigma_position^2)
 *
 * w = 0 when the hit flags of p and q differ (two misses: the normal and position terms are 1);
 * a tap whose colour has a non-finite channel gets w = 0; at a non-finite centre the colour term
 * is 1 for every tap (and the centre tap itself gets 0).  The level's output is
 * sum w c(q) / sum w, or 0 when sum w = 0.  After the last level the albedo is multiplied back
 * where it was divided out.  Tap order is fixed and there are no atomics: the result is
 * deterministic.
 *
 * One device context only: with pt_options.num_devices > 1 or shard_mode != PT_SHARD_NONE the
 * three calls return PT_E_UNSUPPORTED.  The feature planes and two colour buffers are allocated
 * at the first pt_gbuffer_capture and freed by pt_free.  All work is queued on the context's own
 * stream; a speculated next frame (pt_set_speculation) is neither cancelled nor disturbed.
 * Errors: PT_E* codes of pathtrace_abi.h, message in pt_last_error().
 */
#ifndef PT_DENOISE_H
#define PT_DENOISE_H

#include <stdint.h>

#include "pt/pathtrace_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_DENOISE_MAX_LEVELS 8

typedef struct pt_denoise_params {
    int32_t levels;            /* a-trous passes, tap step 1,2,4,...; 1..8, default 5 */
    float   sigma_color;       /* default 0.45 (on mean radiance; halves every level) */
    float   sigma_normal;      /* default 0.35 */
    float   sigma_position;    /* default 0.20 (scene units) */
    int32_t demodulate_albedo; /* default 1: filter colour / albedo, multiply back after */
} pt_denoise_params;

void    pt_denoise_default_params(pt_denoise_params*);

/* First hit of generateRayFromCamera(iteration) for every pixel, into library-owned planes. */
int32_t pt_gbuffer_capture(int32_t iteration);

/* Host copies; any pointer may be NULL.
 *   normal_t[4n]     = normal.xyz | t          (t = -1 and normal 0 on a miss)
 *   position[4n]     = origin + t*dir | hit flag 1.0/0.0   (0 on a miss)
 *   albedo_mat[4n]   = albedo.rgb | materialId as float    (0, -1 on a miss)
 * PT_E_STATE without a captured buffer. */
int32_t pt_gbuffer_get(float* normal_t, float* position, float* albedo_mat, int64_t n_pixels);

/* Filter (accumulated image / samples), guided by the captured planes.
 *   host_out[w*h*3] = denoised mean radiance                               (or NULL)
 *   pbo_device      = sendImageToPBO of the result with iteration 1, i.e.
 *                     clamp(int(c*255))                                    (or NULL)
 * p NULL: the defaults.  Never writes the accumulated image.  Returns when the result is complete.
 * PT_E_STATE without a captured buffer, or with a buffer captured before the last pt_init or
 * before a pt_set_camera that changed the camera.  PT_E_INVALID: levels outside 1..8, a sigma
 * that is <= 0 or not finite, samples < 1. */
int32_t pt_denoise(const pt_denoise_params* p, int32_t samples, pt_uchar4* pbo_device, float* host_out);

/* Tools (tools/denoise_probe.py): with timing enabled, HIP events on the context's stream bracket
 * k_gbuffer and every k_atrous launch; pt_debug_denoise_times returns the last capture's time, the
 * last pt_denoise's kernel time (first launch to last, no host copy) and its per-level times
 * (level_ms holds PT_DENOISE_MAX_LEVELS floats, 0 past the levels run).  Any pointer may be NULL. */
int32_t pt_debug_denoise_timing(int32_t enabled);
int32_t pt_debug_denoise_times(float* capture_ms, float* denoise_ms, float* level_ms);

#ifdef __cplusplus
}
#endif
#endif /* PT_DENOISE_H */
