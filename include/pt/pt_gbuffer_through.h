/*
 * pt_gbuffer_through.h — feature planes of the first NON-SPECULAR surface a camera ray reaches
 * (primary-surface replacement), for the denoiser of include/pt/pt_denoise.h.  On a mirror or a
 * piece of glass the first hit is the smooth surface itself: its normal and position vary slowly
 * and its albedo is the material's white, so nothing stops the filter from blurring what is seen
 * in or through it.  A through-capture follows the camera ray through perfectly specular surfaces
 * and records the guides of the surface it ends on.  A framework addition like the rest of the
 * denoiser: it reads nothing the wavefront writes and changes nothing it computes.
 *
 * Definition.  For every pixel start with camera_ray(iteration) (generateRayFromCamera) and
 * K = max_specular, followed = 0, t_sum = 0, and repeat:
 *
 *   1. intersect the scene with the production intersection of the context's options (the code
 *      pt_gbuffer_capture runs: computeIntersections, hit at parameter t); t_sum = t_sum + t in
 *      float32 on a hit
 *   2. a miss: the pixel holds the miss sentinels pt_gbuffer_get documents; stop
 *   3. the hit material is DELTA when emittance <= 0 and (hasReflective > 0 or hasRefractive > 0)
 *   4. not delta, or followed == K: this is the recorded surface; stop
 *   5. otherwise followed = followed + 1 and the ray continues with scatterRay's own arithmetic
 *      for that material, on a fixed branch that draws no random number:
 *        hasRefractive > 0   the transmissive branch: sampleFSpecularTrans with its fallback to a
 *                            reflection on total internal reflection, direction normalised,
 *                            origin = intersect + direction * 0.001.  Glass (hasReflective > 0 as
 *                            well) takes this branch too: it always refracts
 *        otherwise           the mirror branch: reflect, origin = intersect + normal * 0.00001
 *      with intersect = origin + t * direction, and the normal perturbed by the material's bump
 *      map exactly as kernShadeMaterialProper perturbs it before scatterRay.  Throughput is not
 *      tracked.
 *
 * The planes of pt_gbuffer_get then hold, for a pixel that ended on a surface,
 *   normal_t     the recorded surface's normal | t_sum (the segments' t added in chain order)
 *   position     the last segment's origin + t * direction (rounded as the shader rounds it) | 1
 *   albedo_mat   the recorded surface's albedo (colour or base-colour texel) | its materialId
 * and a fourth plane (pt_gbuffer_get_chain) holds `followed`, 0..K, for every pixel -- for a
 * chain that ended in a miss, the surfaces it followed before.  A pixel that reaches the cap on a
 * delta surface carries that surface's own guides and followed = K.  With max_specular = 0 the
 * three planes are byte-identical to pt_gbuffer_capture's.
 *
 * The chain is deterministic (every ray writes only its own pixel), so two captures of one
 * iteration give identical bytes.  pt_gbuffer_get and pt_denoise work unchanged on a
 * through-capture, with the same invalidation rules.  pt_denoise_temporal does not: its
 * reprojection projects the recorded position through the pinhole camera, which is wrong behind a
 * reflection or refraction, so after a through-capture with max_specular > 0 it returns
 * PT_E_UNSUPPORTED (a capture with max_specular = 0 or pt_gbuffer_capture lifts that).
 *
 * Two ray queues of 32 B per pixel and the `followed` plane are allocated at the first
 * through-capture and freed by pt_free.  All work is queued on the context's own stream; a
 * speculated next frame is neither cancelled nor waited for.  Errors: PT_E_INVALID for
 * max_specular outside 0..PT_GBUFFER_THROUGH_MAX or iteration < 1; PT_E_UNSUPPORTED where
 * pt_gbuffer_capture returns it (several devices, shards, naive mesh mode).
 */
#ifndef PT_GBUFFER_THROUGH_H
#define PT_GBUFFER_THROUGH_H

#include <stdint.h>

#include "pt/pt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_GBUFFER_THROUGH_MAX 8

/* The planes of the first non-specular surface behind up to max_specular delta surfaces. */
int32_t pt_gbuffer_capture_through(int32_t iteration, int32_t max_specular);

/* Host copy of the `followed` plane of the last through-capture, one int32 per pixel.
 * PT_E_STATE unless the captured buffer is a through-capture's. */
int32_t pt_gbuffer_get_chain(int32_t* followed, int64_t n_pixels);

#ifdef __cplusplus
}
#endif
#endif /* PT_GBUFFER_THROUGH_H */
