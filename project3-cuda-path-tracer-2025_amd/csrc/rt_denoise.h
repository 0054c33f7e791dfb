// rt_denoise.h — what the denoiser's entry points share (rt_abi_denoise.h, rt_abi_gbuffer_through.h,
// rt_abi_temporal.h, rt_abi_regress.h).
//
// Owns: denoise_ctx, g_dn_timing / denoise_event, the argument checks (check_*), copy_planes,
// result_out, and atrous_levels, the one driver of the a-trous filter's levels.
// Calls: rt_core.h (State::dn, the DenoiseState), M.n of rt_multi.h, the k_atrous_* kernels of
// pt_denoise_kernels.h.

bool g_dn_timing = false;   // pt_debug_denoise_timing

int32_t denoise_ctx(const char* what) {
    RC(need_init());
    if (M.n > 1 || gp->opts.shard_mode != PT_SHARD_NONE)
        return fail(PT_E_UNSUPPORTED, "%s: one unsharded device context only (num_devices > 1 or shard_mode set)", what);
    return PT_OK;
}
// record event k of one of DenoiseState's arrays (ev, tp_ev, rg_ev), created on first use
int32_t denoise_event(hipEvent_t* events, int k) {
    if (!events[k]) HIPCHK(hipEventCreate(&events[k]));
    HIPCHK(hipEventRecord(events[k], gp->stream));
    return PT_OK;
}

// ---- argument checks; what: the entry point's name, for the message ----
int32_t check_positive(const char* what, const char* name, float v) {
    if (!(v > 0.0f) || !std::isfinite(v)) return fail(PT_E_INVALID, "%s: %s must be positive and finite", what, name);
    return PT_OK;
}
int32_t check_params(const char* what, const pt_denoise_params& p) {
    if (p.levels < 1 || p.levels > PT_DENOISE_MAX_LEVELS)
        return fail(PT_E_INVALID, "%s: levels must be 1 .. %d, got %d", what, PT_DENOISE_MAX_LEVELS, p.levels);
    RC(check_positive(what, "sigma_color", p.sigma_color));
    RC(check_positive(what, "sigma_normal", p.sigma_normal));
    return check_positive(what, "sigma_position", p.sigma_position);
}
int32_t check_samples(const char* what, int32_t samples) {
    if (samples < 1) return fail(PT_E_INVALID, "%s: samples must be >= 1, got %d", what, samples);
    return PT_OK;
}
int32_t check_captured(const char* what) {
    if (!gp->dn.gbuf_valid)
        return fail(PT_E_STATE, "%s: no feature buffer captured for this camera (pt_gbuffer_capture)", what);
    return PT_OK;
}

// the getters: room for the image's pixels, then the planes src[0 .. k) to the non-null dst[]
template <class T, class S>
int32_t copy_planes(const char* what, int64_t n_pixels, int k, T* const* dst, S* const* src) {
    if (n_pixels < gp->pixels_total)
        return fail(PT_E_INVALID, "%s: room for %lld pixels, the image has %d", what, (long long)n_pixels, gp->pixels_total);
    for (int i = 0; i < k; ++i)
        if (dst[i]) HIPCHK(smemcpy(dst[i], src[i], sizeof(S) * (size_t)gp->pixels_total, hipMemcpyDeviceToHost));
    return PT_OK;
}
// the end of a filter call: its float3 result to the caller, if asked for, and the stream drained
int32_t result_out(float* host_out, const float* out3) {
    if (host_out)
        HIPCHK(hipMemcpyAsync(host_out, out3, sizeof(float) * 3 * (size_t)gp->pixels_total, hipMemcpyDeviceToHost, gp->stream));
    HIPCHK(hipStreamSynchronize(gp->stream));
    return PT_OK;
}

// ---- the a-trous levels ----
float inv_sq(double s) { return (float)std::min(1.0 / (s * s), 3.0e38); }

// what every level of a filter call shares: the captured planes, the image's size, the colour
// domain and the normal and position factors (AtrousArgsVar is an AtrousArgs)
void atrous_common(AtrousArgs& a, const pt_denoise_params& p, int32_t samples) {
    float4* const* cur = gp->dn.d_gbuf[gp->dn.gbuf_cur];
    a.gn = cur[0];
    a.gx = cur[1];
    a.ga = cur[2];
    a.W = gp->width;
    a.H = gp->height;
    a.demod = p.demodulate_albedo != 0;
    a.samples = (float)samples;
    a.k_normal = inv_sq(p.sigma_normal);
    a.k_position = inv_sq(p.sigma_position);
}

// level l's kernel: steps 1 and 2 from LDS, the wider ones direct (pt_denoise_kernels.h)
auto atrous_kernel(const AtrousArgs&, int l) { return l == 0 ? k_atrous_lds<1> : l == 1 ? k_atrous_lds<2> : k_atrous_direct; }
auto atrous_kernel(const AtrousArgsVar&, int l) {
    return l == 0 ? k_atrous_lds_var<1> : l == 1 ? k_atrous_lds_var<2> : k_atrous_direct_var;
}

// The levels of one filter call, pt_denoise's (AtrousArgs) or pt_denoise_temporal's (AtrousArgsVar).
// a: what holds for every level; first_in: level 0's input plane, or null for the image (a.first on
// level 0 then, and on no level otherwise); per_level(a, l): called before level l's launch, sets
// the level's own scalar and may record an event.  *out3: where the last level left the result.
template <class Args, class F>
int32_t atrous_levels(Args a, const float4* first_in, int levels, pt_uchar4* pbo, F&& per_level, float** out3) {
    float4* const* color = gp->dn.d_color;
    const dim3 grid((a.W + AT_TILE - 1) / AT_TILE, (a.H + AT_TILE - 1) / AT_TILE);
    for (int l = 0; l < levels; ++l) {
        a.first = l == 0 && !first_in;
        a.last = l == levels - 1;
        a.step = 1 << l;
        a.cin = l > 0 ? color[(l - 1) & 1] : first_in;
        a.cout = a.last ? nullptr : color[l & 1];
        // the last level stores float3 per pixel, in the colour buffer it would have written
        a.out3 = *out3 = a.last ? reinterpret_cast<float*>(color[l & 1]) : nullptr;
        a.pbo = a.last ? pbo : nullptr;
        RC(per_level(a, l));
        hipLaunchKernelGGL(atrous_kernel(a, l), grid, dim3(BLOCK), 0, gp->stream, a);
        HIPCHK(hipGetLastError());
    }
    return PT_OK;
}

