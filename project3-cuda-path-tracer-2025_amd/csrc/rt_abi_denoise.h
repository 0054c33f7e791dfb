// rt_abi_denoise.h — the denoiser's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_gbuffer_*, pt_denoise*, pt_debug_denoise_*.  Calls: rt_core.h, M.n of rt_multi.h, and
// the kernels of pt_denoise_kernels.h.

// ---------------------------------------------------------------------------------------------
// denoiser (include/pt/pt_denoise.h): first-hit feature planes + the a-trous filter
// ---------------------------------------------------------------------------------------------
static bool g_dn_timing = false;   // pt_debug_denoise_timing

static int32_t denoise_ctx(const char* what) {
    RC(need_init());
    if (M.n > 1 || gp->opts.shard_mode != PT_SHARD_NONE)
        return fail(PT_E_UNSUPPORTED, "%s: one unsharded device context only (num_devices > 1 or shard_mode set)", what);
    return PT_OK;
}
static int32_t denoise_event(int k) {
    if (!gp->dn_ev[k]) HIPCHK(hipEventCreate(&gp->dn_ev[k]));
    HIPCHK(hipEventRecord(gp->dn_ev[k], gp->stream));
    return PT_OK;
}

void pt_denoise_default_params(pt_denoise_params* p) {
    if (!p) return;
    p->levels = 5;
    p->sigma_color = 0.45f;
    p->sigma_normal = 0.35f;
    p->sigma_position = 0.20f;
    p->demodulate_albedo = 1;
}

int32_t pt_gbuffer_capture(int32_t iteration) {
    RC(denoise_ctx("pt_gbuffer_capture"));
    if (gp->naive) return fail(PT_E_UNSUPPORTED, "pt_gbuffer_capture: not available in naive mesh mode");
    if (iteration <= 0) return fail(PT_E_INVALID, "iteration is 1-based, got %d", iteration);
    const int n = gp->pixels_total;
    gp->gbuf_valid = false;
    if (!gp->d_gbuf[0]) {
        for (float4*& p : gp->d_gbuf) RC(dalloc(&p, (size_t)n));
        for (float4*& p : gp->d_dn_color) RC(dalloc(&p, (size_t)n));
    }
    const GBuf g{gp->d_gbuf[0], gp->d_gbuf[1], gp->d_gbuf[2]};
    if (g_dn_timing) RC(denoise_event(0));
    // the traversal pt_test_intersect (and the staged pipeline) runs for this context's options
    if (gp->has_bvh && (gp->opts.variant & VAR_BVH_FAST))
        hipLaunchKernelGGL((k_gbuffer<true, true>), dim3(nblocks(n)), dim3(BLOCK), gp->bvh_lds, gp->stream, gp->sc, g,
                           iteration, n);
    else if (gp->has_bvh)
        hipLaunchKernelGGL((k_gbuffer<true, false>), dim3(nblocks(n)), dim3(BLOCK), gp->bvh_lds, gp->stream, gp->sc, g,
                           iteration, n);
    else
        hipLaunchKernelGGL((k_gbuffer<false, false>), dim3(nblocks(n)), dim3(BLOCK), 0, gp->stream, gp->sc, g, iteration, n);
    HIPCHK(hipGetLastError());
    if (g_dn_timing) RC(denoise_event(1));
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (g_dn_timing) HIPCHK(hipEventElapsedTime(&gp->dn_capture_ms, gp->dn_ev[0], gp->dn_ev[1]));
    gp->gbuf_valid = true;
    return PT_OK;
}

int32_t pt_gbuffer_get(float* normal_t, float* position, float* albedo_mat, int64_t n_pixels) {
    RC(denoise_ctx("pt_gbuffer_get"));
    if (!gp->gbuf_valid) return fail(PT_E_STATE, "pt_gbuffer_get: no feature buffer captured for this camera");
    if (n_pixels < gp->pixels_total) return fail(PT_E_INVALID, "pt_gbuffer_get: room for %lld pixels, the image has %d",
                                                 (long long)n_pixels, gp->pixels_total);
    float* dst[3] = {normal_t, position, albedo_mat};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) HIPCHK(smemcpy(dst[k], gp->d_gbuf[k], sizeof(float4) * (size_t)gp->pixels_total, hipMemcpyDeviceToHost));
    return PT_OK;
}

int32_t pt_denoise(const pt_denoise_params* params, int32_t samples, pt_uchar4* pbo, float* host_out) {
    RC(denoise_ctx("pt_denoise"));
    pt_denoise_params p;
    if (params) p = *params;
    else pt_denoise_default_params(&p);
    if (p.levels < 1 || p.levels > PT_DENOISE_MAX_LEVELS)
        return fail(PT_E_INVALID, "pt_denoise: levels must be 1 .. %d, got %d", PT_DENOISE_MAX_LEVELS, p.levels);
    const float sig[3] = {p.sigma_color, p.sigma_normal, p.sigma_position};
    const char* sig_name[3] = {"sigma_color", "sigma_normal", "sigma_position"};
    for (int k = 0; k < 3; ++k)
        if (!(sig[k] > 0.0f) || !std::isfinite(sig[k]))
            return fail(PT_E_INVALID, "pt_denoise: %s must be positive and finite", sig_name[k]);
    if (samples < 1) return fail(PT_E_INVALID, "pt_denoise: samples must be >= 1, got %d", samples);
    if (!gp->gbuf_valid)
        return fail(PT_E_STATE, "pt_denoise: no feature buffer captured for this camera (pt_gbuffer_capture)");
    auto inv_sq = [](double s) { return (float)std::min(1.0 / (s * s), 3.0e38); };
    AtrousArgs a{};
    a.image = gp->d_image;
    a.gn = gp->d_gbuf[0];
    a.gx = gp->d_gbuf[1];
    a.ga = gp->d_gbuf[2];
    a.W = gp->width;
    a.H = gp->height;
    a.demod = p.demodulate_albedo != 0;
    a.samples = (float)samples;
    a.k_normal = inv_sq(p.sigma_normal);
    a.k_position = inv_sq(p.sigma_position);
    const dim3 grid((a.W + AT_TILE - 1) / AT_TILE, (a.H + AT_TILE - 1) / AT_TILE);
    float* out3 = nullptr;
    for (int l = 0; l < p.levels; ++l) {
        a.first = l == 0;
        a.last = l == p.levels - 1;
        a.step = 1 << l;
        a.cin = l > 0 ? gp->d_dn_color[(l - 1) & 1] : nullptr;
        a.cout = a.last ? nullptr : gp->d_dn_color[l & 1];
        // the last level stores float3 per pixel, in the colour buffer it would have written
        a.out3 = out3 = a.last ? reinterpret_cast<float*>(gp->d_dn_color[l & 1]) : nullptr;
        a.pbo = a.last ? pbo : nullptr;
        a.k_color = inv_sq((double)p.sigma_color * std::ldexp(1.0, -l));
        if (g_dn_timing) RC(denoise_event(2 + l));
        if (l == 0) hipLaunchKernelGGL(k_atrous_lds<1>, grid, dim3(BLOCK), 0, gp->stream, a);
        else if (l == 1) hipLaunchKernelGGL(k_atrous_lds<2>, grid, dim3(BLOCK), 0, gp->stream, a);
        else hipLaunchKernelGGL(k_atrous_direct, grid, dim3(BLOCK), 0, gp->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (g_dn_timing) RC(denoise_event(2 + p.levels));
    if (host_out)
        HIPCHK(hipMemcpyAsync(host_out, out3, sizeof(float) * 3 * (size_t)gp->pixels_total, hipMemcpyDeviceToHost, gp->stream));
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (g_dn_timing) {
        HIPCHK(hipEventElapsedTime(&gp->dn_ms, gp->dn_ev[2], gp->dn_ev[2 + p.levels]));
        for (int l = 0; l < PT_DENOISE_MAX_LEVELS; ++l) {
            gp->dn_level_ms[l] = 0.f;
            if (l < p.levels) HIPCHK(hipEventElapsedTime(&gp->dn_level_ms[l], gp->dn_ev[2 + l], gp->dn_ev[3 + l]));
        }
    }
    return PT_OK;
}

int32_t pt_debug_denoise_timing(int32_t enabled) {
    g_dn_timing = enabled != 0;
    return PT_OK;
}

int32_t pt_debug_denoise_times(float* capture_ms, float* denoise_ms, float* level_ms) {
    RC(need_init());
    if (capture_ms) *capture_ms = gp->dn_capture_ms;
    if (denoise_ms) *denoise_ms = gp->dn_ms;
    if (level_ms) memcpy(level_ms, gp->dn_level_ms, sizeof gp->dn_level_ms);
    return PT_OK;
}

