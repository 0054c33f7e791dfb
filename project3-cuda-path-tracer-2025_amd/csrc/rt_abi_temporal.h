// rt_abi_temporal.h — the temporal stage's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_temporal_*, pt_denoise_temporal, pt_debug_temporal_times, and the history / base state
// machine of State::tp_*.  Calls: rt_core.h, denoise_ctx and g_dn_timing of rt_abi_denoise.h, the
// kernels of pt_temporal_kernels.h and k_atrous_*_var of pt_denoise_kernels.h.

// ---------------------------------------------------------------------------------------------
// temporal history for the denoiser (include/pt/pt_denoise_temporal.h)
// ---------------------------------------------------------------------------------------------
static int32_t temporal_event(int k) {
    if (!gp->tp_ev[k]) HIPCHK(hipEventCreate(&gp->tp_ev[k]));
    HIPCHK(hipEventRecord(gp->tp_ev[k], gp->stream));
    return PT_OK;
}

void pt_temporal_default_params(pt_temporal_params* t) {
    if (!t) return;
    t->max_history = 32;
    t->normal_cos_min = 0.9f;
    t->plane_tol = 0.02f;
    t->variance_history_min = 4;
    t->sigma_variance = 4.0f;
}

int32_t pt_temporal_reset(void) {
    RC(denoise_ctx("pt_temporal_reset"));
    gp->tp_history = false;
    gp->tp_base_valid = false;
    return PT_OK;
}

int32_t pt_denoise_temporal(const pt_denoise_params* params, const pt_temporal_params* tparams, int32_t samples,
                            pt_uchar4* pbo, float* host_out) {
    RC(denoise_ctx("pt_denoise_temporal"));
    if (gp->naive) return fail(PT_E_UNSUPPORTED, "pt_denoise_temporal: not available in naive mesh mode");
    pt_denoise_params p;
    if (params) p = *params;
    else pt_denoise_default_params(&p);
    pt_temporal_params t;
    if (tparams) t = *tparams;
    else pt_temporal_default_params(&t);
    if (p.levels < 1 || p.levels > PT_DENOISE_MAX_LEVELS)
        return fail(PT_E_INVALID, "pt_denoise_temporal: levels must be 1 .. %d, got %d", PT_DENOISE_MAX_LEVELS, p.levels);
    const float sig[5] = {p.sigma_color, p.sigma_normal, p.sigma_position, t.plane_tol, t.sigma_variance};
    const char* sig_name[5] = {"sigma_color", "sigma_normal", "sigma_position", "plane_tol", "sigma_variance"};
    for (int k = 0; k < 5; ++k)
        if (!(sig[k] > 0.0f) || !std::isfinite(sig[k]))
            return fail(PT_E_INVALID, "pt_denoise_temporal: %s must be positive and finite", sig_name[k]);
    if (samples < 1) return fail(PT_E_INVALID, "pt_denoise_temporal: samples must be >= 1, got %d", samples);
    if (t.max_history < 1) return fail(PT_E_INVALID, "pt_denoise_temporal: max_history must be >= 1, got %d", t.max_history);
    if (!(t.normal_cos_min >= -1.0f && t.normal_cos_min <= 1.0f))
        return fail(PT_E_INVALID, "pt_denoise_temporal: normal_cos_min must be in [-1, 1]");
    if (t.variance_history_min < 0)
        return fail(PT_E_INVALID, "pt_denoise_temporal: variance_history_min must be >= 0, got %d", t.variance_history_min);
    if (!gp->gbuf_valid)
        return fail(PT_E_STATE, "pt_denoise_temporal: no feature buffer captured for this camera (pt_gbuffer_capture)");
    if (gp->gbuf_through > 0)
        return fail(PT_E_UNSUPPORTED, "pt_denoise_temporal: the feature buffer is a through-capture (max_specular %d): "
                    "a position behind a reflection or refraction cannot be reprojected through the pinhole camera",
                    gp->gbuf_through);
    const int n = gp->pixels_total;
    if (!gp->d_tp[0]) {
        for (float4*& q : gp->d_gbuf[1]) RC(dalloc(&q, (size_t)n));
        for (float4*& q : gp->d_tp) RC(dalloc(&q, (size_t)n));
    }
    const int demod = p.demodulate_albedo != 0;
    if (gp->tp_history && gp->tp_demod != demod) {   // the history is in the other colour domain
        gp->tp_history = false;
        gp->tp_base_valid = false;
    }
    float4* const* cur = gp->d_gbuf[gp->gbuf_cur];
    float4 *bcol = gp->d_tp[0], *bmom = gp->d_tp[1], *col = gp->d_tp[2], *mom = gp->d_tp[3];
    const bool timing = g_dn_timing;
    const bool reproject = !gp->tp_base_valid;
    if (timing) RC(temporal_event(0));
    if (reproject) {
        // reads the history out of the integrated planes before k_temporal_integrate overwrites them
        float4* const* hs = gp->d_gbuf[gp->tp_history ? gp->tp_hist_set : gp->gbuf_cur];
        ReprojectArgs r{};
        r.cur = GBuf{cur[0], cur[1], cur[2]};
        r.hist = GBuf{hs[0], hs[1], hs[2]};
        r.hcol = col;
        r.hmom = mom;
        r.bcol = bcol;
        r.bmom = bmom;
        r.cam = gp->tp_cam;
        r.n = n;
        r.has_history = gp->tp_history;
        r.max_history = (float)t.max_history;
        r.normal_cos_min = t.normal_cos_min;
        r.plane_tol = t.plane_tol;
        hipLaunchKernelGGL(k_reproject, dim3(nblocks(n)), dim3(BLOCK), 0, gp->stream, r);
        HIPCHK(hipGetLastError());
        gp->tp_base_valid = true;
    }
    if (timing) RC(temporal_event(1));
    const dim3 grid((gp->width + AT_TILE - 1) / AT_TILE, (gp->height + AT_TILE - 1) / AT_TILE);
    IntegrateArgs ia{};
    ia.image = gp->d_image;
    ia.ga = cur[2];
    ia.bcol = bcol;
    ia.bmom = bmom;
    ia.col = col;
    ia.mom = mom;
    ia.W = gp->width;
    ia.H = gp->height;
    ia.demod = demod;
    ia.samples = (float)samples;
    ia.var_hist_min = (float)t.variance_history_min;
    hipLaunchKernelGGL(k_temporal_integrate, grid, dim3(BLOCK), 0, gp->stream, ia);
    HIPCHK(hipGetLastError());
    // the integrated planes are the history from here on, whatever happens to the levels below
    gp->tp_history = true;
    gp->tp_hist_set = gp->gbuf_cur;
    gp->tp_cam = gp->sc.cam;
    gp->tp_demod = demod;
    gp->tp_result = true;
    if (timing) RC(temporal_event(2));
    auto inv_sq = [](double s) { return (float)std::min(1.0 / (s * s), 3.0e38); };
    AtrousArgsVar a{};
    a.gn = cur[0];
    a.gx = cur[1];
    a.ga = cur[2];
    a.W = gp->width;
    a.H = gp->height;
    a.demod = demod;
    a.samples = (float)samples;
    a.k_normal = inv_sq(p.sigma_normal);
    a.k_position = inv_sq(p.sigma_position);
    a.mom = mom;
    float* out3 = nullptr;
    for (int l = 0; l < p.levels; ++l) {
        a.first = 0;   // the colour comes from the integrated plane, never from the image
        a.last = l == p.levels - 1;
        a.step = 1 << l;
        a.cin = l > 0 ? gp->d_dn_color[(l - 1) & 1] : col;
        a.cout = a.last ? nullptr : gp->d_dn_color[l & 1];
        a.out3 = out3 = a.last ? reinterpret_cast<float*>(gp->d_dn_color[l & 1]) : nullptr;
        a.pbo = a.last ? pbo : nullptr;
        const double sv = (double)t.sigma_variance * std::ldexp(1.0, -l);
        a.sv2 = (float)std::max(sv * sv, 1.0e-30);
        if (l == 0) hipLaunchKernelGGL(k_atrous_lds_var<1>, grid, dim3(BLOCK), 0, gp->stream, a);
        else if (l == 1) hipLaunchKernelGGL(k_atrous_lds_var<2>, grid, dim3(BLOCK), 0, gp->stream, a);
        else hipLaunchKernelGGL(k_atrous_direct_var, grid, dim3(BLOCK), 0, gp->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (timing) RC(temporal_event(3));
    if (host_out)
        HIPCHK(hipMemcpyAsync(host_out, out3, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, gp->stream));
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (timing) {
        for (int k = 0; k < 3; ++k) HIPCHK(hipEventElapsedTime(&gp->tp_ms[k], gp->tp_ev[k], gp->tp_ev[k + 1]));
        if (!reproject) gp->tp_ms[0] = 0.f;
    }
    return PT_OK;
}

int32_t pt_temporal_get(float* base_color, float* base_moments, float* color, float* moments, int64_t n_pixels) {
    RC(denoise_ctx("pt_temporal_get"));
    if (!gp->tp_result) return fail(PT_E_STATE, "pt_temporal_get: pt_denoise_temporal has not run");
    if (n_pixels < gp->pixels_total) return fail(PT_E_INVALID, "pt_temporal_get: room for %lld pixels, the image has %d",
                                                 (long long)n_pixels, gp->pixels_total);
    float* dst[4] = {base_color, base_moments, color, moments};
    for (int k = 0; k < 4; ++k)
        if (dst[k]) HIPCHK(smemcpy(dst[k], gp->d_tp[k], sizeof(float4) * (size_t)gp->pixels_total, hipMemcpyDeviceToHost));
    return PT_OK;
}

int32_t pt_debug_temporal_times(float* reproject_ms, float* integrate_ms, float* levels_ms) {
    RC(need_init());
    if (reproject_ms) *reproject_ms = gp->tp_ms[0];
    if (integrate_ms) *integrate_ms = gp->tp_ms[1];
    if (levels_ms) *levels_ms = gp->tp_ms[2];
    return PT_OK;
}

