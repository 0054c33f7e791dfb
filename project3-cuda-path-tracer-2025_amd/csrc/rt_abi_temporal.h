// rt_abi_temporal.h — the temporal stage's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_temporal_*, pt_denoise_temporal, pt_debug_temporal_times, and the history / base state
// machine of DenoiseState::tp_*.  Calls: rt_core.h, the checks, denoise_event, copy_planes, result_out
// and atrous_levels (the variance-guided levels) of rt_denoise.h, the kernels of pt_temporal_kernels.h.

// ---------------------------------------------------------------------------------------------
// temporal history for the denoiser (include/pt/pt_denoise_temporal.h)
// ---------------------------------------------------------------------------------------------
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
    gp->dn.tp_history = false;
    gp->dn.tp_base_valid = false;
    return PT_OK;
}

int32_t pt_denoise_temporal(const pt_denoise_params* params, const pt_temporal_params* tparams, int32_t samples,
                            pt_uchar4* pbo, float* host_out) {
    const char* const what = "pt_denoise_temporal";
    RC(denoise_ctx(what));
    if (gp->naive) return fail(PT_E_UNSUPPORTED, "pt_denoise_temporal: not available in naive mesh mode");
    pt_denoise_params p;
    if (params) p = *params;
    else pt_denoise_default_params(&p);
    pt_temporal_params t;
    if (tparams) t = *tparams;
    else pt_temporal_default_params(&t);
    RC(check_params(what, p));
    RC(check_positive(what, "plane_tol", t.plane_tol));
    RC(check_positive(what, "sigma_variance", t.sigma_variance));
    RC(check_samples(what, samples));
    if (t.max_history < 1) return fail(PT_E_INVALID, "pt_denoise_temporal: max_history must be >= 1, got %d", t.max_history);
    if (!(t.normal_cos_min >= -1.0f && t.normal_cos_min <= 1.0f))
        return fail(PT_E_INVALID, "pt_denoise_temporal: normal_cos_min must be in [-1, 1]");
    if (t.variance_history_min < 0)
        return fail(PT_E_INVALID, "pt_denoise_temporal: variance_history_min must be >= 0, got %d", t.variance_history_min);
    RC(check_captured(what));
    DenoiseState& dn = gp->dn;
    if (dn.gbuf_through > 0)
        return fail(PT_E_UNSUPPORTED, "pt_denoise_temporal: the feature buffer is a through-capture (max_specular %d): "
                    "a position behind a reflection or refraction cannot be reprojected through the pinhole camera",
                    dn.gbuf_through);
    const int n = gp->pixels_total;
    if (!dn.d_tp[0]) {
        for (float4*& q : dn.d_gbuf[1]) RC(dalloc(&q, (size_t)n));
        for (float4*& q : dn.d_tp) RC(dalloc(&q, (size_t)n));
    }
    const int demod = p.demodulate_albedo != 0;
    if (dn.tp_history && dn.tp_demod != demod) {   // the history is in the other colour domain
        dn.tp_history = false;
        dn.tp_base_valid = false;
    }
    float4* const* cur = dn.d_gbuf[dn.gbuf_cur];
    float4 *bcol = dn.d_tp[0], *bmom = dn.d_tp[1], *col = dn.d_tp[2], *mom = dn.d_tp[3];
    const bool timing = g_dn_timing;
    const bool reproject = !dn.tp_base_valid;
    if (timing) RC(denoise_event(dn.tp_ev, 0));
    if (reproject) {
        // reads the history out of the integrated planes before k_temporal_integrate overwrites them
        float4* const* hs = dn.d_gbuf[dn.tp_history ? dn.tp_hist_set : dn.gbuf_cur];
        ReprojectArgs r{};
        r.cur = GBuf{cur[0], cur[1], cur[2]};
        r.hist = GBuf{hs[0], hs[1], hs[2]};
        r.hcol = col;
        r.hmom = mom;
        r.bcol = bcol;
        r.bmom = bmom;
        r.cam = dn.tp_cam;
        r.n = n;
        r.has_history = dn.tp_history;
        r.max_history = (float)t.max_history;
        r.normal_cos_min = t.normal_cos_min;
        r.plane_tol = t.plane_tol;
        hipLaunchKernelGGL(k_reproject, dim3(nblocks(n)), dim3(BLOCK), 0, gp->stream, r);
        HIPCHK(hipGetLastError());
        dn.tp_base_valid = true;
    }
    if (timing) RC(denoise_event(dn.tp_ev, 1));
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
    dn.tp_history = true;
    dn.tp_hist_set = dn.gbuf_cur;
    dn.tp_cam = gp->sc.cam;
    dn.tp_demod = demod;
    dn.tp_result = true;
    if (timing) RC(denoise_event(dn.tp_ev, 2));
    AtrousArgsVar a{};
    atrous_common(a, p, samples);
    a.mom = mom;
    float* out3 = nullptr;
    // the colour comes from the integrated plane, never from the image
    RC(atrous_levels(a, col, p.levels, pbo, [&](AtrousArgsVar& lv, int l) {
        const double sv = (double)t.sigma_variance * std::ldexp(1.0, -l);
        lv.sv2 = (float)std::max(sv * sv, 1.0e-30);
        return PT_OK;
    }, &out3));
    if (timing) RC(denoise_event(dn.tp_ev, 3));
    RC(result_out(host_out, out3));
    if (timing) {
        for (int k = 0; k < 3; ++k) HIPCHK(hipEventElapsedTime(&dn.tp_ms[k], dn.tp_ev[k], dn.tp_ev[k + 1]));
        if (!reproject) dn.tp_ms[0] = 0.f;
    }
    return PT_OK;
}

int32_t pt_temporal_get(float* base_color, float* base_moments, float* color, float* moments, int64_t n_pixels) {
    RC(denoise_ctx("pt_temporal_get"));
    if (!gp->dn.tp_result) return fail(PT_E_STATE, "pt_temporal_get: pt_denoise_temporal has not run");
    float* dst[4] = {base_color, base_moments, color, moments};
    return copy_planes("pt_temporal_get", n_pixels, 4, dst, gp->dn.d_tp);
}

int32_t pt_debug_temporal_times(float* reproject_ms, float* integrate_ms, float* levels_ms) {
    RC(need_init());
    if (reproject_ms) *reproject_ms = gp->dn.tp_ms[0];
    if (integrate_ms) *integrate_ms = gp->dn.tp_ms[1];
    if (levels_ms) *levels_ms = gp->dn.tp_ms[2];
    return PT_OK;
}

