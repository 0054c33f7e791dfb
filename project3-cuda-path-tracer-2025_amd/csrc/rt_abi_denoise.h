// rt_abi_denoise.h — the denoiser's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_gbuffer_* (and which of the two plane sets a capture writes), pt_denoise*, pt_debug_denoise_*.
// Calls: rt_core.h (State::dn), with_traversal of rt_pass.h, the checks, copy_planes, result_out and
// atrous_levels of rt_denoise.h, and the kernels of pt_denoise_kernels.h.

// ---------------------------------------------------------------------------------------------
// denoiser (include/pt/pt_denoise.h): first-hit feature planes + the a-trous filter
// ---------------------------------------------------------------------------------------------
void pt_denoise_default_params(pt_denoise_params* p) {
    if (!p) return;
    p->levels = 5;
    p->sigma_color = 0.45f;
    p->sigma_normal = 0.35f;
    p->sigma_position = 0.20f;
    p->demodulate_albedo = 1;
}

// the start of a capture (this file's and rt_abi_gbuffer_through.h's): the context and iteration
// checks, the planes allocated, the captured buffer invalid until the capture completes; g: the
// plane set to write
static int32_t capture_begin(const char* what, int32_t iteration, GBuf* g) {
    RC(denoise_ctx(what));
    if (gp->naive) return fail(PT_E_UNSUPPORTED, "%s: not available in naive mesh mode", what);
    if (iteration <= 0) return fail(PT_E_INVALID, "iteration is 1-based, got %d", iteration);
    DenoiseState& dn = gp->dn;
    const int n = gp->pixels_total;
    dn.gbuf_valid = false;
    dn.gbuf_through = -1;
    if (!dn.d_gbuf[0][0]) {
        for (float4*& p : dn.d_gbuf[0]) RC(dalloc(&p, (size_t)n));
        for (float4*& p : dn.d_color) RC(dalloc(&p, (size_t)n));
    }
    // the temporal history (rt_abi_temporal.h) keeps the planes of its capture: write the other set
    if (dn.tp_history && dn.tp_hist_set == dn.gbuf_cur) dn.gbuf_cur ^= 1;
    dn.tp_base_valid = false;
    float4* const* cur = dn.d_gbuf[dn.gbuf_cur];
    *g = GBuf{cur[0], cur[1], cur[2]};
    return PT_OK;
}
// ... and its end, after the capture's last launch (event 0 went before its first): the wait, the
// capture's time, the buffer valid
static int32_t capture_end() {
    HIPCHK(hipGetLastError());
    if (g_dn_timing) RC(denoise_event(gp->dn.ev, 1));
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (g_dn_timing) HIPCHK(hipEventElapsedTime(&gp->dn.capture_ms, gp->dn.ev[0], gp->dn.ev[1]));
    gp->dn.gbuf_valid = true;
    return PT_OK;
}

int32_t pt_gbuffer_capture(int32_t iteration) {
    GBuf g;
    RC(capture_begin("pt_gbuffer_capture", iteration, &g));
    const int n = gp->pixels_total;
    if (g_dn_timing) RC(denoise_event(gp->dn.ev, 0));
    // the traversal pt_test_intersect (and the staged pipeline) runs for this context's options
    with_traversal([&](auto bvh, auto fast) {
        hipLaunchKernelGGL((k_gbuffer<bvh.value, fast.value>), dim3(nblocks(n)), dim3(BLOCK), traversal_lds(), gp->stream,
                           gp->sc, g, iteration, n);
    });
    return capture_end();
}

int32_t pt_gbuffer_get(float* normal_t, float* position, float* albedo_mat, int64_t n_pixels) {
    RC(denoise_ctx("pt_gbuffer_get"));
    if (!gp->dn.gbuf_valid) return fail(PT_E_STATE, "pt_gbuffer_get: no feature buffer captured for this camera");
    float* dst[3] = {normal_t, position, albedo_mat};
    return copy_planes("pt_gbuffer_get", n_pixels, 3, dst, gp->dn.d_gbuf[gp->dn.gbuf_cur]);
}

int32_t pt_denoise(const pt_denoise_params* params, int32_t samples, pt_uchar4* pbo, float* host_out) {
    RC(denoise_ctx("pt_denoise"));
    pt_denoise_params p;
    if (params) p = *params;
    else pt_denoise_default_params(&p);
    RC(check_params("pt_denoise", p));
    RC(check_samples("pt_denoise", samples));
    RC(check_captured("pt_denoise"));
    DenoiseState& dn = gp->dn;
    AtrousArgs a{};
    a.image = gp->d_image;
    atrous_common(a, p, samples);
    float* out3 = nullptr;
    RC(atrous_levels(a, nullptr, p.levels, pbo, [&](AtrousArgs& lv, int l) {
        lv.k_color = inv_sq((double)p.sigma_color * std::ldexp(1.0, -l));
        return g_dn_timing ? denoise_event(dn.ev, 2 + l) : (int32_t)PT_OK;
    }, &out3));
    if (g_dn_timing) RC(denoise_event(dn.ev, 2 + p.levels));
    RC(result_out(host_out, out3));
    if (g_dn_timing) {
        HIPCHK(hipEventElapsedTime(&dn.ms, dn.ev[2], dn.ev[2 + p.levels]));
        for (int l = 0; l < PT_DENOISE_MAX_LEVELS; ++l) {
            dn.level_ms[l] = 0.f;
            if (l < p.levels) HIPCHK(hipEventElapsedTime(&dn.level_ms[l], dn.ev[2 + l], dn.ev[3 + l]));
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
    if (capture_ms) *capture_ms = gp->dn.capture_ms;
    if (denoise_ms) *denoise_ms = gp->dn.ms;
    if (level_ms) memcpy(level_ms, gp->dn.level_ms, sizeof gp->dn.level_ms);
    return PT_OK;
}

