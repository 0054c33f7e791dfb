// rt_abi_regress.h — the feature regression's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_regress_*, pt_denoise_regress, pt_debug_regress_times and DenoiseState's rg_* / d_rg_tab.
// Calls: rt_core.h, the checks, denoise_event and result_out of rt_denoise.h, and the kernels of
// pt_regress_kernels.h.

// ---------------------------------------------------------------------------------------------
// blockwise feature regression (include/pt/pt_denoise_regress.h)
// ---------------------------------------------------------------------------------------------
static_assert(RG_BLOCK_FLOATS == PT_REGRESS_BLOCK_FLOATS, "block record");

static int regress_blocks_x() { return (gp->width + RG_STRIDE - 1) / RG_STRIDE + 1; }
static int regress_blocks_y() { return (gp->height + RG_STRIDE - 1) / RG_STRIDE + 1; }

void pt_regress_default_params(pt_regress_params* p) {
    if (!p) return;
    p->ridge = 1e-3f;
    p->demodulate_albedo = 1;
}

int32_t pt_denoise_regress(const pt_regress_params* params, int32_t samples, pt_uchar4* pbo, float* host_out) {
    RC(denoise_ctx("pt_denoise_regress"));
    if (gp->naive) return fail(PT_E_UNSUPPORTED, "pt_denoise_regress: not available in naive mesh mode");
    pt_regress_params p;
    if (params) p = *params;
    else pt_regress_default_params(&p);
    RC(check_positive("pt_denoise_regress", "ridge", p.ridge));
    RC(check_samples("pt_denoise_regress", samples));
    RC(check_captured("pt_denoise_regress"));
    DenoiseState& dn = gp->dn;
    const int nbx = regress_blocks_x(), nby = regress_blocks_y();
    if (!dn.d_rg_tab) RC(dalloc(&dn.d_rg_tab, (size_t)nbx * nby * RG_REC));
    RegressArgs a{};
    a.image = gp->d_image;
    a.gn = dn.d_gbuf[dn.gbuf_cur][0];
    a.gx = dn.d_gbuf[dn.gbuf_cur][1];
    a.ga = dn.d_gbuf[dn.gbuf_cur][2];
    a.mats = gp->d_mats;
    a.tab = dn.d_rg_tab;
    a.out3 = reinterpret_cast<float*>(dn.d_color[0]);   // float3 per pixel in a float4 plane
    a.pbo = pbo;
    a.W = gp->width;
    a.H = gp->height;
    a.nbx = nbx;
    a.num_mats = gp->sc.num_mats;
    a.demod = p.demodulate_albedo != 0;
    a.samples = (float)samples;
    a.ridge = p.ridge;
    const bool timing = g_dn_timing;
    if (timing) RC(denoise_event(dn.rg_ev, 0));
    hipLaunchKernelGGL(k_regress_fit, dim3(nbx, nby), dim3(BLOCK), 0, gp->stream, a);
    HIPCHK(hipGetLastError());
    if (timing) RC(denoise_event(dn.rg_ev, 1));
    hipLaunchKernelGGL(k_regress_apply, dim3(nbx - 1, nby - 1), dim3(BLOCK), 0, gp->stream, a);
    HIPCHK(hipGetLastError());
    if (timing) RC(denoise_event(dn.rg_ev, 2));
    dn.rg_result = true;
    RC(result_out(host_out, a.out3));
    if (timing)
        for (int k = 0; k < 2; ++k) HIPCHK(hipEventElapsedTime(&dn.rg_ms[k], dn.rg_ev[k], dn.rg_ev[k + 1]));
    return PT_OK;
}

int32_t pt_regress_get(float* blocks, int64_t n_blocks) {
    RC(denoise_ctx("pt_regress_get"));
    if (!gp->dn.rg_result) return fail(PT_E_STATE, "pt_regress_get: pt_denoise_regress has not run");
    const int64_t nb = (int64_t)regress_blocks_x() * regress_blocks_y();
    if (!blocks || n_blocks < nb)
        return fail(PT_E_INVALID, "pt_regress_get: room for %lld blocks, the image has %lld", (long long)n_blocks, (long long)nb);
    std::vector<float> tab((size_t)nb * RG_REC);   // the records are RG_REC floats apart on the device
    HIPCHK(smemcpy(tab.data(), gp->dn.d_rg_tab, sizeof(float) * tab.size(), hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < nb; ++b) memcpy(blocks + b * RG_BLOCK_FLOATS, &tab[(size_t)b * RG_REC], sizeof(float) * RG_BLOCK_FLOATS);
    return PT_OK;
}

int32_t pt_debug_regress_times(float* fit_ms, float* apply_ms) {
    RC(need_init());
    if (fit_ms) *fit_ms = gp->dn.rg_ms[0];
    if (apply_ms) *apply_ms = gp->dn.rg_ms[1];
    return PT_OK;
}

