// rt_abi_gbuffer_through.h — the through-capture's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_gbuffer_capture_through, pt_gbuffer_get_chain, State::d_chain_* and State::gbuf_through.
// Calls: rt_core.h, denoise_ctx / denoise_event / g_dn_timing of rt_abi_denoise.h (whose planes and
// validity flag a through-capture fills like pt_gbuffer_capture), the kernels of
// pt_gbuffer_through_kernels.h.

// ---------------------------------------------------------------------------------------------
// first non-specular hit (include/pt/pt_gbuffer_through.h): a seeding launch + one launch per round
// ---------------------------------------------------------------------------------------------
// round k's output queue: ping-pong buffers, a counter line per round
static ChainQueue chain_queue(int k) {
    float4* q = gp->d_chain_q[k & 1];
    return ChainQueue{q, q + gp->pixels_total, gp->d_chain_cnt + k * CNT_PAD};
}
// the traversal pt_gbuffer_capture runs for this context's options
#define CHAIN_LAUNCH(kernel, ...)                                                                                       \
    do {                                                                                                                \
        if (gp->has_bvh && (gp->opts.variant & VAR_BVH_FAST))                                                           \
            hipLaunchKernelGGL((kernel<true, true>), grid, dim3(BLOCK), gp->bvh_lds, gp->stream, gp->sc, g, __VA_ARGS__); \
        else if (gp->has_bvh)                                                                                           \
            hipLaunchKernelGGL((kernel<true, false>), grid, dim3(BLOCK), gp->bvh_lds, gp->stream, gp->sc, g, __VA_ARGS__); \
        else                                                                                                            \
            hipLaunchKernelGGL((kernel<false, false>), grid, dim3(BLOCK), 0, gp->stream, gp->sc, g, __VA_ARGS__);       \
    } while (0)

int32_t pt_gbuffer_capture_through(int32_t iteration, int32_t max_specular) {
    RC(denoise_ctx("pt_gbuffer_capture_through"));
    if (max_specular < 0 || max_specular > PT_GBUFFER_THROUGH_MAX)
        return fail(PT_E_INVALID, "pt_gbuffer_capture_through: max_specular must be 0 .. %d, got %d",
                    PT_GBUFFER_THROUGH_MAX, max_specular);
    GBuf g;
    RC(capture_begin("pt_gbuffer_capture_through", iteration, &g));
    const int n = gp->pixels_total;
    if (!gp->d_chain_cnt) {
        for (float4*& q : gp->d_chain_q) RC(dalloc(&q, 2 * (size_t)n));   // origin | pixel, then direction | t_sum
        RC(dalloc(&gp->d_chain_followed, (size_t)n));
        RC(dalloc(&gp->d_chain_cnt, (size_t)(PT_GBUFFER_THROUGH_MAX + 1) * CNT_PAD));
    }
    if (g_dn_timing) RC(denoise_event(0));
    const dim3 grid(nblocks(n));   // every launch: the worst case, one thread per pixel
    hipLaunchKernelGGL(k_chain_reset, dim3(1), dim3(64), 0, gp->stream, gp->d_chain_cnt, PT_GBUFFER_THROUGH_MAX + 1);
    ChainArgs c{ChainQueue{}, chain_queue(0), gp->d_chain_followed, n};
    CHAIN_LAUNCH(k_gbuffer_seed, c, iteration, n, max_specular);
    for (int k = 1; k <= max_specular; ++k) {
        c.in = chain_queue(k - 1);
        c.out = chain_queue(k);
        CHAIN_LAUNCH(k_gbuffer_follow, c, k, max_specular);
    }
    HIPCHK(hipGetLastError());
    if (g_dn_timing) RC(denoise_event(1));
    HIPCHK(hipStreamSynchronize(gp->stream));
    if (g_dn_timing) HIPCHK(hipEventElapsedTime(&gp->dn_capture_ms, gp->dn_ev[0], gp->dn_ev[1]));
    gp->gbuf_valid = true;
    gp->gbuf_through = max_specular;
    return PT_OK;
}

int32_t pt_gbuffer_get_chain(int32_t* followed, int64_t n_pixels) {
    RC(denoise_ctx("pt_gbuffer_get_chain"));
    if (!gp->gbuf_valid || gp->gbuf_through < 0)
        return fail(PT_E_STATE, "pt_gbuffer_get_chain: no through-capture for this camera (pt_gbuffer_capture_through)");
    if (n_pixels < gp->pixels_total) return fail(PT_E_INVALID, "pt_gbuffer_get_chain: room for %lld pixels, the image has %d",
                                                 (long long)n_pixels, gp->pixels_total);
    if (followed)
        HIPCHK(smemcpy(followed, gp->d_chain_followed, sizeof(int32_t) * (size_t)gp->pixels_total, hipMemcpyDeviceToHost));
    return PT_OK;
}

#undef CHAIN_LAUNCH

