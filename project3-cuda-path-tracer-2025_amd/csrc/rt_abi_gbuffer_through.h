// rt_abi_gbuffer_through.h — the through-capture's entry points (inside pt_runtime.hip's extern "C" block).
// Owns: pt_gbuffer_capture_through, pt_gbuffer_get_chain, DenoiseState's d_chain_* and gbuf_through.
// Calls: rt_core.h, with_traversal of rt_pass.h, denoise_ctx / denoise_event / copy_planes of
// rt_denoise.h, capture_begin / capture_end of rt_abi_denoise.h (whose planes and validity flag a
// through-capture fills like pt_gbuffer_capture), the kernels of pt_gbuffer_through_kernels.h.

// ---------------------------------------------------------------------------------------------
// first non-specular hit (include/pt/pt_gbuffer_through.h): a seeding launch + one launch per round
// ---------------------------------------------------------------------------------------------
// round k's output queue: ping-pong buffers, a counter line per round
static ChainQueue chain_queue(int k) {
    float4* q = gp->dn.d_chain_q[k & 1];
    return ChainQueue{q, q + gp->pixels_total, gp->dn.d_chain_cnt + k * CNT_PAD};
}

int32_t pt_gbuffer_capture_through(int32_t iteration, int32_t max_specular) {
    RC(denoise_ctx("pt_gbuffer_capture_through"));
    if (max_specular < 0 || max_specular > PT_GBUFFER_THROUGH_MAX)
        return fail(PT_E_INVALID, "pt_gbuffer_capture_through: max_specular must be 0 .. %d, got %d",
                    PT_GBUFFER_THROUGH_MAX, max_specular);
    GBuf g;
    RC(capture_begin("pt_gbuffer_capture_through", iteration, &g));
    DenoiseState& dn = gp->dn;
    const int n = gp->pixels_total;
    if (!dn.d_chain_cnt) {
        for (float4*& q : dn.d_chain_q) RC(dalloc(&q, 2 * (size_t)n));   // origin | pixel, then direction | t_sum
        RC(dalloc(&dn.d_chain_followed, (size_t)n));
        RC(dalloc(&dn.d_chain_cnt, (size_t)(PT_GBUFFER_THROUGH_MAX + 1) * CNT_PAD));
    }
    if (g_dn_timing) RC(denoise_event(dn.ev, 0));
    const dim3 grid(nblocks(n));   // every launch: the worst case, one thread per pixel
    hipLaunchKernelGGL(k_chain_reset, dim3(1), dim3(64), 0, gp->stream, dn.d_chain_cnt, PT_GBUFFER_THROUGH_MAX + 1);
    ChainArgs c{ChainQueue{}, chain_queue(0), dn.d_chain_followed, n};
    // the traversal pt_gbuffer_capture runs for this context's options
    with_traversal([&](auto bvh, auto fast) {
        hipLaunchKernelGGL((k_gbuffer_seed<bvh.value, fast.value>), grid, dim3(BLOCK), traversal_lds(), gp->stream, gp->sc, g,
                           c, iteration, n, max_specular);
        for (int k = 1; k <= max_specular; ++k) {
            c.in = chain_queue(k - 1);
            c.out = chain_queue(k);
            hipLaunchKernelGGL((k_gbuffer_follow<bvh.value, fast.value>), grid, dim3(BLOCK), traversal_lds(), gp->stream,
                               gp->sc, g, c, k, max_specular);
        }
    });
    RC(capture_end());
    dn.gbuf_through = max_specular;
    return PT_OK;
}

int32_t pt_gbuffer_get_chain(int32_t* followed, int64_t n_pixels) {
    RC(denoise_ctx("pt_gbuffer_get_chain"));
    if (!gp->dn.gbuf_valid || gp->dn.gbuf_through < 0)
        return fail(PT_E_STATE, "pt_gbuffer_get_chain: no through-capture for this camera (pt_gbuffer_capture_through)");
    return copy_planes("pt_gbuffer_get_chain", n_pixels, 1, &followed, &gp->dn.d_chain_followed);
}

