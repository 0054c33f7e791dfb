// rt_spec.h — single-frame speculation: the next frame traced while this one's image is copied out.
//
// Owns: SpecTask / SpecJob and the launcher thread (an instance of host/worker.h), every spec_*
// function, release_graph (the speculative graph goes with the pass graphs), need_single.
// Calls: rt_core.h, rt_pass.h (enqueue_pass, release_pass_graphs), rt_multi.h (the shards of the
// calling context: nshards, shard_ctx, ShardScope).

// ---- single-frame speculation -----------------------------------------------------------------
// main.cpp calls pathtrace(pbo, frame, ++iteration) every frame and copies the 7.68 MB image to
// pageable host memory each time (pathtrace.cu:783): on MI355X that copy (~0.15 ms over PCIe) is
// longer than the frame's kernels (~0.12 ms).  So once frame N is traced, frame N + 1 is traced
// at once on a second stream -- into a plane of its own with a FrameCtl of its own, the accumulated
// image untouched -- while frame N's image is copied out.  At its end the frame forms image +
// plane into a sum buffer (k_spec_sum: the same additions as the frame's own gathers); the call for
// iteration N + 1 then copies that sum out while k_adopt_frame makes it the image and takes over
// the frame's counters, bit for bit what tracing it then would have produced.
// Any call that could make it differ (another iteration, a camera or depth change, multi-frame
// passes, the test and profiling entry points) first waits for it and drops it (spec_cancel).
// Only calls that copy the image out start one.  PT_SPECULATE=0 turns it off.  One device
// context, fused pipeline.
// The speculative frame is queued by a launcher thread: the copy into the caller's pageable memory
// holds the calling thread for its whole ~0.14 ms, so the frame must be queued before it -- and
// queueing it on the calling thread (event wait + graph launch, ~20 us of host time) delayed the
// copy by as much.  The caller records spec_ev_in, hands the launcher {stream, graph, events,
// iteration preset} and goes straight on to the copy; everything that later touches the speculative
// stream, its events or its graph waits for the launcher first (spec_worker_idle).
// One launch: {device, stream, events, graph, iteration preset, k_spec_sum's buffers}.  A call of a
// context of several devices posts one per shard together; the launcher queues them in order.
struct SpecTask {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_done = nullptr;
    hipGraphExec_t exec = nullptr;
    int* iter_ptr = nullptr;
    int preset = -1;                 // < 0: the iteration is already right
    const float* image = nullptr;    // k_spec_sum: image + plane -> sum
    const float* plane = nullptr;
    float* sum = nullptr;
    int nf = 0;
};
// Threading: the launcher thread only ever touches the HIP objects of the tasks handed to it (by
// value) and its own current device (hipSetDevice is per host thread); it never reads the
// runtime's process-global context (gp, M) nor calls RCCL.  The caller waits for it (wait) before
// it touches a posted task's stream, events or graph again.
// One job: a call's tasks, queued in order up to the first error.  The launcher keeps an error
// until one wait() has read it (pth::Worker, sticky).
struct SpecJob {
    SpecTask tasks[PT_MAX_DEVICES];
    int n = 0;

    static hipError_t launch_one(const SpecTask& t) {
        hipError_t e = hipSetDevice(t.device);
        if (e == hipSuccess) e = hipStreamWaitEvent(t.stream, t.ev_in, 0);
        if (e == hipSuccess && t.preset >= 0) e = hipMemsetD32Async((hipDeviceptr_t)t.iter_ptr, t.preset, 1, t.stream);
        if (e == hipSuccess) e = hipGraphLaunch(t.exec, t.stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_spec_sum, dim3(nblocks((t.nf + 3) / 4)), dim3(BLOCK), 0, t.stream, t.image, t.plane,
                               t.sum, t.nf);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(t.ev_done, t.stream);
        return e;
    }
    hipError_t run() const {
        hipError_t e = hipSuccess;
        for (int i = 0; i < n && e == hipSuccess; ++i) e = launch_one(tasks[i]);
        return e;
    }
};
pth::Worker<SpecJob, hipError_t, true> g_spec_launcher;   // joined by spec_release, or idle at process exit

// wait until the posted launches are queued; their error, once
int spec_worker_idle() {
    HIPCHK(g_spec_launcher.wait());
    return PT_OK;
}

// every captured graph of the context: the speculative frame's and the passes'
void release_graph() {
    if (gp->spec_exec) {   // the launcher may still be queueing it, the stream still running it
        (void)spec_worker_idle();
        (void)hipStreamSynchronize(gp->spec_stream);
        (void)hipGraphExecDestroy(gp->spec_exec);
    }
    if (gp->spec_graph) (void)hipGraphDestroy(gp->spec_graph);
    gp->spec_exec = nullptr;
    gp->spec_graph = nullptr;
    release_pass_graphs();
}

// the calling context (g_primary): one device context, or the shards of a multi-device one (each
// speculates its own pixels); not a pixel shard of a one-process-per-GPU job (its caller combines)
bool spec_enabled() {
    return g_primary.tune.speculate && gp == &g_primary && gp->opts.pipeline == PT_PIPELINE_FUSED &&
           (gp->multi || gp->sc.shard.mode != PT_SHARD_PIXELS);
}
int spec_cancel() {
    if (gp->spec_iter == 0) return PT_OK;
    // the stream is drained even when the launcher reports an error: the launch may have failed
    // after the graph was queued (k_spec_sum, the event), and the graph uses the pass buffers the
    // caller's next work on gp->stream overwrites.  spec_iter is cleared once it is drained.
    const hipError_t le = g_spec_launcher.wait();
    const hipError_t se = hipStreamSynchronize(gp->spec_stream);
    gp->spec_iter = 0;
    HIPCHK(le);
    HIPCHK(se);
    return PT_OK;
}
void spec_release() {
    (void)g_spec_launcher.wait();
    if (gp == &g_primary) g_spec_launcher.join();
    if (gp->spec_stream) (void)hipStreamSynchronize(gp->spec_stream);
    // the speculated frame's graph goes with its stream (release_graph would otherwise sync a
    // stream that no longer exists before destroying it)
    if (gp->spec_exec) (void)hipGraphExecDestroy(gp->spec_exec);
    if (gp->spec_graph) (void)hipGraphDestroy(gp->spec_graph);
    gp->spec_exec = nullptr;
    gp->spec_graph = nullptr;
    if (gp->spec_ev_in) (void)hipEventDestroy(gp->spec_ev_in);
    if (gp->spec_ev_done) (void)hipEventDestroy(gp->spec_ev_done);
    if (gp->spec_stream) (void)hipStreamDestroy(gp->spec_stream);
    if (gp->d_ctl_spec) (void)hipFree(gp->d_ctl_spec);
    if (gp->d_spec_plane) (void)hipFree(gp->d_spec_plane);
    for (float*& p : gp->d_spec_sum)
        if (p) (void)hipFree(p), p = nullptr;
    if (gp->copy_stream) (void)hipStreamSynchronize(gp->copy_stream), (void)hipStreamDestroy(gp->copy_stream);
    gp->copy_stream = nullptr;
    gp->spec_stream = nullptr;
    gp->spec_ev_in = gp->spec_ev_done = nullptr;
    gp->d_ctl_spec = nullptr;
    gp->d_spec_plane = nullptr;
    gp->spec_iter = 0;
    gp->spec_dev_iter = 0;
}
// Until the scope ends, the current context's passes go to its speculative stream, counters and
// plane (enqueue_pass reads gp->stream, gp->d_ctl and gp->sc.contrib); restored on every exit path.
struct SpecTarget {
    hipStream_t stream = gp->stream;
    FrameCtl* ctl = gp->d_ctl;
    float* contrib = gp->sc.contrib;
    SpecTarget() {
        gp->stream = gp->spec_stream;
        gp->d_ctl = gp->d_ctl_spec;
        gp->sc.contrib = gp->d_spec_plane;
    }
    ~SpecTarget() {
        gp->stream = stream;
        gp->d_ctl = ctl;
        gp->sc.contrib = contrib;
    }
};
// frame `iter` of the current context on its speculation stream, behind everything queued on
// gp->stream so far: the launch is described in `t` (posted by the caller, with the other shards')
int spec_prepare(int iter, SpecTask& t) {
    if (!gp->spec_stream) {
        HIPCHK(hipStreamCreateWithFlags(&gp->spec_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&gp->spec_ev_in, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&gp->spec_ev_done, hipEventDisableTiming));
        HIPCHK(hipMalloc((void**)&gp->d_ctl_spec, sizeof(FrameCtl)));
        HIPCHK(hipMemsetAsync(gp->d_ctl_spec, 0, sizeof(FrameCtl), gp->spec_stream));
        HIPCHK(hipMalloc((void**)&gp->d_spec_plane, sizeof(float) * 3 * (size_t)gp->pixels_total));
        for (float*& p : gp->d_spec_sum) HIPCHK(hipMalloc((void**)&p, sizeof(float) * 3 * (size_t)gp->pixels_total));
        HIPCHK(hipStreamCreateWithFlags(&gp->copy_stream, hipStreamNonBlocking));
    }
    if (!gp->spec_exec) {   // captured once (released with the pass graphs: camera, depth, buffers)
        hipGraph_t gr = nullptr;
        {
            SpecTarget target;
            HIPCHK(hipStreamBeginCapture(gp->spec_stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue_pass(0, 1, 1);   // iteration: the device's + 1
            const hipError_t e = hipStreamEndCapture(gp->spec_stream, &gr);   // also after a failed enqueue
            RC(rc);
            HIPCHK(e);
        }
        gp->spec_graph = gr;
        HIPCHK(hipGraphInstantiate(&gp->spec_exec, gr, nullptr, nullptr, 0));
    }
    // behind gp->stream's work so far, as ONE graph launch queued by the launcher thread, so that
    // the image copy the caller queues next starts at once.  The captured k_frame_begin advances the
    // speculative FrameCtl's iteration by one: it is preset only when the last speculative frame was
    // not iter - 1 (consecutive calls launch the graph alone)
    HIPCHK(hipEventRecord(gp->spec_ev_in, gp->stream));
    gp->spec_sum_idx ^= 1;   // the other buffer: the one the caller may still be copying from is kept
    t.device = gp->device;
    t.stream = gp->spec_stream;
    t.ev_in = gp->spec_ev_in;
    t.ev_done = gp->spec_ev_done;
    t.exec = gp->spec_exec;
    t.iter_ptr = &gp->d_ctl_spec->iter;
    t.preset = gp->spec_dev_iter != iter - 1 ? iter - 1 : -1;
    t.image = gp->d_image;
    t.plane = gp->d_spec_plane;
    t.sum = gp->d_spec_sum[gp->spec_sum_idx];
    t.nf = 3 * gp->pixels_total;
    gp->spec_dev_iter = iter;
    gp->spec_iter = iter;
    gp->spec_launched += 1;
    return PT_OK;
}
// the call for the speculative frame's iteration: take it over on gp->stream
// on gp->stream (its image and counters) -- and, when the caller copies the image out, the copy
// stream waits for it too: the copy reads the finished sum at once, beside k_adopt_frame
int spec_adopt(bool copy_out) {
    const int iter = gp->spec_iter;
    hipError_t e = g_spec_launcher.wait();   // spec_ev_done recorded
    if (e == hipSuccess) e = hipStreamWaitEvent(gp->stream, gp->spec_ev_done, 0);
    if (e == hipSuccess && copy_out) e = hipStreamWaitEvent(gp->copy_stream, gp->spec_ev_done, 0);
    if (e != hipSuccess) {   // dropped: a retried call for this iteration traces it afresh
        (void)hipStreamSynchronize(gp->spec_stream);
        gp->spec_iter = 0;
        HIPCHK(e);
    }
    const int nf = 3 * gp->pixels_total;
    launch(7, k_adopt_frame, dim3(nblocks((nf + 3) / 4)), dim3(BLOCK), 0, (const float*)gp->d_spec_sum[gp->spec_sum_idx],
           gp->d_image, nf, gp->d_ctl, (const FrameCtl*)gp->d_ctl_spec, gp->ctl_rows);
    HIPCHK(hipGetLastError());
    gp->spec_iter = 0;
    gp->dev_iter = iter;
    gp->last_iter = iter;
    gp->frames_done += 1;
    gp->spec_adopted += 1;
    return PT_OK;
}

// frame `iter` speculated by every shard of the calling context, as one post to the launcher
int spec_launch(int iter) {
    RC(spec_worker_idle());   // the launcher is done with the previous launches (events, graphs)
    SpecJob job;
    job.n = nshards();
    for (int k = 0; k < job.n; ++k) {
        ShardScope sc(shard_ctx(k));
        RC(spec_prepare(iter, job.tasks[k]));
    }
    g_spec_launcher.post(job);
    return PT_OK;
}
// every shard's speculated frame waited for and dropped
int spec_cancel_all() {
    for (int k = 0; k < nshards(); ++k) {
        ShardScope sc(shard_ctx(k));
        RC(spec_cancel());
    }
    return PT_OK;
}
int need_single(const char* what) {
    if (M.n > 1) return fail(PT_E_UNSUPPORTED, "%s: one device context only (pt_options.num_devices > 1)", what);
    return spec_cancel();   // the test / profiling entry points use the path buffers themselves
}

