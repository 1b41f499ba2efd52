// orbx_streams.inc -- extractor, part 3 of 7: the two process-wide stream pools, a handle's create and destroy (every device
// block and event it owns), and what drains or joins its streams (sync_all, flush_pack, flush_part_event, join_parts).

// The chain streams of the latency handles (one robot's live stream each).  The GPU executes about four queues at a time
// and rotates the rest in (tools/live_scale_probe.sh), so K robots are best served by min(K, 4) queues with the chains of
// the robots that share one simply following each other.  A stream gets its hardware queue from the runtime, which does
// NOT spread the streams of handles created one after the other or by several threads at once: traced with rocprofv3
// (tools/live_queues.sh), four robots' own streams landed 1 + 3 on two queues when created under a lock (6.8 k frames/s)
// and anything between 4 x 1 and 2 + 1 + 1 when created concurrently (the same program read 30 k or 18.6 k frames/s
// from run to run).  Four streams created and first used back to back get four queues; the handles take them in turn.
struct ChainPool { hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr}; int users[4] = {0, 0, 0, 0}; bool made = false; };
static ChainPool g_chain[64];
static std::mutex g_chainMu;

// ORBX_LAT_PRIO=0: the chain streams at normal priority.  ONE answer per process, asked by every acquirer (the latency
// extractors and the matchers' thread handles): the first acquirer makes the pool, and a matcher that always asked for
// "high" used to fix the pool's priority before the extractor's switch was looked at (ADVICE r5).
static bool chain_prio_normal() { static const bool v = env_char("ORBX_LAT_PRIO") == '0'; return v; }

static int chain_stream_acquire(int device, int priority, hipStream_t* out, int* idx)
{
    std::lock_guard<std::mutex> lk(g_chainMu);
    ChainPool& cp = g_chain[device & 63];
    if (!cp.made) {
        // made into locals and committed only when all four exist and have been used once: a failure half way leaves the
        // pool empty (the next caller tries again) instead of half made
        hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr};
        void* scratch = nullptr;
        hipError_t e = hipMalloc(&scratch, 256);
        for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipStreamCreateWithPriority(&s[i], hipStreamNonBlocking, priority);
        for (int i = 0; i < 4 && e == hipSuccess; i++) { e = hipMemsetAsync(scratch, 0, 256, s[i]); if (e == hipSuccess) e = hipStreamSynchronize(s[i]); }
        if (scratch) (void)hipFree(scratch);
        if (e != hipSuccess) {
            for (hipStream_t st : s) if (st) (void)hipStreamDestroy(st);
            return fail(ORBX_E_HIP, "cannot make the chain streams of device %d: %s", device, hipGetErrorString(e));
        }
        for (int i = 0; i < 4; i++) cp.s[i] = s[i];
        cp.made = true;
    }
    int best = 0;
    for (int i = 1; i < 4; i++) if (cp.users[i] < cp.users[best]) best = i;
    cp.users[best]++;
    *out = cp.s[best]; *idx = best;
    return ORBX_OK;
}

static void chain_stream_release(int device, int idx)
{
    std::lock_guard<std::mutex> lk(g_chainMu);
    if (idx >= 0 && idx < 4) g_chain[device & 63].users[idx]--;
}

// The four pipeline streams of the throughput handles (more than two frames per call) of a device are ONE set per process:
// every stream a process keeps busy takes part in the GPU's queue rotation (about four run at a time), so two robots'
// offline sequences with four streams each ran at 122 k frames/s together where one runs at 166 k
// (examples/multi_robot --mode batch --robots 2).  Sharing the set, the robots' sub-batches simply follow each other in the
// same four queues; every dependency is an event between streams as before.  (A set per handle was the A/B of round 4.)
struct TputPool { hipStream_t host = nullptr, p[orbx_handle::kMaxSplit] = {nullptr}, match = nullptr; int users = 0; };
static TputPool g_tput[64];
static std::mutex g_tputMu;

static int tput_streams_acquire(orbx_handle* h, int device, int prHi)
{
    std::lock_guard<std::mutex> lk(g_tputMu);
    TputPool& tp = g_tput[device & 63];
    if (!tp.host) {
        // the four streams the pipeline keeps busy are the first four made (later ones share a hardware queue), and queues are
        // bound at a stream's first use: made and used once in this order, the spare sub-batch streams (splits of more than two, unused by the shipped configuration) after.
        // All into a local set, committed only when complete: a failure half way leaves the pool empty, not half made with
        // null streams (the legacy default stream) handed to every later handle.
        TputPool t;
        void* scratch = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&t.host, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&t.p[0], hipStreamNonBlocking, prHi);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&t.p[1], hipStreamNonBlocking, prHi);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&t.match, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc(&scratch, 256);
        for (hipStream_t st : {t.host, t.p[0], t.p[1], t.match}) {
            if (e == hipSuccess) e = hipMemsetAsync(scratch, 0, 256, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (scratch) (void)hipFree(scratch);
        for (int i = 2; i < orbx_handle::kMaxSplit && e == hipSuccess; i++) e = hipStreamCreateWithPriority(&t.p[i], hipStreamNonBlocking, prHi);
        if (e != hipSuccess) {
            for (hipStream_t st : {t.host, t.match}) if (st) (void)hipStreamDestroy(st);
            for (hipStream_t st : t.p) if (st) (void)hipStreamDestroy(st);
            return fail(ORBX_E_HIP, "cannot make the pipeline streams of device %d: %s", device, hipGetErrorString(e));
        }
        tp.host = t.host; tp.match = t.match;
        for (int i = 0; i < orbx_handle::kMaxSplit; i++) tp.p[i] = t.p[i];
    }
    tp.users++;
    h->stream = tp.host; h->stream3 = tp.match;
    for (int i = 0; i < orbx_handle::kMaxSplit; i++) h->streamP[i] = tp.p[i];
    h->sharedStreams = true;
    return ORBX_OK;
}

static void tput_streams_release(orbx_handle* h)
{
    std::lock_guard<std::mutex> lk(g_tputMu);
    TputPool& tp = g_tput[h->device & 63];
    h->stream = nullptr; h->stream3 = nullptr;
    for (int i = 0; i < orbx_handle::kMaxSplit; i++) h->streamP[i] = nullptr;
    h->sharedStreams = false;
    // The set outlives its users: the streams a process makes FIRST are the ones with a hardware queue each, so a handle
    // created after another was destroyed gets these again instead of later-made ones that share a queue.
    --tp.users;
}

static constexpr int kMatchChunks = 4;  // train chunks per query block (wave count x4)

// ------------------------------------------------------------------ create / destroy
// Ownership in one place: what a handle allocates at create goes through these two and is noted on the handle;
// free_device frees the lists (also those of a half-built handle: undo() in create_handle).
template <class T> static hipError_t dev_alloc(orbx_handle* h, T*& p, size_t bytes)
{
    const hipError_t e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) h->ownedBlocks.push_back(p);
    return e;
}
static hipError_t new_event(orbx_handle* h, hipEvent_t& ev)
{
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) h->ownedEvents.push_back(ev);
    return e;
}
// The three blocks that are regrown after create (d_distScratch, d_pyrRanges, d_stereo) are replaced by one of exactly the
// size asked for -- grow_device's 3/2 would change the footprint -- and freed by free_device beside the list.
template <class T> static int regrow_exact(T*& p, size_t& cap, size_t newCap, size_t bytes)
{
    if (p) HIPCHK(hipFree(p));
    p = nullptr; cap = 0;
    HIPCHK(hipMalloc((void**)&p, bytes));
    cap = newCap;
    return ORBX_OK;
}

static void free_device(orbx_handle* h)
{
    if (h->device < 0) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipStream_t st : h->streamP) if (st) (void)hipStreamSynchronize(st);
    if (h->stream3) (void)hipStreamSynchronize(h->stream3);
    h->prof.destroy();
    for (void* p : h->ownedBlocks) (void)hipFree(p);   // (no clear(): every caller deletes the handle next)
    for (void* p : {(void*)h->d_distScratch, (void*)h->d_pyrRanges, h->d_stereo}) if (p) (void)hipFree(p);
    h->pool.stop();
    for (hipStream_t st : {h->streamUp, h->streamDown, h->streamUpQ, h->streamDownQ}) if (st) (void)hipStreamSynchronize(st);
    for (auto& sl : h->slot) {
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_out) (void)hipFree(sl.d_out);
        for (hipEvent_t& e : sl.evUp) if (e) (void)hipEventDestroy(e);
        if (sl.evOut) (void)hipEventDestroy(sl.evOut);
        if (sl.evPacked) (void)hipEventDestroy(sl.evPacked);
    }
    for (hipStream_t st : {h->streamUp, h->streamDown, h->streamUpQ, h->streamDownQ}) if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : h->ownedEvents) (void)hipEventDestroy(e);
    // pooled streams are released, not destroyed: the pipeline set of a throughput handle, the chain stream of a latency handle
    if (h->sharedStreams) tput_streams_release(h);
    if (h->stream) (void)hipStreamDestroy(h->stream);   // (a latency handle's own aux stream)
    if (h->chainIdx >= 0) { chain_stream_release(h->device, h->chainIdx); h->chainIdx = -1; h->streamP[0] = nullptr; }
}

static int create_handle(const OrbxParams* params, int max_w, int max_h, int max_batch, int device, int latCeil, orbx_t** out)
{
    if (!params || !out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    orbx_handle* h = new orbx_handle();
    h->latMaxB = latCeil;
    h->prm = *params;
    int rc = init_tables(h);
    if (rc) { delete h; return rc; }
    h->device = device;
    h->serial = env_char("ORBX_SERIAL") == '1';
    h->matchPopcount = env_char("ORBX_MATCH_POPCOUNT") == '1';
    h->fuseExpand = !h->matchPopcount;   // the matrix-core scan reads the +-1 form k_orient_desc writes beside the 32-byte descriptors
    { const char c = env_char("ORBX_LAT_STREAMS"); if (c == '1' || c == '2') h->latStreams = c - '0'; }
    h->maxW = max_w; h->maxH = max_h; h->maxB = max_batch;
    if (device < 0) { *out = h; return ORBX_OK; }  // host-only handle: tables and geometry queries
    if (max_w < 1 || max_h < 1 || max_batch < 1) { delete h; return fail(ORBX_E_INVALID, "bad maximum shape"); }
    int ndev = orbx_device_count();
    if (ndev == 0) { delete h; return fail(ORBX_E_NO_DEVICE, "no HIP device visible: the ORB front-end has no CPU fallback"); }
    if (device >= ndev) { delete h; return fail(ORBX_E_INVALID, "device %d out of range (%d visible)", device, ndev); }

    HostGeom hg;
    rc = build_geometry(h, max_w, max_h, hg);
    if (rc) { delete h; return rc; }
    auto undo = [&]() { if (h->countedLat) g_latHandles[device & 63].fetch_sub(1); free_device(h); delete h; };   // the half-built handle
    HIPCHK_OR(hipSetDevice(device), undo());
    // The first four streams of a process get a hardware queue each, later ones share the last (observed with
    // rocprofv3 --kernel-trace), and two busy streams on one queue serialise.  The steady-state pipeline therefore
    // uses exactly four: the host-facing stream (uploads, downloads -- idle while a device-resident stream runs --
    // and the blur kernels), sub-batch 0, sub-batch 1, matching.
    // The sub-batch streams carry the chain pyramid -> FAST -> quadtree -> descriptors whose length IS the step; the blur /
    // level-0 FAST stream and the matcher have slack.  Queue priority (which queue's workgroups the dispatcher places
    // first) for the chain: 142.6 k -> 144.0 k frames/s; raising the matcher instead: 138.2 k, the blur stream: 140.6 k.
    int prLo = 0, prHi = 0;
    HIPCHK_OR(hipDeviceGetStreamPriorityRange(&prLo, &prHi), undo());
    const bool latHandle = max_batch <= latCeil;   // every call runs the latency-mode chain; else a throughput handle
    if (!latHandle) {
        // the throughput handles of a device share ONE set of four streams (a set per handle: -7 % with two robots)
        rc = tput_streams_acquire(h, device, prHi);
        if (rc) { free_device(h); delete h; return rc; }
    } else {
        HIPCHK_OR(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), undo());
        // ORBX_LAT_PRIO=0 puts a latency handle's chain at normal priority, the level of the matcher's stream.  High is the
        // default because the high-priority streams of a process get hardware queues of their own pool: K robots' chains then
        // sit on K different queues (17.4 k frames/s with four robots; 5.3 k when they share the normal pool with the
        // matchers' idle streams).  The price: a frame set that is NOT attached (its search on the matcher's normal-priority
        // queue beside the next extraction on the high-priority one) is time-sliced against it in ~50 us quanta --
        // tools/live_d2_trace.sh: 2.7 k frames/s two tickets deep, 8.2 k with both queues at one level.
        if (chain_prio_normal()) prHi = 0;
        // A latency handle's chain runs on one of FOUR process-wide chain streams per device (chain_stream_acquire): which
        // hardware queue a stream of its own would get is the runtime's business, and it does not spread them
        int idx = -1;
        rc = chain_stream_acquire(device, prHi, &h->streamP[0], &idx);
        if (rc) { free_device(h); delete h; return rc; }
        h->chainIdx = idx;
        // (a latency handle never uses a second sub-batch stream or the matching stream: not created, no queue taken)
    }
    // hardware queues are bound at a stream's first use
    {
        void* scratch = nullptr;
        HIPCHK_OR(hipMalloc(&scratch, 256), undo());
        // A latency handle (one or two frames per call: one robot's live stream) only ever keeps its chain's stream(s)
        // busy: bind just those, so that the handles of K robots in one process land on K different hardware queues
        // instead of all putting their chain on the second queue of four
        if (latHandle) { g_latHandles[device & 63].fetch_add(1); h->countedLat = true; }
        // (a latency handle's chain stream is bound already; its aux stream only where the two-queue form will run; the
        // shared set of a throughput handle was bound when it was made)
        if (latHandle && h->latStreams == 2) { HIPCHK_OR(hipMemsetAsync(scratch, 0, 256, h->stream), undo()); HIPCHK_OR(hipStreamSynchronize(h->stream), undo()); }
        HIPCHK_OR(hipFree(scratch), undo());
    }
    for (int i = 0; i < orbx_handle::kMaxSplit; i++) {
        HIPCHK_OR(new_event(h, h->evPyr[i]), undo());
        HIPCHK_OR(new_event(h, h->evBlur[i]), undo());
        HIPCHK_OR(new_event(h, h->evPart[i]), undo());
        HIPCHK_OR(new_event(h, h->evFast0[i]), undo());
    }
    HIPCHK_OR(new_event(h, h->evStart), undo());
    for (int i = 0; i < 2; i++) { HIPCHK_OR(new_event(h, h->evMatch[i]), undo()); HIPCHK_OR(new_event(h, h->evMatched[i]), undo()); }
    const size_t B = (size_t)max_batch;
    // capacities with head-room so that smaller shapes (different cell layouts) also fit
    h->cellsCap = hg.cells.size() * 2 + 64;
    h->tabsCap = hg.tabs.size() * 2 + 64;
    h->imgFrameBytes = (size_t)align_up(max_w, 64) * max_h;
    h->pyrCapFrame = (size_t)hg.g.pyrFrameBytes + 4096;
    h->blurCapFrame = (size_t)hg.g.blurFrameBytes + 4096;
    h->candCapFrame = (size_t)hg.g.candFrameRecs + 1024;
    h->keptCapFrame = (size_t)hg.g.keptFrameRecs + 64;
    h->maxKp = hg.g.maxKp + 64;
    // the geometry block, and behind it k_orient_desc's tables: they depend on the pattern and on umax alone, so they are made
    // here once (configure_shape rewrites the Geom in front of them for every new shape)
    HIPCHK_OR(dev_alloc(h, h->d_geom, sizeof(Geom) + sizeof(OrientTables)), undo());
    {
        OrientTables ot;
        build_orient_tables(h->umax, ot);
        HIPCHK_OR(hipMemcpy(h->d_geom + 1, &ot, sizeof ot, hipMemcpyHostToDevice), undo());
    }
    HIPCHK_OR(dev_alloc(h, h->d_cells, h->cellsCap * sizeof(Cell)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_tabs, h->tabsCap * sizeof(short4)), undo());
    h->pyrRangesCap = 64 * ORBX_MAXL;
    HIPCHK_OR(hipMalloc(&h->d_pyrRanges, h->pyrRangesCap * sizeof(PyrRange)), undo());   // (regrown by configure_shape: not in the list)
    HIPCHK_OR(dev_alloc(h, h->d_pyr, h->pyrCapFrame * B), undo());
    HIPCHK_OR(dev_alloc(h, h->d_blur, h->blurCapFrame * B), undo());
    HIPCHK_OR(dev_alloc(h, h->d_candRaw, h->candCapFrame * B * sizeof(uint64_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_candA, h->candCapFrame * B * sizeof(uint64_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_candB, h->candCapFrame * B * sizeof(uint64_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_candCount, B * ORBX_MAXL * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_cellCount, B * h->cellsCap * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_kept, h->keptCapFrame * B * sizeof(uint64_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_keptCount, B * ORBX_MAXL * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_err, 8 * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_kps, 2 * (B + 1) * h->maxKp * sizeof(OrbxKeyPointDev)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_desc, 2 * (B + 1) * (size_t)h->maxKp * 32), undo());
    HIPCHK_OR(dev_alloc(h, h->d_count, 2 * (B + 1) * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_match, 2 * B * h->maxKp * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_binOf, B * (size_t)h->maxKp), undo());
    HIPCHK_OR(dev_alloc(h, h->d_hist, B * 32 * sizeof(int32_t)), undo());
    HIPCHK_OR(dev_alloc(h, h->d_nmatch, 2 * B * sizeof(int32_t)), undo());
    h->partialSlots = std::max<size_t>(B * kMatchChunks, 16);  // few frames: up to 8 train chunks per frame (k_match_mfma)
    HIPCHK_OR(dev_alloc(h, h->d_partial, h->partialSlots * h->maxKp * sizeof(uint2)), undo());
    // a slot of the +-1 buffer: the descriptors in MFMA tile order, then the keypoints' ANGLES as a plain float array (round 5:
    // the acceptance rule's rotation test read them out of the 28-byte keypoint records -- 7 MB of the stream matcher's 22 MB
    // of fetches per step for 1 MB of angles)
    h->xAngOff = (int64_t)align_up(h->maxKp, orbm::kMfmaRowsPerBlock) * orbm::kMfmaDescBytes;
    h->xPitch = h->xAngOff + (int64_t)align_up(h->maxKp * 4, 4096);
    HIPCHK_OR(hipFuncSetAttribute((const void*)orbm::k_match_mfma, hipFuncAttributeMaxDynamicSharedMemorySize, orbm::kMfmaLdsBytes), undo());  // its ring of train tiles
    HIPCHK_OR(dev_alloc(h, h->d_xdesc, 2 * (B + 1) * (size_t)h->xPitch), undo());
    HIPCHK_OR(hipMemset(h->d_xdesc, 0, 2 * (B + 1) * (size_t)h->xPitch), undo());
    HIPCHK_OR(hipMemset(h->d_err, 0, 8 * sizeof(int32_t)), undo());
    h->d_errCur = h->d_err;
    HIPCHK_OR(hipMemset(h->d_count, 0, 2 * (B + 1) * sizeof(int32_t)), undo());
    HIPCHK_OR(hipMemset(h->d_hist, 0, B * 32 * sizeof(int32_t)), undo());
    HIPCHK_OR(hipMemset(h->d_nmatch, 0, 2 * B * sizeof(int32_t)), undo());
    live_add(h);
    *out = h;
    return ORBX_OK;
}

extern "C" int orbx_create(const OrbxParams* params, int max_w, int max_h, int max_batch, int device, orbx_t** out)
{
    return create_handle(params, max_w, max_h, max_batch, device, lat_max_b(), out);
}

// A handle for the LIVE frames of up to max_cameras (<= 8) cameras: every call of 1 .. max_cameras frames runs the
// latency-mode chain (one queue, frames up by a copy kernel, results behind a flag).  What a hub that gathers the frames
// of several robots' tracking threads creates (include/orbslamm_hub.hpp); orbx_create keeps that mode to one or two frames.
extern "C" int orbx_create_live(const OrbxParams* params, int max_w, int max_h, int max_cameras, int device, orbx_t** out)
{
    if (max_cameras < 1 || max_cameras > kLatMaxBatchCeil) return fail(ORBX_E_INVALID, "a live handle takes 1..%d cameras per call (%d asked for): larger batches are orbx_create's throughput mode", kLatMaxBatchCeil, max_cameras);
    return create_handle(params, max_w, max_h, max_cameras, device, std::max(max_cameras, lat_max_b()), out);
}

extern "C" void orbx_destroy(orbx_t* h)
{
    if (!h) return;
    if (h->countedLat) g_latHandles[h->device & 63].fetch_sub(1);
    live_remove(h);
    free_device(h);
    delete h;
}

// ------------------------------------------------------------------ draining and joining
static int flush_pack(orbx_handle* h)
{
    if (!h->packPending) return ORBX_OK;
    h->packPending = false;
    hipLaunchKernelGGL(k_pack_host, dim3(16, h->packB), dim3(256), 0, h->streamP[0], h->packPa);
    HIPCHK(hipGetLastError());
    return ORBX_OK;
}

static int sync_all(orbx_handle* h)
{
    { int rcp = flush_pack(h); if (rcp) return rcp; }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (hipStream_t st : h->streamP) if (st) HIPCHK(hipStreamSynchronize(st));
    if (h->stream3) HIPCHK(hipStreamSynchronize(h->stream3));
    for (hipStream_t st : {h->streamUp, h->streamDown, h->streamUpQ, h->streamDownQ}) if (st) HIPCHK(hipStreamSynchronize(st));
    h->matchPending[0] = h->matchPending[1] = false;
    h->evOutOfSet[0] = h->evOutOfSet[1] = nullptr;
    return ORBX_OK;
}

// make `s` wait for every sub-batch of the last extraction
// An event between two kernels of a stream costs ~5 us of gap (a record riding on the kernel's own packet as well:
// tools/live_timeline.sh), and in the latency mode the chain of kernels IS the call -- so the chain's "done" event is
// not put into the queue behind the descriptors but recorded when somebody on another stream asks for it: later on the
// same stream, hence never too early.
static int flush_part_event(orbx_handle* h)
{
    if (h->partLazy) { HIPCHK(hipEventRecord(h->evPart[0], h->streamP[0])); h->partLazy = false; }
    return ORBX_OK;
}

static int join_parts(orbx_handle* h, hipStream_t s)
{
    int rc = flush_part_event(h);
    if (rc) return rc;
    for (int p = 0; p < h->lastParts; p++) HIPCHK(hipStreamWaitEvent(s, h->evPart[p], 0));
    return ORBX_OK;
}
