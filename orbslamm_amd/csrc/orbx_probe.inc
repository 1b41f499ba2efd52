// orbx_probe.inc -- extractor, part 7 of 7: stereo matching between two handles, and what looks inside one -- pyramid levels,
// FAST candidates, stream reset, the serial switch, the profiler's entries, the orbx_debug_* experiments.

// void Frame::ComputeStereoMatches()   src/Frame.cc:466-638
extern "C" int orbx_compute_stereo_matches(orbx_t* left, orbx_t* right, int frame, float mb, float mbf,
                                           float* u_right, float* depth, int cap, int* n_left)
{
    int rc = orbx_sync(right);
    if (rc) return rc;
    if ((rc = orbx_sync(left))) return rc;  // also leaves the device of `left` current
    if (left->device != right->device) return fail(ORBX_E_INVALID, "the two extractors live on different devices");
    if (left->curW == 0 || left->curW != right->curW || left->curH != right->curH || left->nlevels != right->nlevels)
        return fail(ORBX_E_INVALID, "left and right frames differ in shape or pyramid");
    if (frame < 0 || frame >= left->lastB || frame >= right->lastB) return fail(ORBX_E_INVALID, "frame %d not in the last batches", frame);
    if (!(mb > 0.f) || !(mbf > 0.f)) return fail(ORBX_E_INVALID, "stereo baseline (mb, mbf) must be positive");
    if (left->maxKp >= 65536 || right->maxKp >= 65536) return fail(ORBX_E_UNSUPPORTED, "more than 65535 keypoints per frame");
    int32_t n = 0;
    HIPCHK(hipMemcpy(&n, r_count(left, left->curSet) + 1 + frame, sizeof n, hipMemcpyDeviceToHost));
    if (n_left) *n_left = n;
    if (n > cap) return fail(ORBX_E_CAPACITY, "%d keypoints, caller capacity %d", n, cap);
    if (n == 0) return ORBX_OK;
    // scratch: three arrays of maxKp entries, grown on first use
    const size_t need = (size_t)left->maxKp * 12 + 64;
    if (need > left->stereoBytes && (rc = regrow_exact(left->d_stereo, left->stereoBytes, need, need))) return rc;
    StereoArgs a;
    a.kL = r_kps(left, left->curSet) + (size_t)(frame + 1) * left->maxKp; a.dL = r_desc(left, left->curSet) + (size_t)(frame + 1) * left->maxKp * 32;
    a.nL = r_count(left, left->curSet) + 1 + frame;
    a.kR = r_kps(right, right->curSet) + (size_t)(frame + 1) * right->maxKp; a.dR = r_desc(right, right->curSet) + (size_t)(frame + 1) * right->maxKp * 32;
    a.nR = r_count(right, right->curSet) + 1 + frame;
    a.gL = left->d_geom; a.gR = right->d_geom;
    a.srcL = left->lastSrc; a.srcR = right->lastSrc; a.srcL.f0 = a.srcR.f0 = 0;
    a.fL = a.fR = frame;
    for (int l = 0; l < ORBX_MAXL; l++) { a.sf[l] = l < left->nlevels ? left->mvScaleFactor[l] : 1.f; a.isf[l] = l < left->nlevels ? left->mvInvScaleFactor[l] : 1.f; }
    a.mb = mb; a.mbf = mbf;
    a.uRight = (float*)left->d_stereo; a.depth = a.uRight + left->maxKp; a.sad = (int32_t*)(a.depth + left->maxKp);
    int32_t* d_nAcc = a.sad + left->maxKp;
    hipStream_t s = left->stream;
    hipLaunchKernelGGL(k_stereo_match, dim3((n + 3) / 4), dim3(256), 0, s, a);
    const size_t lds = (size_t)left->maxKp * 4;
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_stereo_median, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_stereo_median, dim3(1), dim3(1024), lds, s, a.nL, (const int32_t*)a.sad, a.uRight, a.depth, d_nAcc);
    HIPCHK(hipGetLastError());
    if (u_right) HIPCHK(hipMemcpyAsync(u_right, a.uRight, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (depth) HIPCHK(hipMemcpyAsync(depth, a.depth, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

extern "C" int orbx_pyramid_level(orbx_t* h, int frame, int level, int blurred, uint8_t* dst, int* w, int* hh)
{
    int rc = orbx_sync(h);
    if (rc) return rc;
    if (h->curW == 0) return fail(ORBX_E_INVALID, "no frame extracted yet");
    if (level < 0 || level >= h->geom.nlevels || frame < 0 || frame >= h->lastB) return fail(ORBX_E_INVALID, "bad frame/level");
    const LevelGeom& L = h->geom.lv[level];
    if (w) *w = L.w;
    if (hh) *hh = L.h;
    if (!dst) return ORBX_OK;
    const uint8_t* srcp; size_t sp;
    if (blurred) { srcp = h->d_blur + (size_t)frame * h->geom.blurFrameBytes + L.blurOff; sp = L.blurStride; }
    else if (level == 0) { srcp = h->lastSrc.img0 + (size_t)frame * h->lastSrc.pitch0; sp = h->lastSrc.stride0; }
    else { srcp = h->d_pyr + (size_t)frame * h->geom.pyrFrameBytes + L.pyrOff; sp = L.stride; }
    HIPCHK(hipMemcpy2D(dst, L.w, srcp, sp, L.w, L.h, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_level_candidates(orbx_t* h, int frame, int level, uint64_t* dst, int cap, int* n)
{
    int rc = orbx_sync(h);
    if (rc) return rc;
    if (h->curW == 0 || level < 0 || level >= h->geom.nlevels || frame < 0 || frame >= h->lastB) return fail(ORBX_E_INVALID, "bad frame/level");
    // FAST leaves every cell's survivors in the cell's own segment: gather them
    const LevelGeom& L = h->geom.lv[level];
    std::vector<int32_t> counts(std::max(L.nCells, 1));
    if (L.nCells) HIPCHK(hipMemcpy(counts.data(), h->d_cellCount + (size_t)frame * h->geom.totalCells + L.cellBase, (size_t)L.nCells * 4, hipMemcpyDeviceToHost));
    int total = 0;
    for (int c = 0; c < L.nCells; c++) total += counts[c];
    if (n) *n = total;
    if (!dst) return ORBX_OK;
    if (total > cap) return fail(ORBX_E_CAPACITY, "%d candidates, capacity %d", total, cap);
    std::vector<uint64_t> seg(L.candCap);
    HIPCHK(hipMemcpy(seg.data(), h->d_candRaw + (size_t)frame * h->geom.candFrameRecs + L.candOff, (size_t)L.candCap * 8, hipMemcpyDeviceToHost));
    int o = 0;
    for (int c = 0; c < L.nCells; c++)
        for (int i = 0; i < counts[c]; i++) dst[o++] = seg[h->cells[L.cellBase + c].candOff + i];
    return ORBX_OK;
}

extern "C" int orbx_reset_stream(orbx_t* h)
{
    int rc = check_device(h);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    for (int set = 0; set < 2; set++) HIPCHK(hipMemsetAsync(r_count(h, set), 0, sizeof(int32_t), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbx_set_serial(orbx_t* h, int serial)
{
    int rc = check_device(h);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    h->serial = serial != 0;
    return ORBX_OK;
}

extern "C" int orbx_profile_enable(orbx_t* h, int enable)
{
    int rc = check_device(h);
    if (rc) return rc;
    h->prof.on = enable != 0;
    // events for ~250 steps up front, so that the timed region creates none
    if (enable) while (h->prof.pool.size() < 8192) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) break; h->prof.pool.push_back(e); }
    return ORBX_OK;
}

extern "C" int orbx_profile_select(orbx_t* h, const char* kernel)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (!kernel) { h->prof.only = -1; return ORBX_OK; }
    for (int i = 0; i < P_COUNT; i++)
        if (!strcmp(kernel, kProfNames[i])) { h->prof.only = i; return ORBX_OK; }
    return fail(ORBX_E_INVALID, "no kernel named %s", kernel);
}

extern "C" int orbx_profile_read(orbx_t* h, OrbxProfile* out, int reset)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    if ((rc = sync_all(h))) return rc;
    h->prof.collect();
    out->n = P_COUNT;
    for (int i = 0; i < P_COUNT; i++) {
        out->name[i] = kProfNames[i];
        out->ms[i] = h->prof.ms[i];
        out->launches[i] = h->prof.launches[i];
        if (reset) { h->prof.ms[i] = 0; h->prof.launches[i] = 0; }
    }
    return ORBX_OK;
}

// ------------------------------------------------------------------ co-run experiment (tools/pair_overlap.py)
// Kernel i repeated on one stream while kernel j runs on another for at least three times as long: the per-launch time of
// i beside j against i alone.  Works on the buffers of the last extracted + matched batch (every stage is idempotent on
// its inputs).  PMC counters cannot do this: rocprofv3 serialises dispatches while it collects them.
// Diagnostics: what the link gives plain pinned copies of the host path's sizes on THIS box -- the ceiling bench.py's
// host_path figures are read against.  up_bytes host-to-device and down_bytes device-to-host per repetition, first one
// direction at a time, then both at once on two streams (how the pipeline uses the link).  GB/s of payload.
extern "C" int orbx_debug_link_rate(orbx_t* h, size_t up_bytes, size_t down_bytes, int reps, float* h2d_gbs, float* d2h_gbs, float* both_up_gbs, float* both_down_gbs)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (!up_bytes || !down_bytes || reps < 1) return fail(ORBX_E_INVALID, "bad argument");
    void *hu = nullptr, *hd = nullptr, *du = nullptr, *dd = nullptr;
    hipStream_t s1 = nullptr, s2 = nullptr;
    auto cleanup = [&]() { if (hu) (void)hipHostFree(hu); if (hd) (void)hipHostFree(hd); if (du) (void)hipFree(du); if (dd) (void)hipFree(dd); if (s1) (void)hipStreamDestroy(s1); if (s2) (void)hipStreamDestroy(s2); };
    HIPCHK_OR(hipHostMalloc(&hu, up_bytes), cleanup()); HIPCHK_OR(hipHostMalloc(&hd, down_bytes), cleanup()); HIPCHK_OR(hipMalloc(&du, up_bytes), cleanup()); HIPCHK_OR(hipMalloc(&dd, down_bytes), cleanup());
    HIPCHK_OR(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking), cleanup()); HIPCHK_OR(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking), cleanup());
    memset(hu, 1, up_bytes);
    HIPCHK_OR(hipMemsetAsync(dd, 2, down_bytes, s2), cleanup()); HIPCHK_OR(hipStreamSynchronize(s2), cleanup());
    using clk = std::chrono::steady_clock;
    auto run = [&](bool up, bool down, double& sec) -> hipError_t {
        for (int w = 0; w < 2; w++) {   // first round warms the queues
            const auto t0 = clk::now();
            for (int i = 0; i < reps; i++) {
                hipError_t e;
                if (up && (e = hipMemcpyAsync(du, hu, up_bytes, hipMemcpyHostToDevice, s1)) != hipSuccess) return e;
                if (down && (e = hipMemcpyAsync(hd, dd, down_bytes, hipMemcpyDeviceToHost, s2)) != hipSuccess) return e;
            }
            hipError_t e;
            if ((e = hipStreamSynchronize(s1)) != hipSuccess || (e = hipStreamSynchronize(s2)) != hipSuccess) return e;
            sec = std::chrono::duration<double>(clk::now() - t0).count();
        }
        return hipSuccess;
    };
    double t = 0;
    HIPCHK_OR(run(true, false, t), cleanup()); if (h2d_gbs) *h2d_gbs = (float)(up_bytes * (double)reps / t / 1e9);
    HIPCHK_OR(run(false, true, t), cleanup()); if (d2h_gbs) *d2h_gbs = (float)(down_bytes * (double)reps / t / 1e9);
    HIPCHK_OR(run(true, true, t), cleanup());
    if (both_up_gbs) *both_up_gbs = (float)(up_bytes * (double)reps / t / 1e9);
    if (both_down_gbs) *both_down_gbs = (float)(down_bytes * (double)reps / t / 1e9);
    cleanup();
    return ORBX_OK;
}

extern "C" int orbx_debug_stage_rows(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t w, int rows)
{
    if (!dst || !src || rows < 0 || dpitch < w || spitch < w) return fail(ORBX_E_INVALID, "bad argument");
    stage_rows(dst, dpitch, src, spitch, w, rows);
    return g_stageNt && w >= 128 && !(((uintptr_t)dst | dpitch) & 31) ? 1 : 0;
}

extern "C" int orbx_debug_blur_ops(int walk, uint32_t* dst, int* steps_per_run)
{
    if (!dst) return fail(ORBX_E_INVALID, "bad argument");
    static constexpr BlurOps kTile = make_blur_ops(false), kWalk = make_blur_ops(true);
    memcpy(dst, walk ? kWalk.v : kTile.v, sizeof kTile.v);
    if (steps_per_run) *steps_per_run = kBlurRunSteps;
    return ORBX_OK;
}

extern "C" int orbx_debug_pair_overlap(orbx_t* h, int nb, float target_ms, int* n_kernels, const char** names,
                                       float* alone_ms, float* co_ms, int32_t* lds_bytes, int32_t* wg_threads, int32_t* wgs)
{
    int rc = orbx_sync(h);
    if (rc) return rc;
    if (h->lastB < 1 || nb < 1 || nb > h->lastB) return fail(ORBX_E_INVALID, "run a batch of at least %d frames first", nb);
    if (!h->streamP[1]) return fail(ORBX_E_UNSUPPORTED, "a latency handle has one chain stream: create the handle with orbx_create and max_batch > 2");
    constexpr int K = 6;
    static const char* kNames[K] = {"k_pyramid", "k_fast", "k_distribute", "k_blur", "k_orient_desc", "k_match_mfma"};
    if (n_kernels) *n_kernels = K;
    const Geom& g = h->geom;
    FrameSrc src = h->lastSrc; src.f0 = 0;
    Launcher L{h, src, nb};
    const int set = h->curSet, cellsL0 = g.lv[0].nCells;
    auto launch = [&](int k, hipStream_t s) {
        switch (k) {
        case 0: (void)L.pyramid(s); break;
        case 1: L.fast(s, 0, cellsL0); L.fast(s, cellsL0, g.totalCells - cellsL0); break;
        case 2: L.dist(s, 0, g.nlevels); break;
        case 3: L.blur(s); break;
        case 4: (void)L.desc(s, set); break;
        default: match_kernels(h, s, set, nb, 0.7f, 50, 1); break;
        }
    };
    if (lds_bytes && wg_threads && wgs) {
        const size_t pl = pyr_lds_bytes(h->pyrBufA, h->pyrBufB, h->pyrTabCap);
        const size_t fl = fast_lds_bytes(h->tileRows, h->tileStrideDw, h->fastSmapPitch, h->fastListCap);
        const int nqb = (h->maxKp + orbm::kMfmaRowsPerBlock - 1) / orbm::kMfmaRowsPerBlock;
        const int32_t l[K] = {(int32_t)pl, (int32_t)fl, (int32_t)(dist_lds_bytes(h->nodeCap, g.maxCellsPerLevel) + 5552), (kBlurWalkInWords + kBlurMfmaOutWords) * 4, 31104, orbm::kMfmaLdsBytes};
        const int32_t t[K] = {256, 64, kDistThreads, 256, kKpPerBlock / 8 * 64, 256};
        const int32_t w[K] = {h->pyrBlocks * nb, g.totalCells * nb, g.nlevels * nb, h->blurRuns.base[g.nlevels] * nb, h->kpBlocksTotal * nb, nqb * nb};
        for (int k = 0; k < K; k++) { lds_bytes[k] = l[k]; wg_threads[k] = t[k]; wgs[k] = w[k]; }
    }
    for (int k = 0; k < K; k++) if (names) names[k] = kNames[k];
    hipStream_t sa = h->streamP[0], sb = h->streamP[1];
    hipEvent_t e0, e1, eGo;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventCreateWithFlags(&eGo, hipEventDisableTiming));
    auto timed = [&](int i, int j, int ni, int nj, float& ms) -> int {  // j < 0: alone
        HIPCHK(hipEventRecord(eGo, h->stream));
        HIPCHK(hipStreamWaitEvent(sa, eGo, 0));
        if (j >= 0) { HIPCHK(hipStreamWaitEvent(sb, eGo, 0)); for (int r = 0; r < nj / 4; r++) launch(j, sb); }  // a head start
        HIPCHK(hipEventRecord(e0, sa));
        for (int r = 0; r < ni; r++) { launch(i, sa); if (j >= 0) for (int q = 0; q * ni < nj - nj / 4 && q < 8; q++) launch(j, sb); }
        HIPCHK(hipEventRecord(e1, sa));
        HIPCHK(hipStreamSynchronize(sa)); HIPCHK(hipStreamSynchronize(sb));
        float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1));
        ms = t / ni;
        return ORBX_OK;
    };
    float alone[K];
    for (int i = 0; i < K; i++) {
        float t;
        if ((rc = timed(i, -1, 4, 0, t))) return rc;                  // warm
        if ((rc = timed(i, -1, 20, 0, t))) return rc;
        alone[i] = t;
        if (alone_ms) alone_ms[i] = t;
    }
    for (int i = 0; i < K; i++)
        for (int j = 0; j < K; j++) {
            const int ni = std::max(4, (int)(target_ms / alone[i]));
            const int nj = std::max(8, (int)(4.f * ni * alone[i] / alone[j]));   // j's stream stays busy ~4x as long as i's alone time
            float t;
            if ((rc = timed(i, j, ni, nj, t))) return rc;
            if (co_ms) co_ms[i * K + j] = t;
        }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(eGo);
    return orbx_sync(h);
}
