// orbx_pipeline.inc -- extractor, part 4 of 7: a frame shape onto the device (configure_shape), the kernel launches of one
// (sub-)batch (Launcher), the event graph of a call (run_extract), the device-resident entries.

// ------------------------------------------------------------------ shape configuration
static int configure_shape(orbx_handle* h, int w, int hh)
{
    if (h->curW == w && h->curH == hh) return ORBX_OK;
    if (w > h->maxW || hh > h->maxH) return fail(ORBX_E_INVALID, "frame %dx%d exceeds the handle's maximum %dx%d", w, hh, h->maxW, h->maxH);
    HostGeom hg;
    int rc = build_geometry(h, w, hh, hg);
    if (rc) return rc;
    if (hg.cells.size() > h->cellsCap || hg.tabs.size() > h->tabsCap || (size_t)hg.g.pyrFrameBytes > h->pyrCapFrame ||
        (size_t)hg.g.blurFrameBytes > h->blurCapFrame || (size_t)hg.g.candFrameRecs > h->candCapFrame ||
        (size_t)hg.g.keptFrameRecs > h->keptCapFrame || hg.g.maxKp > h->maxKp)
        return fail(ORBX_E_INVALID, "frame %dx%d needs more scratch than the handle was created with", w, hh);
    const size_t dl = dist_lds_bytes(hg.nodeCap, hg.g.maxCellsPerLevel);
    h->distInLds = dl <= 156 * 1024;
    if (h->distInLds && dl > 48 * 1024 &&
        hipFuncSetAttribute((const void*)k_distribute<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl) != hipSuccess) {
        // the kernel's static LDS (a few KB) comes on top of the dynamic part: a node list within a few KB of the CU's 160 KB is
        // refused by the runtime -- found by tests/soak/fuzz_soak.py (3 990 features on one level) -- and takes the global-scratch form
        (void)hipGetLastError();
        h->distInLds = false;
    }
    if (h->distInLds) {
        // (the fused form carries two blur tiles' static LDS as well: where that does not fit beside the node lists, the two kernels follow each other)
        h->distBlurOk = hipFuncSetAttribute((const void*)k_distribute_blur, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl) == hipSuccess;
        if (!h->distBlurOk) (void)hipGetLastError();
    } else {
        // per-level target too large for LDS: node list in a global scratch region per (frame, level)
        const size_t need = dl * (size_t)h->maxB * hg.g.nlevels;
        if (need > h->distScratchBytes && ((rc = sync_all(h)) || (rc = regrow_exact(h->d_distScratch, h->distScratchBytes, need, need)))) return rc;
    }
    hg.g.maxKp = h->maxKp;  // output slots keep their create-time pitch
    if ((rc = sync_all(h))) return rc;
    HIPCHK(hipMemcpy(h->d_geom, &hg.g, sizeof(Geom), hipMemcpyHostToDevice));
    if (!hg.cells.empty()) HIPCHK(hipMemcpy(h->d_cells, hg.cells.data(), hg.cells.size() * sizeof(Cell), hipMemcpyHostToDevice));
    if (!hg.tabs.empty()) HIPCHK(hipMemcpy(h->d_tabs, hg.tabs.data(), hg.tabs.size() * sizeof(short4), hipMemcpyHostToDevice));
    h->pyrFused = hg.pyrFused;
    if (hg.pyrFused) {
        if (hg.pyrRanges.size() > h->pyrRangesCap && (rc = regrow_exact(h->d_pyrRanges, h->pyrRangesCap, hg.pyrRanges.size(), hg.pyrRanges.size() * sizeof(PyrRange)))) return rc;
        HIPCHK(hipMemcpy(h->d_pyrRanges, hg.pyrRanges.data(), hg.pyrRanges.size() * sizeof(PyrRange), hipMemcpyHostToDevice));
        h->pyrBlocks = hg.pyrBlocks; h->pyrBufA = hg.pyrBufA; h->pyrBufB = hg.pyrBufB; h->pyrTabCap = hg.pyrTabCap;
        const size_t pl = pyr_lds_bytes(h->pyrBufA, h->pyrBufB, h->pyrTabCap);
        if (pl > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_pyramid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl));
    }
    for (int l = 0; l < ORBX_MAXL; l++) {
        h->tabs.xtab[l] = h->d_tabs + (l < hg.g.nlevels ? hg.xoff[l] : 0);
        h->tabs.ytab[l] = h->d_tabs + (l < hg.g.nlevels ? hg.yoff[l] : 0);
    }
    h->geom = hg.g;
    h->cells = hg.cells;
    h->tileStrideDw = hg.tileStrideDw; h->tileRows = hg.tileRows; h->fastListCap = hg.fastListCap; h->nodeCap = hg.nodeCap;
    h->tileRows0 = hg.tileRows0; h->fastListCap0 = hg.fastListCap0;
    h->fastSmapPitch = hg.fastSmapPitch; h->fastSmapPitch0 = hg.fastSmapPitch0;
    h->blurTiles = hg.bt; h->blurRuns = hg.br; h->kpBlocks = hg.kb; h->kpBlocksTotal = hg.kbTotal;
    h->curW = w; h->curH = hh;
    // a new shape starts a new stream
    for (int set = 0; set < 2; set++) HIPCHK(hipMemset(r_count(h, set), 0, sizeof(int32_t)));
    return ORBX_OK;
}

// ------------------------------------------------------------------ the pipeline
// grid.y of the launches that map (block, frame) through xcd_block_frame
static inline unsigned xcd_grid_y(int nb) { return nb < 8 ? (unsigned)nb : 8u * (unsigned)((nb + 7) / 8); }
// xcdFrames of k_pyramid and k_distribute: from eight frames on a frame's blocks go to ONE XCD (0: the plain (block, frame) grid)
static inline int xcd_frames(int nb) { return nb >= 8 ? nb : 0; }
template <class T> struct as_declared { using type = T; };   // (keeps launch_done's arguments out of template deduction)

// done != nullptr: the event rides on the kernel's own dispatch packet (hipExtLaunchKernelGGL) -- a separate
// hipEventRecord between two kernels of a stream costs ~6 us of gap (tools/b1_timeline.sh), which only matters
// where the chain of kernels IS the latency of a call.  (A launch the profiler brackets is followed by a plain record.)
template <class... KArgs>
static int launch_done(orbx_handle* h, int profId, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t done,
                       typename as_declared<KArgs>::type... args)
{
    h->prof.begin(profId, s);
    if (done && !h->prof.cur) hipExtLaunchKernelGGL(kernel, grid, block, lds, s, nullptr, done, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    h->prof.end(s);
    if (done && h->prof.cur) HIPCHK(hipEventRecord(done, s));
    return ORBX_OK;
}

// kernel launches of one (sub-)batch: frames [f0, f0 + nb) of `src`
struct Launcher {
    orbx_handle* h;
    FrameSrc src;   // src.f0 = first frame
    int nb;
    void fast(hipStream_t fs, int cell0, int ncells) const
    {
        if (ncells <= 0) return;
        const Geom& g = h->geom;
        const bool l0 = cell0 == 0 && ncells == g.lv[0].nCells;  // the level-0 launch has its own, smaller LDS footprint
        const int rows = l0 ? h->tileRows0 : h->tileRows, cap = l0 ? h->fastListCap0 : h->fastListCap;
        const int sp = l0 ? h->fastSmapPitch0 : h->fastSmapPitch;
        const size_t lds = fast_lds_bytes(rows, h->tileStrideDw, sp, cap);
        h->prof.begin(P_FAST, fs);
        if (h->tileStrideDw == 12)
            hipLaunchKernelGGL(k_fast<48>, dim3(ncells, xcd_grid_y(nb)), dim3(64), lds, fs, h->d_geom, h->d_cells, src, h->d_candRaw,
                               h->d_cellCount, h->d_errCur, rows, cap, sp, nb, cell0);
        else
            hipLaunchKernelGGL(k_fast<80>, dim3(ncells, xcd_grid_y(nb)), dim3(64), lds, fs, h->d_geom, h->d_cells, src, h->d_candRaw,
                               h->d_cellCount, h->d_errCur, rows, cap, sp, nb, cell0);
        h->prof.end(fs);
    }
    void dist(hipStream_t ds, int l0, int nl) const  // quadtree of levels [l0, l0 + nl)
    {
        if (nl <= 0) return;
        const Geom& g = h->geom;
        h->prof.begin(P_DISTRIBUTE, ds);
        const size_t dl = dist_lds_bytes(h->nodeCap, g.maxCellsPerLevel);
        DistArgs da{h->d_geom, h->d_candRaw, h->d_candA, h->d_candB, h->d_cells, h->d_cellCount, h->d_candCount, h->d_kept, h->d_keptCount,
                    h->d_errCur, h->nodeCap, src.f0, nullptr, 0, l0, 0};
        // a frame's eight levels on the XCD that ran the frame's FAST cells and will run its descriptors (the plain (level, frame)
        // grid puts LEVEL l on XCD l)
        if (h->distInLds) {
            da.xcdFrames = xcd_frames(nb);
            hipLaunchKernelGGL(k_distribute<true>, dim3(nl, xcd_grid_y(nb)), dim3(kDistThreads), dl, ds, da);
        } else {
            da.gscratch = h->d_distScratch + (size_t)src.f0 * g.nlevels * (dl / 4); da.scratchWords = (int)(dl / 4);
            hipLaunchKernelGGL(k_distribute<false>, dim3(nl, nb), dim3(kDistThreads), 0, ds, da);
        }
        h->prof.end(ds);
    }
    int pyramid(hipStream_t s, hipEvent_t done = nullptr) const
    {
        const Geom& g = h->geom;
        if (g.nlevels > 1 && h->pyrFused) {
            // a frame's blocks on ONE XCD (neighbouring blocks read the same level-0 rows and columns for their halos; FAST, blur and
            // descriptors of the frame run there too; the plain (block, frame) grid put block b of every frame on XCD b mod 8)
            return launch_done(h, P_RESIZE, k_pyramid, dim3(h->pyrBlocks, xcd_grid_y(nb)), dim3(kPyrThreads), pyr_lds_bytes(h->pyrBufA, h->pyrBufB, h->pyrTabCap), s, done,
                               h->d_geom, src, h->tabs, h->d_pyrRanges, h->pyrBufA, h->pyrBufB, h->pyrTabCap, xcd_frames(nb));
        }
        for (int l = 1; l < g.nlevels; l++) {
            h->prof.begin(P_RESIZE, s);
            hipLaunchKernelGGL(k_resize_level, dim3((g.lv[l].w + 255) / 256, (g.lv[l].h + 3) / 4, nb), dim3(64, 4, 1), 0, s,
                               h->d_geom, src, h->tabs, l);
            h->prof.end(s);
        }
        if (done) HIPCHK(hipEventRecord(done, s));
        return ORBX_OK;
    }
    // latency mode, one queue: quadtree (all levels) and Gaussian in one launch (k_distribute_blur); false = not available here
    bool dist_blur(hipStream_t s) const
    {
        const Geom& g = h->geom;
        if (!h->distInLds || !h->distBlurOk || h->prof.cur || src.f0 != 0) return false;
        const size_t dl = dist_lds_bytes(h->nodeCap, g.maxCellsPerLevel);
        const int nTiles = h->blurTiles.base[g.nlevels];
        DistArgs da{h->d_geom, h->d_candRaw, h->d_candA, h->d_candB, h->d_cells, h->d_cellCount, h->d_candCount, h->d_kept, h->d_keptCount,
                    h->d_errCur, h->nodeCap, src.f0, nullptr, 0, 0};
        hipLaunchKernelGGL(k_distribute_blur, dim3(g.nlevels + (nTiles + 1) / 2, nb), dim3(kDistThreads), dl, s, da, src, h->blurTiles, nTiles);
        return true;
    }
    // the column walk; lat = a call of up to latMaxB frames (the latency chain, and the small calls that take the throughput
    // loop: one level, ORBX_SERIAL) keeps the one-tile kernel: a frame or two want many short workgroups
    void blur(hipStream_t s, bool lat = false) const
    {
        h->prof.begin(P_BLUR, s);
        if (lat) hipLaunchKernelGGL(k_blur_mfma, dim3(h->blurTiles.base[h->geom.nlevels], xcd_grid_y(nb)), dim3(256), 0, s, h->d_geom, src, h->blurTiles, nb);
        else hipLaunchKernelGGL(k_blur_walk, dim3(h->blurRuns.base[h->geom.nlevels], xcd_grid_y(nb)), dim3(256), 0, s, h->d_geom, src, h->blurRuns, nb);
        h->prof.end(s);
    }
    // The output slots of `set` were read by the matching two batches back and by its download (host path); a wait is
    // only enqueued when that work sits on another stream (every cross-stream wait costs microseconds of latency).
    // lat as for blur: such a call keeps four keypoints per wave on 256 threads, every other one runs eight on 128
    int desc(hipStream_t s, int set, hipEvent_t done = nullptr, bool lat = false) const
    {
        if (h->matchPending[set] && h->matchStream[set] != s) HIPCHK(hipStreamWaitEvent(s, h->evMatch[set], 0));
        if (h->evOutOfSet[set] && h->outStream[set] != s) HIPCHK(hipStreamWaitEvent(s, h->evOutOfSet[set], 0));
        for (hipEvent_t e : h->evExtReader[set]) HIPCHK(hipStreamWaitEvent(s, e, 0));
        h->evExtReader[set].clear();  // this stream is behind them now, and it is the only writer of the set
        // the +-1 form of the descriptors for the matrix-core scan, slot f + 1 of the set (frames src.f0 ..)
        uint8_t* const xOut = h->fuseExpand ? r_xdesc(h, set) + (size_t)h->xPitch : nullptr;   // (the kernel adds frame * xPitch, like frame * maxKp for the others)
        return launch_done(h, P_ORIENT_DESC, lat ? k_orient_desc<4> : k_orient_desc<8>, dim3(h->kpBlocksTotal, xcd_grid_y(nb)), dim3(kKpPerBlock / (lat ? 4 : 8) * 64), 0, s, done, h->d_geom, src,
                           h->kpBlocks, h->d_kept, h->d_keptCount, r_kps(h, set) + h->maxKp, r_desc(h, set) + (size_t)h->maxKp * 32, r_count(h, set) + 1, nb, xOut, h->xPitch, h->xAngOff);
    }
};

// ------------------------------------------------------------------ how a call is cut
// Frames [f0, f1) of sub-batch `part` of a call of B frames.  The host path uploads a batch in exactly the parts run_extract
// runs it in (an event behind each): both take the mode and the ranges from here.
struct FrameRange { int f0, f1; };
static inline FrameRange part_range(int B, int part, int nparts) { return {(int)((int64_t)B * part / nparts), (int)((int64_t)B * (part + 1) / nparts)}; }
// lat: the call runs as one latency-mode chain (up to latMaxB frames, not with ORBX_SERIAL); parts: its sub-batches otherwise
struct CallMode { bool lat; int parts; };
static inline CallMode call_mode(const orbx_handle* h, int B)
{
    const bool lat = B <= h->latMaxB && !h->serial;
    return {lat, lat || h->serial ? 1 : std::min(h->nsplit, B)};
}

// Two event graphs.
// THROUGHPUT (B > 2): the batch is cut into sub-batches that run on separate stream groups: the latency-bound kernels
// of one sub-batch (quadtree, descriptors) overlap the throughput-bound ones (FAST, matching) of the other.  Level-0
// FAST runs beside the pyramid on the blur stream; the quadtree of all levels follows FAST on the sub-batch's stream.
// (Moving the level-0 quadtree ahead -- right behind the level-0 FAST, or behind the blur -- was measured at 64 frames
// per step: 128.3 k -> 118.8 k and 111.2 k frames/s, two A/B rounds each: on the blur stream it delays the blur and
// with it the descriptors.  It stays where it was.)
// LATENCY (one or two frames, the per-frame drop-in entry): nothing else keeps the GPU busy, the chain IS the call.
//   main (streamP[0]):  [frames arrive here on the host path] pyramid -> FAST 1.. -> quadtree 1.. -> descriptors
//   aux  (stream):      FAST 0 -> quadtree 0 -> blur
// one cross-stream wait in front of the descriptors; the level-0 quadtree (as long as levels 1.. together: one
// workgroup per level) runs beside pyramid + FAST instead of behind them.
// sIn = the stream on which the frames become available (nullptr: the host-facing stream, where the device-resident
// entry has always taken them from).
static int run_extract(orbx_handle* h, const uint8_t* d_imgs, int B, int w, int hh, int stride, size_t pitch,
                       const hipEvent_t* evUploaded = nullptr, hipStream_t sIn = nullptr, bool lazyDone = false)
{
    int rc = flush_pack(h);   // (a result kernel nobody took along: in front of the kernels that overwrite what it reads)
    if (rc) return rc;
    if ((rc = configure_shape(h, w, hh))) return rc;
    if (B < 1 || B > h->maxB) return fail(ORBX_E_INVALID, "batch %d outside [1,%d]", B, h->maxB);
    if (((uintptr_t)d_imgs & 3) || (stride & 3) || (pitch & 3) || stride < w)
        return fail(ORBX_E_INVALID, "device frames need 4-byte aligned base/stride/pitch and stride >= width");
    const Geom& g = h->geom;
    FrameSrc src;
    src.img0 = d_imgs; src.stride0 = stride; src.pitch0 = (int64_t)pitch;
    src.pyr = h->d_pyr; src.blur = h->d_blur; src.f0 = 0;
    // the pyramid/blur buffers use the geometry's per-frame sizes as pitch
    hipStream_t s0 = h->stream;
    if (!sIn) sIn = s0;
    const int nsplit = call_mode(h, B).parts;
    // The latency chain wants a pyramid to run level 0 beside: with ONE level a latency-mode call takes the throughput loop below,
    // its one part on streamP[0].  The host path does not look at the levels: it has sent the frames up on sIn = streamP[0]
    // without an upload event, and that loop then orders them by evStart, recorded on sIn, as it does for every such sIn.
    const bool lat = call_mode(h, B).lat && g.nlevels > 1;
    // Sub-batch p owns stream streamP[p] across calls: it follows its own previous work (its frames' scratch
    // buffers) and the upload, nothing else -- the next batch's pyramid of sub-batch 0 starts while this batch's
    // sub-batch 1 is still in its quadtree.  Consumers join through evPart (join_parts).
    // evFrames = "the frames are there", for the streams that did not carry them: the upload's own event (host path,
    // throughput mode: the frames arrive on a copy stream) or one recorded behind the upload on the stream that did
    // (latency mode).  A device-resident call has nothing to announce (the caller's frames are complete, every hazard
    // on the scratch buffers is ordered by the sub-batch chains below).  Never an event recorded on the host-facing
    // stream: it would sit behind the previous step's blur, and the next pyramid would wait for a kernel it does not
    // depend on.
    const bool devCall = !evUploaded && sIn == s0;
    // frames, kernels, results in ONE queue -- stream order is all the ordering there is, no event anywhere in the chain --
    // or (ORBX_LAT_STREAMS=2) level 0 beside the pyramid on a second one.  Until the frames went up through a copy kernel
    // the two-queue form was 8-12 us faster for a robot alone on the GPU; since then the chain starts the instant the
    // upload ends and one queue wins there as well (0.195 against 0.200-0.203 ms per frame), as it always did with several
    // robots (the GPU runs about four queues at a time: 16.2 k against 8.6 k frames/s with four).
    const int latStreams = h->latStreams ? h->latStreams : 1;
    const bool oneStream = lat && latStreams == 1 && sIn == h->streamP[0];
    hipEvent_t evFrames = nullptr;
    if (!evUploaded && !h->serial && !devCall && !oneStream) {   // (evUploaded: per sub-batch, below)
        HIPCHK(hipEventRecord(h->evStart, sIn));
        evFrames = h->evStart;
    }
    // A frame's scratch (pyramid and blur levels, candidate segments, kept records) is ordered between two calls by
    // the stream of the sub-batch that owns the frame.  When the batch size -- and with it the frame -> sub-batch
    // map -- changes between two calls that the caller did not separate by a sync, a frame can change hands: its new
    // owner's pyramid would overwrite what the old owner's descriptor kernel may still be reading.  On such a call
    // (never in a steady stream) every stream first joins all sub-batches of the previous call.
    if (!h->serial && h->lastParts > 0 && (B != h->prevB || nsplit != h->prevSplit)) {
        if ((rc = flush_part_event(h))) return rc;
        for (int p = 0; p < h->lastParts; p++) {
            HIPCHK(hipStreamWaitEvent(s0, h->evPart[p], 0));
            for (int q = 0; q < nsplit; q++) HIPCHK(hipStreamWaitEvent(h->streamP[q], h->evPart[p], 0));
        }
    }
    h->prevB = B; h->prevSplit = nsplit;
    h->lastParts = 0;
    h->curSet ^= 1;
    const int set = h->curSet;
    const int cellsL0 = g.lv[0].nCells;
    h->lastLat = lat;
    if (lat) {
        hipStream_t sm = h->streamP[0], sa = s0;
        Launcher L{h, src, B};
        if (oneStream) {
            // (a handle that ran the two-stream chain before would have to join `s0` here; the mode is fixed at create)
            // (hipExtAnyOrderLaunch -- a packet without the barrier bit, so that level-0 FAST would run beside the pyramid and the
            // blur beside the quadtree in this one queue -- is ignored on gfx9: tried, the trace shows the kernels one after the other)
            if ((rc = L.pyramid(sm))) return rc;
            L.fast(sm, 0, g.totalCells);   // every level in one launch (two, level 0 apart, where level 0 can run ahead of the pyramid)
            if (!L.dist_blur(sm)) {
                L.dist(sm, 0, g.nlevels);
                L.blur(sm, true);
            }
        } else {
            if (evFrames && sIn != sm) HIPCHK(hipStreamWaitEvent(sm, evFrames, 0));
            if (evFrames && sIn != sa) HIPCHK(hipStreamWaitEvent(sa, evFrames, 0));
            // aux: level 0 needs no pyramid.  (The previous call's quadtree and descriptors, which read what these two
            // overwrite, ran on `sm` in front of the upload / evStart that `sa` has just been made to follow.)
            if (sIn == sa && h->partEverRan[0]) { if ((rc = flush_part_event(h))) return rc; HIPCHK(hipStreamWaitEvent(sa, h->evPart[0], 0)); }
            L.fast(sa, 0, cellsL0);
            L.dist(sa, 0, 1);
            if ((rc = L.pyramid(sm, h->evPyr[0]))) return rc;
            L.fast(sm, cellsL0, g.totalCells - cellsL0);
            L.dist(sm, 1, g.nlevels - 1);
            HIPCHK(hipStreamWaitEvent(sa, h->evPyr[0], 0));
            L.blur(sa, true);
            HIPCHK(hipEventRecord(h->evFast0[0], sa));  // the aux chain is through
            HIPCHK(hipStreamWaitEvent(sm, h->evFast0[0], 0));
        }
        if ((rc = L.desc(sm, set, lazyDone ? nullptr : h->evPart[0], true))) return rc;
        h->lastParts = 1; h->partLazy = lazyDone; h->partEverRan[0] = true;
    } else {
        for (int part = 0; part < nsplit; part++) {
            const FrameRange fr = part_range(B, part, nsplit);
            const int f0 = fr.f0, nb = fr.f1 - fr.f0;
            if (nb <= 0) continue;
            hipStream_t s = h->serial ? s0 : h->streamP[part];
            hipStream_t s2 = h->serial ? s : s0;  // blur: see orbx_create on the choice of streams
            if (evUploaded) {  // host path, throughput mode: this sub-batch's frames arrive on a copy stream
                HIPCHK(hipStreamWaitEvent(s, evUploaded[part], 0));
                if (s2 != s) HIPCHK(hipStreamWaitEvent(s2, evUploaded[part], 0));
            }
            if (evFrames && !h->serial) HIPCHK(hipStreamWaitEvent(s, evFrames, 0));
            if (evFrames && !h->serial && sIn != s0 && part == 0) HIPCHK(hipStreamWaitEvent(s0, evFrames, 0));
            src.f0 = f0;
            Launcher L{h, src, nb};
            // FAST of level 0 needs no pyramid: on the blur stream it runs beside the (latency-bound) pyramid kernel.
            // It overwrites this sub-batch's candidate segments, which the previous batch's quadtree read.
            const bool splitFast = !h->serial && g.nlevels > 1;
            if (splitFast) {
                if (h->partEverRan[part]) HIPCHK(hipStreamWaitEvent(s2, h->evPart[part], 0));
                L.fast(s2, 0, cellsL0);
                HIPCHK(hipEventRecord(h->evFast0[part], s2));
            } else {
                L.fast(s, 0, cellsL0);
            }
            if ((rc = L.pyramid(s))) return rc;
            // blur only needs the pyramid: run it on a second stream beside FAST + quadtree
            HIPCHK(hipEventRecord(h->evPyr[part], s));
            HIPCHK(hipStreamWaitEvent(s2, h->evPyr[part], 0));
            L.blur(s2, B <= h->latMaxB);
            HIPCHK(hipEventRecord(h->evBlur[part], s2));
            // FAST of levels >= 1 behind the pyramid (level 0 went ahead, see above)
            L.fast(s, cellsL0, g.totalCells - cellsL0);
            if (splitFast) HIPCHK(hipStreamWaitEvent(s, h->evFast0[part], 0));
            L.dist(s, 0, g.nlevels);
            HIPCHK(hipStreamWaitEvent(s, h->evBlur[part], 0));
            if ((rc = L.desc(s, set, nullptr, B <= h->latMaxB))) return rc;
            HIPCHK(hipEventRecord(h->evPart[h->lastParts++], s));
            h->partEverRan[part] = true;
        }
    }
    HIPCHK(hipGetLastError());
    h->lastB = B;
    src.f0 = 0;
    h->lastSrc = src;
    return ORBX_OK;
}

extern "C" int orbx_extract_batch_device(orbx_t* h, const uint8_t* d_imgs, int B, int w, int hh, int stride, size_t pitch)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (!d_imgs || w < 1 || hh < 1) return fail(ORBX_E_INVALID, "empty device frame");
    return run_extract(h, d_imgs, B, w, hh, stride, pitch);
}

extern "C" int orbx_device_results(orbx_t* h, OrbxKeyPoint** d_kps, uint8_t** d_desc, int32_t** d_counts, int* cap)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (d_kps) *d_kps = (OrbxKeyPoint*)(r_kps(h, h->curSet) + h->maxKp);
    if (d_desc) *d_desc = r_desc(h, h->curSet) + (size_t)h->maxKp * 32;
    if (d_counts) *d_counts = r_count(h, h->curSet) + 1;
    if (cap) *cap = h->maxKp;
    return ORBX_OK;
}

extern "C" int orbx_sync(orbx_t* h)
{
    int rc = check_device(h);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
#ifdef ORBX_FAST_STATS
    {
        unsigned long long st[16];
        if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_fastStats), sizeof st) == hipSuccess && st[0])
            fprintf(stderr, "FAST stats (one cell in 64): pass0 cells %llu visits %llu corners %llu | pass1 cells %llu visits %llu corners %llu | detection px %llu | "
                            "10 ns ticks: tile load %llu, stage 1 %llu, stage 2 %llu, stage 3 %llu\n",
                    st[0], st[1], st[2], st[4], st[5], st[6], st[8], st[9], st[10], st[11], st[12]);
    }
#endif
    int32_t err = 0;
    HIPCHK(hipMemcpy(&err, h->d_err, sizeof err, hipMemcpyDeviceToHost));
    if (err) {
        (void)hipMemset(h->d_err, 0, sizeof err);
        return fail(ORBX_E_CAPACITY, "device scratch overflow (flags 0x%x)", err);
    }
    return ORBX_OK;
}

extern "C" int orbx_device_alloc(orbx_t* h, size_t bytes, void** d_ptr)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (!d_ptr || bytes == 0) return fail(ORBX_E_INVALID, "bad argument");
    HIPCHK(hipMalloc(d_ptr, bytes));
    return ORBX_OK;
}

extern "C" int orbx_device_free(orbx_t* h, void* d_ptr)
{
    int rc = check_device(h);
    if (rc) return rc;
    if ((rc = sync_all(h))) return rc;
    if (d_ptr) HIPCHK(hipFree(d_ptr));
    return ORBX_OK;
}

extern "C" int orbx_upload(orbx_t* h, void* d_dst, const void* h_src, size_t bytes)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (!d_dst || !h_src) return fail(ORBX_E_INVALID, "null argument");
    HIPCHK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return ORBX_OK;
}

extern "C" int orbx_download(orbx_t* h, int frame, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out)
{
    int rc = orbx_sync(h);
    if (rc) return rc;
    if (frame < 0 || frame >= h->lastB) return fail(ORBX_E_INVALID, "frame %d not in the last batch", frame);
    int32_t n = 0;
    HIPCHK(hipMemcpy(&n, r_count(h, h->curSet) + 1 + frame, sizeof n, hipMemcpyDeviceToHost));
    if (n_out) *n_out = n;
    if (n > cap) return fail(ORBX_E_CAPACITY, "%d keypoints, caller capacity %d", n, cap);
    if (n > 0) {
        if (kps) HIPCHK(hipMemcpy(kps, r_kps(h, h->curSet) + (size_t)(frame + 1) * h->maxKp, (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyDeviceToHost));
        if (desc) HIPCHK(hipMemcpy(desc, r_desc(h, h->curSet) + (size_t)(frame + 1) * h->maxKp * 32, (size_t)n * 32, hipMemcpyDeviceToHost));
    }
    return ORBX_OK;
}
