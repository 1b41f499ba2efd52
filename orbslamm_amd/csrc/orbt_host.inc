// orbt_host.inc -- host side of the Tracking-shaped searches (k_frame_build, k_proj_candidates, k_proj_resolve and their
// frame-set forms); part of orbslamm_hip.hip.
//
// One call = one packed upload (pinned staging), two or three launches, one download, one host sync: no allocation, no
// count -> sync -> reserve in the middle (round 2's proj_core: ~10 pageable copies, two syncs, a serial resolve).
// The frame-set entries keep B frames and the results of B searches in HBM and make no host sync at all.

// ------------------------------------------------------------------ staging
static int orbm_pinned(orbm_handle* h, size_t bytes) { return grow_pinned(h->h_stage, h->h_stageCap, bytes, true, nullptr, &h->nHostAlloc); }

// The two ends of a drop-in call (host arrays in, host arrays out) ride on the call's own compute queue: the staging
// block goes up and the results come down through orbx::k_upload, a one-lane kernel raises a flag behind them and the
// host polls it.  A DMA engine's completion reaches the compute queue ~20 us after the copy's end, the compute queue's
// reaches the engine as late, and hipStreamSynchronize wakes the caller 20-50 us after the last packet
// (tools/live_dma_gap.sh, tools/live_timeline.sh).  Only blocks whose size is no multiple of 16 take the engine.
static int stage_up(orbm_handle* h, hipStream_t s, void* dev, const void* host, size_t bytes)
{
    if (bytes & 15) { HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s)); return ORBX_OK; }
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((bytes / 16 + 255) / 256)), dim3(256), 0, s, (const uint4*)host, (uint4*)dev, (int)(bytes / 16));
    return ORBX_OK;
}

static int stage_down_wait(orbm_handle* h, hipStream_t s, void* host, const void* dev, size_t bytes)
{
    if (bytes & 15) {
        HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return ORBX_OK;
    }
    volatile int32_t* flag = (volatile int32_t*)((uint8_t*)h->h_stage + h->h_stageCap);
    const int32_t want = ++h->stageSeq;
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((bytes / 16 + 255) / 256)), dim3(256), 0, s, (const uint4*)dev, (uint4*)host, (int)(bytes / 16));
    hipLaunchKernelGGL(k_raise_flag, dim3(1), dim3(64), 0, s, (int32_t*)flag, want);   // (behind the copy kernel's end-of-kernel release)
    HIPCHK(hipGetLastError());
    if (!wait_flag(flag, want)) HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

constexpr int kProjMaxTrain = 8192;      // the LDS form: resolve 12 bytes per train feature (+ queries, candidates); candidates 16 bytes
constexpr int kProjMaxCells = 16383;     // the LDS form: cell starts as uint16
constexpr int kProjMaxTrainBig = 65535;  // beyond the LDS form (ProjCommon::big): a candidate entry holds the train index in 16 bits
constexpr size_t kProjLdsBudget = 160 * 1024 - 512;  // the kernels' static LDS is ~300 bytes
constexpr size_t kProjQueryBytes = 17;  // resolve LDS per query
constexpr int kTrackFlagPairs = 8;       // orbm_track_frames with at most this many pairs publishes through flags

// Few pairs (a live stream, a drop-in call): sixteen lanes per query instead of four -- the walk of a window costs a wave its
// longest lane, and a single pair's 17 workgroups leave the GPU empty anyway: k_track_candidates 26 -> 13 us for one pair of
// 2000-feature frames.  Many pairs: four (each workgroup stages the train frame's grid, 38 KB; workgroups abound).
static int cand_lanes(int npairs)
{
    return npairs <= 4 ? orbt::kCandLanesWide : orbt::kCandLanes;
}

// LDS split of the two kernels of a projection search
struct ProjPlan { orbt::ProjCommon c; size_t ldsCand, ldsResolve; };
static int proj_lds_plan(int nt, int nq, int ncell, ProjPlan& pl, int stagePerQuery = 48)
{
    if (nt > kProjMaxTrainBig || nq > orbt::kMaxQueryIters * orbt::kThreads)
        return fail(ORBX_E_UNSUPPORTED, "%d train features, %d queries: a candidate entry holds the train index, a post the query index, in 16 bits (at most %d / %d)",
                    nt, nq, kProjMaxTrainBig, orbt::kMaxQueryIters * orbt::kThreads);
    orbt::ProjCommon& c = pl.c;
    c.tCap = std::max(64, align_up(nt, 64));
    c.cellCap = align_up(ncell + 1, 2);
    // candidates per query of a slice before the distance cut that fit the LDS staging list (a longer slice takes the
    // unstaged path: same lists, but the arena chunk is sized before the cut and the resolve may not fit LDS)
    c.stageCap = orbt::kCandQueries * stagePerQuery;
    c.lanes = orbt::kCandLanes;
    c.waveTail = true;   // the last rounds of the resolve run on the first wave alone
    const size_t candFixed = (size_t)c.tCap * 16 + (size_t)c.cellCap * 2;
    if (nt > kProjMaxTrain || ncell > kProjMaxCells || candFixed > kProjLdsBudget) {
        // the frame's grid does not fit a CU's LDS: the walk reads it from memory, the resolve keeps every table in memory
        // (ProjPair::tscr, qscr) -- the same lists and rounds, slower; the reference's loops take any size
        c.big = 1;
        c.stageCap = (int)std::min<size_t>((size_t)c.stageCap, kProjLdsBudget / 8) & ~3;
        pl.ldsCand = (size_t)c.stageCap * 8;
        c.qCap = 0; c.ldsCand = 0; pl.ldsResolve = 0;
        return ORBX_OK;
    }
    // a staging list that does not fit shrinks (down to none: the slices then list straight into the arena, unfiltered)
    c.stageCap = (int)std::min<size_t>((size_t)c.stageCap, (kProjLdsBudget - candFixed) / 8) & ~3;
    pl.ldsCand = candFixed + (size_t)c.stageCap * 8;
    // resolve: the per-train tables (12 bytes each) are always in LDS; the per-query tables (17 bytes: offset, best, second = result, state, two pending-list slots) and the candidate
    // lists (10 bytes: entry, query, two live-list slots) only while they fit -- otherwise the rounds run from memory
    const size_t trainBytes = (size_t)c.tCap * 12;   // <= 96 KB at kProjMaxTrain
    c.qCap = std::min(std::max(64, align_up(nq, 64)), 4096);
    const size_t minCand = 4096 * 10;                // below this many LDS candidates the LDS rounds are not worth their tables
    if (trainBytes + (size_t)c.qCap * kProjQueryBytes + minCand > kProjLdsBudget) {
        const size_t room = kProjLdsBudget > trainBytes + minCand ? kProjLdsBudget - trainBytes - minCand : 0;
        c.qCap = (int)(room / kProjQueryBytes) & ~63;
    }
    if (c.qCap < 64) { c.qCap = 0; c.ldsCand = 0; pl.ldsResolve = trainBytes; return ORBX_OK; }
    const size_t fixed = trainBytes + (size_t)c.qCap * kProjQueryBytes;
    // what a search with th = 30 lists (~8 per train feature), not the whole CU
    c.ldsCand = (int)std::min<size_t>((kProjLdsBudget - fixed) / 10, (size_t)c.tCap * 8) & ~3;
    pl.ldsResolve = fixed + (size_t)c.ldsCand * 10;
    return ORBX_OK;
}

// ... and the rest of the plan for a search over explicit query arrays (a pool's projection, host-listed queries): no scale table,
// and the queries come in no particular order
static void proj_plan_queries(orbt::ProjCommon& c, int npairs)
{
    c.scale = nullptr; c.nlevels = 1;
    c.interleave = 0;
    if (!c.big) c.lanes = cand_lanes(npairs);
}

static int lds_attr(const void* fn, size_t bytes, size_t& have)
{
    if (bytes > 64 * 1024 && bytes > have) {
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kProjLdsBudget));
        have = kProjLdsBudget;
    }
    return ORBX_OK;
}

// Frame::Frame's tail for frames whose grid does not fit one workgroup's LDS (more than ~8 K features, or a very fine grid): the
// same products -- mvKeysUn, angles, descriptors, mGrid as CSR in push_back order, the grid-ordered records -- from the
// general-size kernels (orbm::k_undistort, k_grid_count / _fill / _sort, k_grid_records), frame by frame.  The feature counts
// are read back first when they live on the device: a slow path for sizes the reference's loops take and no shipped
// configuration has (SingleRobotScenario/src/Frame.cc:196-245 has no bound).
static int frame_build_big(orbm_handle* h, const orbt::FrameBuildArgs& fa, int nframes, hipStream_t s)
{
    int rc;
    const int ncell = fa.fs.ncell;
    std::vector<int32_t> counts((size_t)nframes, fa.srcN);
    if (fa.srcCount) {
        HIPCHK(hipMemcpyAsync(counts.data(), fa.srcCount, (size_t)nframes * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if ((rc = orbm_reserve(h, G_CNT, (size_t)ncell * 4)) || (rc = orbm_reserve(h, G_FILL, (size_t)ncell * 4))) return rc;
    const OrbmGrid grid = {fa.grid.minX, fa.grid.minY, fa.grid.invW, fa.grid.invH, fa.grid.cols, fa.grid.rows};
    const orbm::UndistArgs und = fa.und;
    for (int src = 0; src < nframes; src++) {
        const int slot = (fa.slot0 + src) % fa.slotMod;
        const int n = std::min(counts[(size_t)src], fa.fs.cap);
        const orbm::KeyDev* sk = fa.srcKeys + (int64_t)src * fa.srcCap;
        orbm::KeyDev* dk = fa.fs.keysUn + (int64_t)slot * fa.fs.cap;
        int32_t* cs = fa.fs.cellStart + (int64_t)slot * (ncell + 1);
        int32_t* ci = fa.fs.cellIdx + (int64_t)slot * fa.fs.cap;
        if (n) {
            if (fa.undistort) hipLaunchKernelGGL(orbm::k_undistort, dim3((n + 255) / 256), dim3(256), 0, s, sk, n, und, dk);
            else HIPCHK(hipMemcpyAsync(dk, sk, (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(fa.fs.desc + (int64_t)slot * fa.fs.cap * 32, fa.srcDesc + (int64_t)src * fa.srcCap * 32, (size_t)n * 32, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpy2DAsync(fa.fs.ang + (int64_t)slot * fa.fs.cap, 4, (const uint8_t*)sk + 12, sizeof(OrbxKeyPoint), 4, (size_t)n, hipMemcpyDeviceToDevice, s));
        }
        orbm::GridDev gd;
        if ((rc = grid_build_device(&grid, dk, n, slot_ptr<int32_t>(h, G_CNT), cs, slot_ptr<int32_t>(h, G_FILL), ci, s, gd))) return rc;
        if (n) hipLaunchKernelGGL(orbm::k_grid_records, dim3((n + 255) / 256), dim3(256), 0, s, (const orbm::KeyDev*)dk, (const int32_t*)cs, ncell, (const int32_t*)ci,
                                  fa.fs.rec + (int64_t)slot * fa.fs.cap);
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(fa.fs.n + slot), n, 1, s));
    }
    HIPCHK(hipGetLastError());
    // the count / fill scratch is the HANDLE's (G_CNT, G_FILL): when the build rode on another stream (a frame set attached to
    // an extractor) it must be through before a later grid build on the handle's own stream may reuse them -- slow path anyway
    if (s != h->stream) HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

static inline bool frame_build_fits_lds(int cap, int ncell) { return (size_t)ncell * 8 + (size_t)align_up(cap, 2) * 14 <= kProjLdsBudget && cap <= 65535; }

static int frame_build_launch(orbm_handle* h, const orbt::FrameBuildArgs& fa, int nframes, hipStream_t stream = nullptr)
{
    if (!stream) stream = h->stream;
    const size_t lds = (size_t)fa.fs.ncell * 8 + (size_t)align_up(fa.fs.cap, 2) * 14;
    if (!frame_build_fits_lds(fa.fs.cap, fa.fs.ncell)) return frame_build_big(h, fa, nframes, stream);
    int rc;
    if ((rc = lds_attr((const void*)orbt::k_frame_build, lds, h->ldsAttr[2]))) return rc;
    hipLaunchKernelGGL(orbt::k_frame_build, dim3(nframes), dim3(orbt::kThreads), lds, stream, fa);
    HIPCHK(hipGetLastError());
    return ORBX_OK;
}

static int proj_launch(orbm_handle* h, const orbt::ProjPair* d_pairs, int npairs, int nqMax, const ProjPlan& pl, hipStream_t stream = nullptr)
{
    int rc;
    if (!stream) stream = h->stream;
    if ((rc = lds_attr((const void*)orbt::k_proj_candidates, pl.ldsCand, h->ldsAttr[0])) ||
        (rc = lds_attr((const void*)orbt::k_proj_resolve, pl.ldsResolve, h->ldsAttr[1]))) return rc;
    const int perSlice = orbt::kCandThreads / pl.c.lanes;
    const int slices = (nqMax + perSlice - 1) / perSlice;
    if (slices) hipLaunchKernelGGL(orbt::k_proj_candidates, dim3(slices, npairs), dim3(orbt::kCandThreads), pl.ldsCand, stream, d_pairs, pl.c);
    hipLaunchKernelGGL(orbt::k_proj_resolve, dim3(npairs), dim3(orbt::kThreads), pl.ldsResolve, stream, d_pairs, pl.c);
    HIPCHK(hipGetLastError());
    return ORBX_OK;
}

// train side of a projection search, resident in HBM
struct ProjTrain {
    orbm::GridDev gd;
    const orbm::KeyDev* keys;
    const int32_t *cellStart, *cellIdx;
    const uint8_t* desc;
    int nt;
    const uint4* rec;   // grid-ordered records (orbt::FrameSetDev::rec)
};

// train side given as host arrays: keys + descriptors ride in the same staging block and k_frame_build makes the grid
struct ProjTrainHost { const OrbmGrid* grid; const OrbxKeyPoint* keys; const uint8_t* desc; };

// the scratch frame of a host-array train side (T_FS): keysUn | desc | ang | cellStart | cellIdx | rec | n
struct ScratchFrame { size_t fKeys, fDesc, fAng, fStart, fIdx, fRec, fN, bytes; };
static ScratchFrame scratch_frame_layout(int nt, int ncell)
{
    Packer fk;
    ScratchFrame f;
    f.fKeys = fk.take((size_t)nt * sizeof(OrbxKeyPoint)); f.fDesc = fk.take((size_t)nt * 32); f.fAng = fk.take((size_t)nt * 4);
    f.fStart = fk.take((size_t)(ncell + 1) * 4); f.fIdx = fk.take((size_t)nt * 4); f.fRec = fk.take((size_t)nt * 16); f.fN = fk.take(16);
    f.bytes = fk.off;
    return f;
}
static orbt::FrameSetDev scratch_frame_dev(uint8_t* fs, const ScratchFrame& f, int nt, int ncell)
{
    return {(orbm::KeyDev*)(fs + f.fKeys), fs + f.fDesc, (float*)(fs + f.fAng), (int32_t*)(fs + f.fStart), (int32_t*)(fs + f.fIdx), (uint4*)(fs + f.fRec), (int32_t*)(fs + f.fN), nt, ncell};
}
static inline bool same_grid(const OrbmGrid& a, const OrbmGrid& b)
{
    return a.minX == b.minX && a.minY == b.minY && a.invW == b.invW && a.invH == b.invH && a.cols == b.cols && a.rows == b.rows;
}

// The train side of the NEXT orbm_search_by_projection(_stereo) on this handle goes up NOW and its grid is built, asynchronously:
// a member of the drop-in class calls this first and walks its MapPoints (the reference's mutex-guarded getters: ~100 us for a
// frame's worth, ORBmatcher.cc:1355-1392) while the device works; the search then finds the frame resident and sends only the
// queries.  A hint, not a contract: the search compares the caller's pointers, count and grid with what was prepared and does
// its own upload when they differ.  The arrays must not change between the two calls.
extern "C" int orbm_projection_prepare(orbm_t* h, const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un, const uint8_t* tdesc, int nt)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    h->prep.valid = false;
    if (nt < 0 || (nt && (!t_keys_un || !tdesc))) return fail(ORBX_E_INVALID, "bad argument");
    if (nt == 0) return ORBX_OK;
    if (!grid || grid->cols < 1 || grid->rows < 1 || grid->cols * grid->rows > (1 << 20)) return fail(ORBX_E_INVALID, "bad grid");
    if (nt > kProjMaxTrainBig) return ORBX_OK;   // (the search will refuse it with its own message)
    hipStream_t s = h->stream;
    if (h->prep.inFlight) { HIPCHK(hipStreamSynchronize(s)); h->prep.inFlight = false; }   // a prepare nobody consumed: its upload may still read h_prep
    const int ncell = grid->cols * grid->rows;
    const ScratchFrame lay = scratch_frame_layout(nt, ncell);
    const size_t kb = ((size_t)nt * sizeof(OrbxKeyPoint) + 15) & ~(size_t)15, db = (size_t)nt * 32, up = kb + db;
    if ((rc = grow_pinned(h->h_prep, h->h_prepCap, up, false, nullptr, &h->nHostAlloc)) || (rc = orbm_reserve(h, T_FS, lay.bytes)) ||
        (rc = orbm_reserve(h, T_PREP, up)))
        return rc;
    uint8_t* hp = (uint8_t*)h->h_prep;
    uint8_t* dp = slot_ptr<uint8_t>(h, T_PREP);
    memcpy(hp, t_keys_un, (size_t)nt * sizeof(OrbxKeyPoint));
    memcpy(hp + kb, tdesc, db);
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((up / 16 + 255) / 256)), dim3(256), 0, s, (const uint4*)hp, (uint4*)dp, (int)(up / 16));
    orbt::FrameBuildArgs fa{};
    fa.fs = scratch_frame_dev(slot_ptr<uint8_t>(h, T_FS), lay, nt, ncell);
    fa.srcKeys = (const orbm::KeyDev*)dp; fa.srcDesc = dp + kb; fa.srcCount = nullptr; fa.srcCap = nt; fa.srcN = nt;
    fa.slot0 = 0; fa.slotMod = 1;
    fa.grid = {grid->minX, grid->minY, grid->invW, grid->invH, grid->cols, grid->rows};
    fa.undistort = 0;
    if ((rc = frame_build_launch(h, fa, 1))) return rc;
    h->prep.valid = true; h->prep.inFlight = true;
    h->prep.keys = t_keys_un; h->prep.desc = tdesc; h->prep.nt = nt; h->prep.grid = *grid; h->prep.seq = h->callSeq;
    return ORBX_OK;
}

static int proj_core(orbm_handle* h, const OrbmProjParams* pp, const float* q_uvr, const int8_t* q_lvl, const uint8_t* qdesc,
                     const float* qangle, const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq, const ProjTrain* trDev,
                     const ProjTrainHost* trHost, int nt, uint8_t* t_occ, int32_t* assign, int* nmatches,
                     const float* q_ur = nullptr, const float* t_uright = nullptr)
{
    int rc;
    const bool stereo = q_ur && t_uright;
    const OrbmGrid* g = trHost ? trHost->grid : nullptr;
    const int ncell = trHost ? g->cols * g->rows : trDev->gd.cols * trDev->gd.rows;
    ProjPlan pl{};
    if ((rc = proj_lds_plan(nt, nq, ncell, pl))) return rc;
    orbt::ProjCommon& c = pl.c;
    c.mode = pp->mode; c.nnratio = pp->nnratio; c.checkOri = pp->check_ori; c.thDist = pp->th_dist;
    proj_plan_queries(c, 1);

    Packer pk;
    const size_t oPair = pk.take(sizeof(orbt::ProjPair));
    const size_t oUvr = pk.take((size_t)nq * 12), oLvl = pk.take((size_t)nq * 2), oQd = pk.take((size_t)nq * 32);
    const size_t oQa = qangle ? pk.take((size_t)nq * 4) : 0, oQv = qvalid ? pk.take((size_t)nq) : 0, oQo = q_obs_pos ? pk.take((size_t)nq) : 0;
    const size_t oQur = stereo ? pk.take((size_t)nq * 4) : 0, oTur = stereo ? pk.take((size_t)nt * 4) : 0;
    // the train side may be resident already (orbm_projection_prepare with these very arrays): then only the queries go up
    // (good for the call that directly follows the prepare on this handle: anything in between, and the hint is void -- a buffer
    // address alone proves nothing about its contents a call later)
    const bool prepared = trHost && h->prep.valid && h->prep.seq + 1 == h->callSeq && h->prep.keys == trHost->keys && h->prep.desc == trHost->desc && h->prep.nt == nt && same_grid(h->prep.grid, *g);
    h->prep.valid = false;   // one search per prepare (the scratch frame is this call's to overwrite otherwise)
    const bool upTrain = trHost && !prepared;
    const size_t oTk = upTrain ? pk.take((size_t)nt * sizeof(OrbxKeyPoint)) : 0, oTd = upTrain ? pk.take((size_t)nt * 32) : 0;
    const size_t oAssign = pk.take((size_t)nt * 4), oOcc = pk.take((size_t)nt), oNm = pk.take(16);
    const size_t total = pk.off;
    const ScratchFrame lay = scratch_frame_layout(nt, ncell);
    const bool freshTotal = slot_cap(h, T_STATS) == 0;
    if ((rc = orbm_pinned(h, total)) || (rc = orbm_reserve(h, {{T_STAGE, total}, {T_OFF, (size_t)nq * 8}, {T_QRES, (size_t)nq * 16}, {T_STATS, 16},
                                                               {T_CAND, std::max<size_t>((size_t)nq * 64 * 8, 1 << 19)}})) ||
        (c.big && (rc = orbm_reserve(h, T_TSCR, (size_t)c.tCap * 12))) || (trHost && (rc = orbm_reserve(h, T_FS, lay.bytes)))) return rc;
    if (freshTotal) HIPCHK(hipMemsetAsync(slot_ptr(h, T_STATS), 0, 16, h->stream));  // the candidate counter: zero on entry, left zero by every resolve

    for (int attempt = 0; attempt < 2; attempt++) {
        uint8_t* hs = (uint8_t*)h->h_stage;
        uint8_t* ds = slot_ptr<uint8_t>(h, T_STAGE);
        hipStream_t s = h->stream;
        memcpy(hs + oUvr, q_uvr, (size_t)nq * 12); memcpy(hs + oLvl, q_lvl, (size_t)nq * 2); memcpy(hs + oQd, qdesc, (size_t)nq * 32);
        if (qangle) memcpy(hs + oQa, qangle, (size_t)nq * 4);
        if (qvalid) memcpy(hs + oQv, qvalid, (size_t)nq);
        if (q_obs_pos) memcpy(hs + oQo, q_obs_pos, (size_t)nq);
        if (stereo) { memcpy(hs + oQur, q_ur, (size_t)nq * 4); memcpy(hs + oTur, t_uright, (size_t)nt * 4); }
        if (upTrain) { memcpy(hs + oTk, trHost->keys, (size_t)nt * sizeof(OrbxKeyPoint)); memcpy(hs + oTd, trHost->desc, (size_t)nt * 32); }
        memcpy(hs + oAssign, assign, (size_t)nt * 4); memcpy(hs + oOcc, t_occ, (size_t)nt);
        orbt::ProjPair P{};
        ProjTrain tr;
        orbt::FrameBuildArgs fa{};
        if (trHost) {
            fa.fs = scratch_frame_dev(slot_ptr<uint8_t>(h, T_FS), lay, nt, ncell);
            fa.srcKeys = (const orbm::KeyDev*)(ds + oTk); fa.srcDesc = ds + oTd; fa.srcCount = nullptr; fa.srcCap = nt; fa.srcN = nt;
            fa.slot0 = 0; fa.slotMod = 1;
            fa.grid = {g->minX, g->minY, g->invW, g->invH, g->cols, g->rows};
            fa.undistort = 0;
            tr = {fa.grid, fa.fs.keysUn, fa.fs.cellStart, fa.fs.cellIdx, fa.fs.desc, nt, fa.fs.rec};
        } else {
            tr = *trDev;
        }
        P.grid = tr.gd; P.tkeys = tr.keys; P.cellStart = tr.cellStart; P.trec = tr.rec; P.tdesc = tr.desc;
        P.ntPtr = nullptr; P.nt = nt;
        P.quvr = (const float*)(ds + oUvr); P.qlvl = (const int8_t*)(ds + oLvl); P.qdesc = ds + oQd;
        P.qang = qangle ? (const float*)(ds + oQa) : nullptr;
        P.qvalid = qvalid ? ds + oQv : nullptr; P.qobs = q_obs_pos ? ds + oQo : nullptr;
        P.qur = stereo ? (const float*)(ds + oQur) : nullptr; P.turight = stereo ? (const float*)(ds + oTur) : nullptr;
        P.qkeys = nullptr; P.nqPtr = nullptr; P.nq = nq;
        P.toccIn = ds + oOcc; P.toccOut = ds + oOcc;
        P.assign = (int32_t*)(ds + oAssign); P.initAssign = 0;
        P.nmatch = (int32_t*)(ds + oNm);
        P.total = slot_ptr<int32_t>(h, T_STATS);
        P.candOff = slot_ptr<int32_t>(h, T_OFF); P.candCnt = P.candOff + nq; P.cand = slot_ptr<uint2>(h, T_CAND); P.candCap = (int)(slot_cap(h, T_CAND) / 8);
        P.qres = slot_ptr<int32_t>(h, T_QRES); P.qscr = P.qres + nq; P.stats = (int32_t*)(ds + oNm) + 1;
        P.tscr = c.big ? slot_ptr<int32_t>(h, T_TSCR) : nullptr;
        memcpy(hs + oPair, &P, sizeof P);
        if ((rc = stage_up(h, s, ds, hs, total))) return rc;
        if (upTrain && (rc = frame_build_launch(h, fa, 1))) return rc;   // (prepared: built already, ahead of this call on the same stream)
        if ((rc = proj_launch(h, (const orbt::ProjPair*)(ds + oPair), 1, nq, pl))) return rc;
        if ((rc = stage_down_wait(h, s, hs + oAssign, ds + oAssign, total - oAssign))) return rc;
        h->prep.inFlight = false;   // everything enqueued before this call's results has run
        const int32_t* tail = (const int32_t*)(hs + oNm);
        if (tail[0] < 0) {  // more candidates than the arena holds: grow it once, run again
            if (attempt) return fail(ORBX_E_CAPACITY, "candidate arena overflow");
            if ((rc = orbm_reserve(h, T_CAND, (size_t)(-tail[0]) * 8))) return rc;
            continue;
        }
        memcpy(assign, hs + oAssign, (size_t)nt * 4); memcpy(t_occ, hs + oOcc, (size_t)nt);
        if (nmatches) *nmatches = tail[0];
        h->lastRounds = tail[1]; h->lastCands = tail[2];
        return ORBX_OK;
    }
    return ORBX_OK;
}

// ------------------------------------------------------------------ frame set: the matcher-side state of B frames in HBM
// Frame::Frame's tail (Frame.cc:196-210) for a whole batch in ONE launch, straight from the extractor's device results
// (counts are read on the device: no host sync), and SearchByProjection(CurrentFrame, LastFrame) for a batch of frame
// pairs in ONE launch.  Results (assign tables, match counts) are written by the kernel into pinned host memory:
// "download" is a stream sync.
struct orbm_frameset_bow;
static void frameset_bow_free(struct orbm_frameset* fs);

// One result set of a frame set's searches: its completion event, pair count, the value its flags carry once raised (0: none
// are -- wait on the event), and the search that filled it, which orbm_track_results runs again when its candidates overflowed.
// A search takes next(), begin()s the set (it holds none) before it enqueues anything, writes its arguments and enqueues its
// launches and the event from them, and only then commit()s: a failed call leaves the previous search the newest.
struct ResultRecord {
    enum Kind { kNone, kFramePairs, kQueries };
    Kind kind = kNone;
    hipEvent_t ev = nullptr;
    int pairs = 0; int32_t flagValue = 0;
    OrbmProjParams pp{};
    uint32_t builds = 0;   // the frame set's build count when the search was issued: a slot stamped later has been rebuilt since
    // frame pairs: th and the slot pairs
    float th = 0;
    std::vector<int32_t> cur, last;
    // queries: train slot, query slot (-1: queries from the host); the set's staging block (its share of h_q, ProjPair first,
    // `total` bytes) as allocated at epoch qEpoch; the launch plan
    int slot = -1, qslot = -1, nq = 0;
    uint32_t qEpoch = 0;
    size_t total = 0;
    ProjPlan plan{};
    // queries made on the device from a map-point pool (orbw_host.inc): `total` covers the block's head alone (pair record |
    // occupancy), the query block behind it is the projection kernel's and stays as it left it -- a replay reads it again,
    // not the pool; the status bytes lie at oStatus of the set's pinned share
    bool fromPool = false;
    size_t oStatus = 0;
    // what orbq_track_pose (orbq_host.inc) needs to read the search's ids where they lie: the pool, the ids block's offset in
    // the set's pinned share, or the keyframe store whose S they are with the count of its updates at the issue; `accepted`: the
    // host has received the table through orbm_track_results with ORBX_OK
    const void* pool = nullptr; uint64_t poolSerial = 0;     // (the serial: an object made later at the same address is another)
    size_t oIds = 0;
    const void* store = nullptr; uint64_t storeSerial = 0;
    uint32_t storeUpdates = 0;
    bool accepted = false;
};
struct ResultRing {   // kSets result sets in rotation: a caller may read up to kSets - 1 calls behind the newest
    static constexpr int kSets = 4;
    ResultRecord rec[kSets];
    int newest = 0;
    int next() const { return (newest + 1) % kSets; }
    int back(int b) const { return (newest + kSets - b) % kSets; }
    int begin(int set)
    {
        rec[set].kind = ResultRecord::kNone; rec[set].pairs = 0; rec[set].flagValue = 0; rec[set].accepted = false;
        if (!rec[set].ev) HIPCHK(hipEventCreateWithFlags(&rec[set].ev, hipEventDisableTiming));
        return ORBX_OK;
    }
    void commit(int set, ResultRecord::Kind kind, int pairs, int32_t flagValue) { newest = set; rec[set].kind = kind; rec[set].pairs = pairs; rec[set].flagValue = flagValue; }
    void destroy() { for (auto& r : rec) if (r.ev) (void)hipEventDestroy(r.ev); }
};

struct orbm_frameset {
    orbm_frameset_bow* bow = nullptr;   // orbt_bow_host.inc: allocated by the first orbm_frameset_compute_bow
    orbm_handle* owner = nullptr;
    int device = -1;
    int slots = 0, cap = 0, ncell = 0, nlevels = 0;
    orbm::GridDev gd{};
    orbm::UndistArgs und{};
    int undistort = 0;
    float bounds[4] = {0, 0, 0, 0};
    uint8_t* d_block = nullptr;   // one allocation: keysUn | desc | ang | cellStart | cellIdx | n | scale | candOff | candCnt | qres | occ | total
    orbt::FrameSetDev fs{};
    float* d_scale = nullptr;
    int32_t* d_candOff = nullptr; int32_t* d_candCnt = nullptr; int32_t* d_qres = nullptr; uint8_t* d_occ = nullptr; int32_t* d_total = nullptr; int32_t* d_qscr = nullptr;
    int32_t* d_tscr = nullptr;   // [slots][3 tCap]: the resolve's per-train tables of a set whose frames are too large for the LDS form (ProjCommon::big)
    uint2* d_cand = nullptr; int candCapPair = 0;
    uint8_t* h_block = nullptr;   // pinned, one share per result set (set_tables): assign[R][slots][cap] | nmatch[R][slots] | stats[R][slots][2] | flag[R][slots]
    int32_t* h_assign = nullptr; int32_t* h_nmatch = nullptr; int32_t* h_stats = nullptr;
    int32_t* h_flag = nullptr;                 // raised by the resolve behind a pair's results (at most kTrackFlagPairs pairs)
    ResultRing res;
    int32_t seq = 0;                           // value the flags of the newest search carry
    uint32_t builds = 0;                       // frame builds so far
    std::vector<uint32_t> slotBuilt;           // per slot: the build count that last wrote it
    hipEvent_t evExt[2] = {nullptr, nullptr};  // this set's build has read the extractor's result set s
    std::vector<orbx_handle*> readOf;          // extractors whose evExtReader lists may hold them
    // orbm_frameset_attach: the set's kernels ride on this extractor's own stream, right behind the kernels whose
    // output they read (the live stream: no cross-stream hand-over, no host hop between Frame::Frame and the search)
    orbx_handle* liveEx = nullptr;
    // the query searches: one pinned block + its device twin per result set (pair record | queries | occupancy); qEpoch counts
    // their allocations (a larger local map than any before reallocates all four)
    uint8_t* h_q = nullptr; uint8_t* d_q = nullptr; size_t qBytes = 0;   // per set
    uint32_t qEpoch = 0;
};

// the stream a frame set's kernels are enqueued on
static inline hipStream_t fs_stream(const orbm_frameset* fs) { return fs->liveEx ? fs->liveEx->streamP[0] : fs->owner->stream; }

// result set `set`'s share of the pinned tables: assign[slots][cap], nmatch[slots], stats[slots][2], flag[slots]
struct SetTables { int32_t *assign, *nmatch, *stats, *flag; };
static inline SetTables set_tables(const orbm_frameset* fs, int set)
{
    const size_t S = (size_t)fs->slots, C = (size_t)fs->cap;
    return {fs->h_assign + set * S * C, fs->h_nmatch + set * S, fs->h_stats + set * S * 2, fs->h_flag + set * S};
}

// every pair of the set's search has raised its flag (a search without flags never has)
static inline bool flags_raised(const ResultRecord& r, const int32_t* flag)
{
    bool up = r.flagValue != 0;
    for (int p = 0; p < r.pairs && up; p++) up = ((const volatile int32_t*)flag)[p] == r.flagValue;
    return up;
}

extern "C" int orbm_frameset_destroy(orbm_frameset_t* fs)
{
    if (!fs) return ORBX_OK;
    if (fs->device >= 0) {
        (void)hipSetDevice(fs->device);
        if (fs->liveEx && live_has(fs->liveEx)) { (void)flush_pack(fs->liveEx); fs->liveEx->attachedSets--; (void)hipStreamSynchronize(fs->liveEx->streamP[0]); }
        if (live_has(fs->owner)) (void)hipStreamSynchronize(fs->owner->stream);
        else (void)hipDeviceSynchronize();  // the matcher handle went first
        frameset_bow_free(fs);
        if (fs->d_block) (void)hipFree(fs->d_block);
        if (fs->d_cand) (void)hipFree(fs->d_cand);
        if (fs->h_block) (void)hipHostFree(fs->h_block);
        if (fs->h_q) (void)hipHostFree(fs->h_q);
        if (fs->d_q) (void)hipFree(fs->d_q);
        fs->res.destroy();
        for (auto e : fs->evExt) {
            if (!e) continue;
            for (orbx_handle* x : fs->readOf)
                if (live_has(x)) for (auto& lst : x->evExtReader) lst.erase(std::remove(lst.begin(), lst.end(), e), lst.end());
            (void)hipEventDestroy(e);
        }
    }
    delete fs;
    return ORBX_OK;
}

extern "C" int orbm_frameset_create(orbm_t* h, int slots, int cap, const float K[4], const float D[5], const OrbmGrid* grid,
                                    const float bounds[4], const float* scale_factors, int nlevels, orbm_frameset_t** out)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!out || slots < 1 || cap < 1 || !K || !D || !bounds || !scale_factors || nlevels < 1 || nlevels > ORBX_MAX_LEVELS)
        return fail(ORBX_E_INVALID, "bad argument");
    if (!grid || grid->cols < 1 || grid->rows < 1 || grid->cols * grid->rows > (1 << 20)) return fail(ORBX_E_INVALID, "bad grid");
    if (slots > 32767) return fail(ORBX_E_INVALID, "at most 32767 slots");
    if (cap > kProjMaxTrainBig) return fail(ORBX_E_UNSUPPORTED, "frame capacity %d: at most %d features per frame (16-bit feature indices in the candidate lists)", cap, kProjMaxTrainBig);
    ProjPlan plan0{};
    if ((rc = proj_lds_plan(cap, cap, grid->cols * grid->rows, plan0))) return rc;
    const bool bigSet = plan0.c.big != 0;   // frames beyond the LDS form: general-size build, tables in memory (slower; the reference has no bound)
    *out = nullptr;
    orbm_frameset* f = new orbm_frameset;
    f->slotBuilt.assign((size_t)slots, 0u);
    for (auto& r : f->res.rec) { r.cur.reserve((size_t)slots); r.last.reserve((size_t)slots); }   // no allocation in the per-frame path
    f->owner = h; f->device = h->device; f->slots = slots; f->cap = cap; f->ncell = grid->cols * grid->rows; f->nlevels = nlevels;
    f->gd = {grid->minX, grid->minY, grid->invW, grid->invH, grid->cols, grid->rows};
    f->und = {K[0], K[1], K[2], K[3], D[0], D[1], D[2], D[3], D[4]};
    f->undistort = D[0] != 0.0f;  // Frame.cc:406-410
    memcpy(f->bounds, bounds, sizeof f->bounds);
    Packer pk;
    const size_t S = (size_t)slots, C = (size_t)cap;
    const size_t oK = pk.take(S * C * sizeof(OrbxKeyPoint)), oD = pk.take(S * C * 32), oA = pk.take(S * C * 4);
    const size_t oCs = pk.take(S * (f->ncell + 1) * 4), oCi = pk.take(S * C * 4), oRec = pk.take(S * C * 16), oN = pk.take(S * 4), oSc = pk.take((size_t)nlevels * 4);
    const size_t oOff = pk.take(S * C * 4), oCnt = pk.take(S * C * 4), oQr = pk.take(S * C * 4), oQs = pk.take(S * C * 12), oOcc = pk.take(S * C), oTot = pk.take(S * 4);
    const size_t oTs = bigSet ? pk.take(S * (size_t)plan0.c.tCap * 12) : 0;
    f->candCapPair = (int)std::max<size_t>(C * 64, 1 << 16);
    Packer hp;
    const size_t R = ResultRing::kSets;
    const size_t hA = hp.take(R * S * C * 4), hN = hp.take(R * S * 4), hS = hp.take(R * S * 8), hF = hp.take(R * S * 4);
    HIPCHK_OR(hipMalloc(&f->d_block, pk.off), orbm_frameset_destroy(f));
    HIPCHK_OR(hipMalloc(&f->d_cand, S * (size_t)f->candCapPair * 8), orbm_frameset_destroy(f));
    // read by the host behind an event -- or, for the few pairs of a live stream, behind a flag while the kernel's queue
    // is still busy: explicitly coherent (fine-grained), whatever HIP_HOST_COHERENT says
    HIPCHK_OR(hipHostMalloc(&f->h_block, hp.off, hipHostMallocCoherent), orbm_frameset_destroy(f));
    memset(f->h_block + hF, 0, R * S * 4);
    HIPCHK_OR(hipMemsetAsync(f->d_block + oN, 0, S * 4, h->stream), orbm_frameset_destroy(f));
    HIPCHK_OR(hipMemsetAsync(f->d_block + oTot, 0, S * 4, h->stream), orbm_frameset_destroy(f));
    HIPCHK_OR(hipMemcpyAsync(f->d_block + oSc, scale_factors, (size_t)nlevels * 4, hipMemcpyHostToDevice, h->stream), orbm_frameset_destroy(f));
    HIPCHK_OR(hipStreamSynchronize(h->stream), orbm_frameset_destroy(f));
    uint8_t* b = f->d_block;
    f->fs = {(orbm::KeyDev*)(b + oK), b + oD, (float*)(b + oA), (int32_t*)(b + oCs), (int32_t*)(b + oCi), (uint4*)(b + oRec), (int32_t*)(b + oN), cap, f->ncell};
    f->d_scale = (float*)(b + oSc);
    f->d_candOff = (int32_t*)(b + oOff); f->d_candCnt = (int32_t*)(b + oCnt); f->d_qres = (int32_t*)(b + oQr); f->d_occ = b + oOcc;
    f->d_total = (int32_t*)(b + oTot); f->d_qscr = (int32_t*)(b + oQs);
    f->d_tscr = bigSet ? (int32_t*)(b + oTs) : nullptr;
    f->h_assign = (int32_t*)(f->h_block + hA); f->h_nmatch = (int32_t*)(f->h_block + hN); f->h_stats = (int32_t*)(f->h_block + hS);
    f->h_flag = (int32_t*)(f->h_block + hF);
    *out = f;
    return ORBX_OK;
}

static int frameset_check(orbm_frameset* fs)
{
    if (!fs || !fs->owner) return fail(ORBX_E_INVALID, "null frame set");
    if (!live_has(fs->owner)) return fail(ORBX_E_INVALID, "the frame set's matcher handle was destroyed");
    if (fs->liveEx && !live_has(fs->liveEx)) return fail(ORBX_E_INVALID, "the extractor the frame set is attached to was destroyed");
    return orbm_check(fs->owner);
}

// the arguments of a build of n frames into slots (slot0 + i) % slots, which it stamps with the new build count
static orbt::FrameBuildArgs frameset_build_args(orbm_frameset* fs, int slot0, int n, const OrbxKeyPoint* d_keys, const uint8_t* d_desc,
                                                const int32_t* d_counts, int src_cap)
{
    orbt::FrameBuildArgs fa{};
    fa.fs = fs->fs;
    fa.srcKeys = (const orbm::KeyDev*)d_keys; fa.srcDesc = d_desc; fa.srcCount = d_counts; fa.srcCap = src_cap; fa.srcN = 0;
    fa.slot0 = slot0; fa.slotMod = fs->slots;
    fa.grid = fs->gd; fa.und = fs->und; fa.undistort = fs->undistort;
    fs->builds++;
    for (int i = 0; i < n; i++) fs->slotBuilt[(size_t)((slot0 + i) % fs->slots)] = fs->builds;
    return fa;
}

extern "C" int orbm_frameset_build(orbm_frameset_t* fs, int slot0, int n, const OrbxKeyPoint* d_keys, const uint8_t* d_desc,
                                   const int32_t* d_counts, int src_cap)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (slot0 < 0 || slot0 >= fs->slots || n < 0 || n > fs->slots || !d_keys || !d_desc || !d_counts || src_cap < 1)
        return fail(ORBX_E_INVALID, "bad argument");
    if ((uintptr_t)d_desc & 15) return fail(ORBX_E_INVALID, "descriptors must be 16-byte aligned");
    if (n == 0) return ORBX_OK;
    return frame_build_launch(fs->owner, frameset_build_args(fs, slot0, n, d_keys, d_desc, d_counts, src_cap), n, fs_stream(fs));
}

// the frames of the extractor's last batch, ordered behind its kernels on the device; the extractor will not overwrite
// that result set before this build has read it
extern "C" int orbm_frameset_build_from_extractor(orbm_frameset_t* fs, int slot0, orbx_t* ex)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!ex || ex->device != fs->owner->device) return fail(ORBX_E_INVALID, "extractor and frame set must share the device");
    const int B = ex->lastB;
    if (slot0 < 0 || slot0 >= fs->slots || B < 1 || B > fs->slots) return fail(ORBX_E_INVALID, "bad argument");
    if (fs->cap < ex->maxKp) return fail(ORBX_E_CAPACITY, "frame set capacity %d is below the extractor's %d keypoints per frame (orbx_max_keypoints)", fs->cap, ex->maxKp);
    const int set = ex->curSet;
    hipStream_t ms = fs_stream(fs);
    // attached to this extractor and its last call was a latency-mode one (the whole chain ran on streamP[0]): stream
    // order alone puts the build behind the descriptors and in front of the next extraction -- no event either way
    // (an event between two kernels of a chain costs ~5 us of gap, tools/live_timeline.sh)
    const bool sameStream = fs->liveEx == ex && ex->lastLat;
    if (!sameStream && ((rc = flush_pack(ex)) || (rc = join_parts(ex, ms)))) return rc;
    const orbt::FrameBuildArgs fa = frameset_build_args(fs, slot0, B, (const OrbxKeyPoint*)(r_kps(ex, set) + ex->maxKp), r_desc(ex, set) + (size_t)ex->maxKp * 32,
                                                        r_count(ex, set) + 1, ex->maxKp);
    if (sameStream && ex->packPending && ex->packB == B && frame_build_fits_lds(fs->fs.cap, fs->fs.ncell)) {
        // the ticket's results go to the host from the build's own launch (k_frame_build_pack)
        const size_t lds = (size_t)fa.fs.ncell * 8 + (size_t)align_up(fa.fs.cap, 2) * 14;
        if ((rc = lds_attr((const void*)orbt::k_frame_build_pack, lds, fs->owner->ldsAttr[7]))) return rc;
        ex->packPending = false;
        hipLaunchKernelGGL(orbt::k_frame_build_pack, dim3(B * (1 + orbt::kPackParts)), dim3(orbt::kThreads), lds, ms, fa, ex->packPa, B);
        HIPCHK(hipGetLastError());
        return ORBX_OK;
    }
    if ((rc = flush_pack(ex)) || (rc = frame_build_launch(fs->owner, fa, B, ms))) return rc;
    if (sameStream) return ORBX_OK;
    if (!fs->evExt[set]) HIPCHK(hipEventCreateWithFlags(&fs->evExt[set], hipEventDisableTiming));
    HIPCHK(hipEventRecord(fs->evExt[set], ms));
    auto& lst = ex->evExtReader[set];
    if (std::find(lst.begin(), lst.end(), fs->evExt[set]) == lst.end()) lst.push_back(fs->evExt[set]);
    if (std::find(fs->readOf.begin(), fs->readOf.end(), ex) == fs->readOf.end()) fs->readOf.push_back(ex);
    return ORBX_OK;
}

extern "C" int orbm_frameset_sync(orbm_frameset_t* fs)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(fs_stream(fs)));
    return ORBX_OK;
}

// The live stream (one frame per robot per call, M/Examples/Monocular/mono_kitti.cc:80-101): Frame::Frame's tail and the
// searches of Tracking become part of the extractor's own chain of kernels.  ex = nullptr detaches.  Both streams are
// drained on the switch, so the frames already in the set stay valid.
extern "C" int orbm_frameset_attach(orbm_frameset_t* fs, orbx_t* ex)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (ex && (!live_has(ex) || ex->device != fs->owner->device)) return fail(ORBX_E_INVALID, "extractor and frame set must share the device");
    HIPCHK(hipStreamSynchronize(fs_stream(fs)));
    if (fs->bow) return fail(ORBX_E_UNSUPPORTED, "attach the frame set before its first orbm_frameset_compute_bow");
    if (fs->liveEx && live_has(fs->liveEx)) { if ((rc = flush_pack(fs->liveEx))) return rc; fs->liveEx->attachedSets--; }
    fs->liveEx = ex;
    if (ex) ex->attachedSets++;
    HIPCHK(hipStreamSynchronize(fs_stream(fs)));
    return ORBX_OK;
}

extern "C" int orbm_frameset_download(orbm_frameset_t* fs, int slot, OrbxKeyPoint* keys_un, uint8_t* desc, int cap, int* n_out)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (slot < 0 || slot >= fs->slots) return fail(ORBX_E_INVALID, "slot %d outside the frame set", slot);
    hipStream_t s = fs_stream(fs);
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, fs->fs.n + slot, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_out) *n_out = n;
    if (n > cap) return fail(ORBX_E_CAPACITY, "%d features, caller capacity %d", n, cap);
    if (n && keys_un) HIPCHK(hipMemcpyAsync(keys_un, fs->fs.keysUn + (size_t)slot * fs->cap, (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyDeviceToHost, s));
    if (n && desc) HIPCHK(hipMemcpyAsync(desc, fs->fs.desc + (size_t)slot * fs->cap * 32, (size_t)n * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

// SearchByProjection(CurrentFrame = slot cur[p], LastFrame = slot last[p], th, bMono = true) for npairs pairs; every
// LastFrame feature is a query (as if it held a MapPoint with observations), projected with the identity pose.
// Asynchronous, uploads nothing (the pair records are made on the device from the slot numbers); results alternate
// between four pinned result sets so that a caller can read call n-1 .. n-3 while call n runs.
// the launches of the frame-to-frame search that result set `set`'s record holds (+ the set's event); flags: the few-pairs
// flag protocol, its flags carry fs->seq + 1
static int track_frames_issue(orbm_frameset_t* fs, int set, bool flags)
{
    int rc;
    orbm_handle* h = fs->owner;
    hipStream_t st = fs_stream(fs);
    const ResultRecord& r = fs->res.rec[set];
    const int npairs = (int)r.cur.size();
    if (npairs) {
        ProjPlan pl{};
        if ((rc = proj_lds_plan(fs->cap, fs->cap, fs->ncell, pl, r.th > 20.f ? 72 : 32))) return rc;  // th = 15: ~12 per query listed, th = 30: ~45
        orbt::ProjCommon& c = pl.c;
        c.mode = 4; c.nnratio = r.pp.nnratio; c.checkOri = r.pp.check_ori; c.thDist = r.pp.th_dist;
        c.scale = fs->d_scale; c.nlevels = fs->nlevels;
        c.interleave = npairs <= 4;
        if (!c.big) c.lanes = cand_lanes(npairs);
        if ((rc = lds_attr((const void*)orbt::k_track_candidates, pl.ldsCand, h->ldsAttr[3])) ||
            (rc = lds_attr((const void*)orbt::k_track_resolve, pl.ldsResolve, h->ldsAttr[4]))) return rc;
        const SetTables t = set_tables(fs, set);
        orbt::TrackArgs a{};
        a.fs = fs->fs; a.grid = fs->gd;
        a.th = r.th; a.minX = fs->bounds[0]; a.maxX = fs->bounds[1]; a.minY = fs->bounds[2]; a.maxY = fs->bounds[3];
        a.occ = fs->d_occ; a.assign = t.assign; a.nmatch = t.nmatch; a.stats = t.stats;
        a.total = fs->d_total; a.candOff = fs->d_candOff; a.candCnt = fs->d_candCnt; a.cand = fs->d_cand; a.candCap = fs->candCapPair; a.qres = fs->d_qres; a.qscr = fs->d_qscr; a.tscr = c.big ? fs->d_tscr : nullptr;
        a.flag = flags ? t.flag : nullptr; a.flagValue = fs->seq + 1;
        const int perSlice = orbt::kCandThreads / c.lanes;
        const int slices = (fs->cap + perSlice - 1) / perSlice;
        for (int p0 = 0; p0 < npairs; p0 += orbt::kTrackMaxPairs) {
            const int nb = std::min(orbt::kTrackMaxPairs, npairs - p0);
            a.pair0 = p0;
            for (int i = 0; i < nb; i++) { a.cur[i] = (int16_t)r.cur[(size_t)(p0 + i)]; a.last[i] = (int16_t)r.last[(size_t)(p0 + i)]; }
            hipLaunchKernelGGL(orbt::k_track_candidates, dim3(slices, nb), dim3(orbt::kCandThreads), pl.ldsCand, st, a, c);
            hipLaunchKernelGGL(orbt::k_track_resolve, dim3(nb), dim3(orbt::kThreads), pl.ldsResolve, st, a, c);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(r.ev, st));
    return ORBX_OK;
}

extern "C" int orbm_track_frames(orbm_frameset_t* fs, const OrbmProjParams* pp, float th, const int32_t* cur_slots,
                                 const int32_t* last_slots, int npairs)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!pp || pp->mode != 4) return fail(ORBX_E_INVALID, "the frame-to-frame search is mode 4");
    if (npairs < 0 || npairs > fs->slots || (npairs && (!cur_slots || !last_slots))) return fail(ORBX_E_INVALID, "bad argument");
    for (int p = 0; p < npairs; p++)
        if (cur_slots[p] < 0 || cur_slots[p] >= fs->slots || last_slots[p] < 0 || last_slots[p] >= fs->slots)
            return fail(ORBX_E_INVALID, "slot outside the frame set");
    const int set = fs->res.next();
    if ((rc = fs->res.begin(set))) return rc;
    ResultRecord& r = fs->res.rec[set];
    r.pp = *pp; r.builds = fs->builds; r.th = th; r.cur.assign(cur_slots, cur_slots + npairs); r.last.assign(last_slots, last_slots + npairs);
    // few pairs (a live stream): every resolve workgroup raises a flag behind its results, orbm_track_results polls it
    const bool flags = npairs > 0 && npairs <= kTrackFlagPairs;
    if ((rc = track_frames_issue(fs, set, flags))) return rc;
    fs->res.commit(set, ResultRecord::kFramePairs, npairs, flags ? ++fs->seq : 0);
    return ORBX_OK;
}

// a query search lists into the whole arena
static inline void query_arena(const orbm_frameset* fs, orbt::ProjPair& P) { P.cand = fs->d_cand; P.candCap = (int)std::min<size_t>((size_t)fs->slots * fs->candCapPair, 0x7FFFFFFF); }

// the launches of the query search that result set `set`'s record holds (+ the set's event): its staging block goes up through
// the copy kernel of the live chain (orbx::k_upload: the DMA engine's completion reaches the compute queue ~20 us after the
// copy's end, a kernel's successor follows it at once), the search follows
static int track_queries_issue(orbm_frameset_t* fs, int set)
{
    int rc;
    const ResultRecord& r = fs->res.rec[set];
    hipStream_t st = fs_stream(fs);
    uint8_t* ds = fs->d_q + (size_t)set * fs->qBytes;
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((r.total / 16 + 255) / 256)), dim3(256), 0, st, (const uint4*)(fs->h_q + (size_t)set * fs->qBytes), (uint4*)ds, (int)(r.total / 16));
    if ((rc = proj_launch(fs->owner, (const orbt::ProjPair*)ds, 1, r.nq, r.plan, st))) return rc;
    HIPCHK(hipEventRecord(r.ev, st));
    return ORBX_OK;
}

// result set `set`'s share of the query staging (pinned block + device twin) holds `total` bytes and is free to be written
static int query_block_take(orbm_frameset_t* fs, int set, size_t total)
{
    const ResultRecord& r = fs->res.rec[set];
    if (total > fs->qBytes) {   // (first call, or a larger local map than any before: the only allocation, behind a drain)
        HIPCHK(hipStreamSynchronize(fs_stream(fs)));
        if (fs->h_q) HIPCHK(hipHostFree(fs->h_q));
        if (fs->d_q) HIPCHK(hipFree(fs->d_q));
        fs->h_q = nullptr; fs->d_q = nullptr; fs->qBytes = 0;
        fs->qEpoch++;
        const size_t want = (total * 3 / 2 + 4095) & ~(size_t)4095;
        HIPCHK(hipHostMalloc(&fs->h_q, want * ResultRing::kSets, hipHostMallocCoherent));   // (read by the copy kernel where it lies)
        HIPCHK(hipMalloc(&fs->d_q, want * ResultRing::kSets));
        fs->qBytes = want;
    } else if (r.ev && !flags_raised(r, set_tables(fs, set).flag)) {
        // the search that last read this set's block (four calls ago) must be through: its flags say so without a runtime
        // call (an event query costs tens of microseconds)
        HIPCHK(hipEventSynchronize(r.ev));
    }
    return ORBX_OK;
}

// int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th)   ORBmatcher.cc:45-129,
// the search Tracking::SearchLocalPoints runs on every frame (Tracking.cc:1242-1249), with the frame resident in the set:
// the local map's projections (Frame::isInFrustum, Frame.cc:269-325) go up in ONE pinned block, two launches follow on
// the set's stream, the table lands in the set's pinned result block behind a flag -- no allocation, no sync inside.
// qslot >= 0: the queries ARE the features of that slot (descriptors and angles stay in HBM), only their projections come
// from the host
static int track_queries(orbm_frameset_t* fs, int slot, int qslot, const OrbmProjParams* pp, const float* q_uvr, const int8_t* q_lvl,
                         const uint8_t* qdesc, const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq, const uint8_t* t_occ)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!pp || pp->mode < 3 || pp->mode > 6) return fail(ORBX_E_INVALID, "mode must be 3 .. 6");
    if (slot < 0 || slot >= fs->slots || qslot >= fs->slots || nq < 0 || (nq && (!q_uvr || !q_lvl || (!qdesc && qslot < 0)))) return fail(ORBX_E_INVALID, "bad argument");
    if (qslot >= 0 && nq > fs->cap) return fail(ORBX_E_INVALID, "%d projections for a frame of at most %d features", nq, fs->cap);
    const size_t C = (size_t)fs->cap, S = (size_t)fs->slots;
    if ((size_t)nq > S * C || nq > orbt::kMaxQueryIters * orbt::kThreads)
        return fail(ORBX_E_UNSUPPORTED, "%d queries: the set's scratch holds slots x cap = %zu", nq, S * C);
    const int set = fs->res.next();
    ResultRecord& r = fs->res.rec[set];
    Packer pk;
    const size_t oPair = pk.take(sizeof(orbt::ProjPair));
    const size_t oUvr = pk.take((size_t)nq * 12), oLvl = pk.take((size_t)nq * 2), oQd = qslot < 0 ? pk.take((size_t)nq * 32) : 0;
    const size_t oQv = qvalid ? pk.take((size_t)nq) : 0, oQo = q_obs_pos ? pk.take((size_t)nq) : 0, oOcc = t_occ ? pk.take(C) : 0;
    const size_t total = pk.off;
    if ((rc = query_block_take(fs, set, total))) return rc;
    if ((rc = fs->res.begin(set))) return rc;
    ProjPlan& pl = r.plan;
    if ((rc = proj_lds_plan(fs->cap, nq, fs->ncell, pl))) return rc;
    orbt::ProjCommon& c = pl.c;
    c.mode = pp->mode; c.nnratio = pp->nnratio; c.thDist = pp->th_dist;
    c.checkOri = qslot >= 0 ? pp->check_ori : 0;   // (host-side queries carry no angles: modes 4 / 5 run without the rotation check then)
    proj_plan_queries(c, 1);   // (a local map's MapPoints come in no particular order)
    uint8_t* hs = fs->h_q + (size_t)set * fs->qBytes;
    uint8_t* ds = fs->d_q + (size_t)set * fs->qBytes;
    memcpy(hs + oUvr, q_uvr, (size_t)nq * 12); memcpy(hs + oLvl, q_lvl, (size_t)nq * 2);
    if (qslot < 0) memcpy(hs + oQd, qdesc, (size_t)nq * 32);
    if (qvalid) memcpy(hs + oQv, qvalid, (size_t)nq);
    if (q_obs_pos) memcpy(hs + oQo, q_obs_pos, (size_t)nq);
    if (t_occ) memcpy(hs + oOcc, t_occ, C);
    const SetTables t = set_tables(fs, set);
    orbt::ProjPair P{};
    orbt::proj_train(P, orbt::train_side(fs->fs, slot, fs->gd));
    P.quvr = (const float*)(ds + oUvr); P.qlvl = (const int8_t*)(ds + oLvl);
    P.qdesc = qslot < 0 ? ds + oQd : fs->fs.desc + (int64_t)qslot * C * 32;
    P.qang = qslot < 0 ? nullptr : fs->fs.ang + (int64_t)qslot * C;
    P.qvalid = qvalid ? ds + oQv : nullptr; P.qobs = q_obs_pos ? ds + oQo : nullptr;
    P.nqPtr = qslot < 0 ? nullptr : fs->fs.n + qslot; P.nq = nq;   // (never more queries than the slot holds features)
    P.toccIn = t_occ ? ds + oOcc : nullptr; P.toccOut = fs->d_occ;
    P.assign = t.assign; P.initAssign = 1; P.nmatch = t.nmatch; P.stats = t.stats; P.flag = t.flag; P.flagValue = fs->seq + 1;
    P.total = fs->d_total; P.candOff = fs->d_candOff; P.candCnt = fs->d_candCnt; query_arena(fs, P);
    P.qres = fs->d_qres; P.qscr = fs->d_qscr; P.tscr = c.big ? fs->d_tscr : nullptr;
    memcpy(hs + oPair, &P, sizeof P);
    r.pp = *pp; r.builds = fs->builds; r.slot = slot; r.qslot = qslot; r.nq = nq; r.total = total; r.qEpoch = fs->qEpoch; r.fromPool = false;
    if ((rc = track_queries_issue(fs, set))) return rc;
    fs->res.commit(set, ResultRecord::kQueries, 1, ++fs->seq);
    return ORBX_OK;
}

extern "C" int orbm_track_local_points(orbm_frameset_t* fs, int slot, const OrbmProjParams* pp, const float* q_uvr, const int8_t* q_lvl,
                                       const uint8_t* qdesc, const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq, const uint8_t* t_occ)
{
    if (nq && !qdesc) return fail(ORBX_E_INVALID, "bad argument");
    return track_queries(fs, slot, -1, pp, q_uvr, q_lvl, qdesc, qvalid, q_obs_pos, nq, t_occ);
}

// int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono)
// ORBmatcher.cc:1330-1472 with a REAL pose: the caller projects LastFrame's MapPoints with CurrentFrame.mTcw (:1362-1378, cv::Mat
// algebra on the host) and hands over u, v, radius and the octave window per LastFrame feature; descriptors, angles and
// both frames' grids never leave HBM.
extern "C" int orbm_track_frame_projected(orbm_frameset_t* fs, int cur_slot, int last_slot, const OrbmProjParams* pp, const float* q_uvr,
                                          const int8_t* q_lvl, const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq, const uint8_t* t_occ)
{
    if (last_slot < 0) return fail(ORBX_E_INVALID, "bad argument");
    return track_queries(fs, cur_slot, last_slot, pp, q_uvr, q_lvl, nullptr, qvalid, q_obs_pos, nq, t_occ);
}

// waits for the last (back = 0) or an earlier (back = 1 .. 3) search; views into the frame set's pinned result block (valid
// until three more calls have been issued): assign[p * cap + t] = LastFrame feature matched to CurrentFrame feature t or -1
extern "C" int orbm_track_results(orbm_frameset_t* fs, int back, const int32_t** assign, const int32_t** nmatches, int* npairs, int* cap)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (back < 0 || back >= ResultRing::kSets) return fail(ORBX_E_INVALID, "back must be 0 .. %d", ResultRing::kSets - 1);
    const int set = fs->res.back(back);
    ResultRecord& r = fs->res.rec[set];
    if (!r.ev) return fail(ORBX_E_INVALID, "no such search has been issued");
    const SetTables t = set_tables(fs, set);
    const size_t S = (size_t)fs->slots;
    bool landed = false;
    if (r.flagValue) {
        for (int spin = 0; spin < 400000 && !(landed = flags_raised(r, t.flag)); spin++) cpu_relax();
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    if (!landed) HIPCHK(hipEventSynchronize(r.ev));
    int need = 0;
    for (int p = 0; p < r.pairs; p++)
        if (t.nmatch[p] < 0) need = std::max(need, -t.nmatch[p] - 1);
    if (need > 0 && r.kind != ResultRecord::kNone) {
        // a pair's candidates did not fit the arena (64 per feature; the kernels count what they could not list and write
        // nothing past it): grow it and run the search this set's record holds again, into the same set -- slow path, allocates.
        // Refused when a slot it read has been rebuilt by a later frame since (callers that run tickets deep: every build
        // stamps its slots with a generation), or a query search's staging block has been reallocated by a larger one.
        auto rebuilt = [&](int slot) { return slot >= 0 && fs->slotBuilt[(size_t)slot] > r.builds; };
        bool moved = false;
        if (r.kind == ResultRecord::kFramePairs) {
            for (size_t p = 0; p < r.cur.size(); p++) moved |= rebuilt(r.cur[p]) || rebuilt(r.last[p]);
        } else {
            moved = rebuilt(r.slot) || rebuilt(r.qslot) || r.qEpoch != fs->qEpoch;
            need = (int)((need + S - 1) / S);   // (the query search lists into the whole arena: size each pair's share)
        }
        if (moved)
            return fail(ORBX_E_CAPACITY, "the search's candidates exceed the arena and a slot it read has been rebuilt (or its staging block reallocated) since it was "
                                         "issued: it cannot be run again -- read a search's results before its slots are reused, or search fewer pairs per call");
        HIPCHK(hipStreamSynchronize(fs_stream(fs)));
        const size_t newCap = (size_t)need + (size_t)need / 4 + 1024;
        if (newCap * S * 8 > ((size_t)1 << 32)) return fail(ORBX_E_CAPACITY, "%d candidates per pair are more than the frame set can list", need);
        uint2* bigger = nullptr;
        HIPCHK(hipMalloc(&bigger, S * newCap * 8));
        HIPCHK(hipFree(fs->d_cand));
        fs->d_cand = bigger; fs->candCapPair = (int)newCap;
        if (r.kind == ResultRecord::kFramePairs) {
            if ((rc = track_frames_issue(fs, set, false))) return rc;
            r.flagValue = 0;
        } else {   // (only the search that takes a set writes its staging block: only the arena in its pair record changes)
            query_arena(fs, *(orbt::ProjPair*)(fs->h_q + (size_t)set * fs->qBytes));
            if ((rc = track_queries_issue(fs, set))) return rc;
        }
        HIPCHK(hipEventSynchronize(r.ev));
    }
    for (int p = 0; p < r.pairs; p++)
        if (t.nmatch[p] < 0) return fail(ORBX_E_CAPACITY, "pair %d: %d candidates exceed the arena of %d", p, -t.nmatch[p] - 1, fs->candCapPair);
    r.accepted = true;
    if (assign) *assign = t.assign;
    if (nmatches) *nmatches = t.nmatch;
    if (npairs) *npairs = r.pairs;
    if (cap) *cap = fs->cap;
    return ORBX_OK;
}

// of the last search, after orbm_track_results
extern "C" int orbm_track_stats(orbm_frameset_t* fs, int pair, int* rounds, int* candidates)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    const ResultRecord& r = fs->res.rec[fs->res.newest];
    if (pair < 0 || pair >= r.pairs || !r.ev) return fail(ORBX_E_INVALID, "bad argument");
    HIPCHK(hipEventSynchronize(r.ev));
    const int32_t* st = set_tables(fs, fs->res.newest).stats;
    if (rounds) *rounds = st[2 * pair];
    if (candidates) *candidates = st[2 * pair + 1];
    return ORBX_OK;
}

extern "C" int orbm_last_search_stats(orbm_t* h, int* rounds, int* candidates)
{
    if (!h) return fail(ORBX_E_INVALID, "null handle");
    if (rounds) *rounds = h->lastRounds;
    if (candidates) *candidates = h->lastCands;
    return ORBX_OK;
}

#ifdef ORBT_PHASE_TIMING
extern "C" int orbm_debug_build_phases(double* us, int n)
{
    unsigned long long t[12];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(t, HIP_SYMBOL(orbt::g_orbtBuild), sizeof t));
    for (int i = 0; i < n && i < 11; i++) us[i] = (double)(t[i + 1] - t[i]) * 0.01;
    return ORBX_OK;
}
extern "C" int orbm_debug_round_census(int32_t* out, int nrounds)
{
    int32_t t[64][2];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(t, HIP_SYMBOL(orbt::g_orbtCensus), sizeof t));
    for (int i = 0; i < nrounds && i < 64; i++) { out[2 * i] = t[i][0]; out[2 * i + 1] = t[i][1]; }
    return ORBX_OK;
}
extern "C" int orbm_debug_phase_times(double* us, int n)
{
    unsigned long long t[16];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(t, HIP_SYMBOL(orbt::g_orbtPhase), sizeof t));
    for (int i = 0; i < n && i < 15; i++) us[i] = (double)(t[i + 1] - t[i]) * 0.01;
    return ORBX_OK;
}
#endif
