// orbe_host.inc -- host side of the loop correction over a keyframe store (part of orbslamm_hip.hip; kernels:
// orbe_kernels.hip, ABI: include/orbslamm_correct.h, DESIGN.md §8x).
//   the store     the columns it reads (centres, octaves) and the resident mpRefKF array are the store's: set in orbu_host.inc,
//                 freed by orbu_store_destroy
//   the blocks    the claim words (pool-sized) at the first correction; the per-keyframe and per-point arrays grow with the largest
//                 K and the largest count of moved points seen.  This file owns these alone: the observation index and its
//                 per-point arrays are orbr_host.inc's
//   a call        poses, claim, count, scan, the total down, the FIRST synchronisation (the count of moved points sizes what
//                 follows and answers ORBX_E_CAPACITY); place, move, orbr_issue (orbr's mark / count / segments / place and its
//                 two refresh kernels), the records, orbr's header down, the second synchronisation; orbr_check_header;
//                 then the commit as a launch of its own, the records down into the outputs, the last synchronisation

static_assert(sizeof(OrbePoint) == 4 * orbe::kPointWords && sizeof(OrbeKeyFrame) == sizeof(orbe::KfRec) && sizeof(OrbeKeyFrame) == 192, "orbslamm_correct.h layouts");
static_assert(offsetof(OrbePoint, pos) == 4 * orbe::P_POS && offsetof(OrbePoint, normal) == 4 * orbe::P_NORMAL && offsetof(OrbePoint, min_distance) == 4 * orbe::P_MIN &&
              offsetof(OrbePoint, n_obs) == 4 * orbe::P_NOBS && offsetof(OrbePoint, status) == 4 * orbe::P_STATUS, "OrbePoint as the kernels write it");
static_assert(offsetof(OrbeKeyFrame, non_corrected) == offsetof(orbe::KfRec, non) && offsetof(OrbeKeyFrame, Tiw) == offsetof(orbe::KfRec, Tiw) &&
              offsetof(OrbeKeyFrame, Ow) == offsetof(orbe::KfRec, Ow) && offsetof(OrbeKeyFrame, n_points) == offsetof(orbe::KfRec, nPts), "OrbeKeyFrame as the kernels write it");

struct orbe_blocks {
    uint8_t* d_block = nullptr;                      // claims | header
    uint8_t* d_kf = nullptr; size_t kfCap = 0;       // kf | inv | rowCnt | rowStart, for the largest K so far
    uint8_t* d_pts = nullptr; size_t ptsCap = 0;     // ids | ownerRank | ownerIdx | ref | newPos | out, for the largest n so far
    std::vector<int32_t> order;                      // the listed keyframes by rank: positions in the caller's list
    orbe::Dev dev{};
};

static void orbe_release(orbu_store* s)
{
    if (!s->correct) return;
    orbu_marks_drop(s, s->correct->dev.own);
    if (s->correct->d_block) (void)hipFree(s->correct->d_block);
    if (s->correct->d_kf) (void)hipFree(s->correct->d_kf);
    if (s->correct->d_pts) (void)hipFree(s->correct->d_pts);
    delete s->correct;
    s->correct = nullptr;
}

// (the pool's mutex is held) the fixed block, and the per-keyframe arrays for K keyframes
static int orbe_blocks_ensure(orbu_store* s, int K)
{
    orbw_pool* p = s->pool;
    if (!s->correct) {
        orbe_blocks* b = new orbe_blocks();
        Packer pk;
        const size_t oOwn = pk.take((size_t)p->cap * 8), marks = pk.off, oHdr = pk.take(orbe::H_INTS * 4), bytes = pk.off;
        if (int rc = orbu_block_once(p, b->d_block, bytes, 0)) { delete b; return rc; }
        b->dev.own = (unsigned long long*)(b->d_block + oOwn); b->dev.hdr = (int32_t*)(b->d_block + oHdr);
        b->dev.pool = p->dev;
        s->correct = b; s->marks[s->nMarks++] = {b->dev.own, marks};   // (the claim words)
    }
    orbe_blocks* b = s->correct;
    Packer pk;
    const size_t N = (size_t)K;
    const size_t oKf = pk.take(N * sizeof(orbe::KfRec)), oInv = pk.take(N * sizeof(orbe::Sim3)), oCnt = pk.take(N * 4), oStart = pk.take(N * 4);
    int rc = grow_device(b->d_kf, b->kfCap, pk.off, 1 << 12, &p->stream, &p->h->nDevAlloc);
    if (rc) return rc;
    b->dev.kf = (orbe::KfRec*)(b->d_kf + oKf); b->dev.inv = (orbe::Sim3*)(b->d_kf + oInv); b->dev.rowCnt = (int32_t*)(b->d_kf + oCnt); b->dev.rowStart = (int32_t*)(b->d_kf + oStart);
    b->dev.refKf = s->d_refKf; b->dev.ctr = s->ctr.d;
    return ORBX_OK;
}

// (the pool's mutex is held) the per-point arrays for n moved points
static int orbe_points_ensure(orbu_store* s, int n)
{
    orbw_pool* p = s->pool;
    orbe_blocks* b = s->correct;
    Packer pk;
    const size_t N = (size_t)n;
    const size_t oIds = pk.take(N * 4), oRank = pk.take(N * 4), oIdx = pk.take(N * 4), oRef = pk.take(N * 4), oPos = pk.take(N * 12), oOut = pk.take(N * sizeof(OrbePoint));
    int rc = grow_device(b->d_pts, b->ptsCap, pk.off, 1 << 16, &p->stream, &p->h->nDevAlloc);
    if (rc) return rc;
    b->dev.ids = (int32_t*)(b->d_pts + oIds); b->dev.ownerRank = (int32_t*)(b->d_pts + oRank); b->dev.ownerIdx = (int32_t*)(b->d_pts + oIdx);
    b->dev.ref = (int32_t*)(b->d_pts + oRef); b->dev.newPos = (float*)(b->d_pts + oPos); b->dev.out = (uint32_t*)(b->d_pts + oOut);
    return ORBX_OK;
}

extern "C" int orbe_correct_sim3(orbu_store_t* s, const int32_t* slots, const float* Tiw, int K, int anchor, const double* Scw, const int32_t* skip_ids, int n_skip,
                                 const float* scale_factors, int nlevels, int commit, OrbeKeyFrame* out_kf, OrbePoint* out_pts, int pts_cap, int* n_pts)
{
    if (K < 0 || n_skip < 0 || pts_cap < 0) return fail(ORBX_E_INVALID, "negative count");
    if (!slots || !Tiw || !Scw || !scale_factors || !out_kf || !n_pts || (n_skip > 0 && !skip_ids) || (pts_cap > 0 && !out_pts)) return fail(ORBX_E_INVALID, "null argument");
    if (K == 0) return fail(ORBX_E_INVALID, "no keyframe listed");
    if (anchor < 0 || anchor >= K) return fail(ORBX_E_INVALID, "anchor %d outside [0, %d)", anchor, K);
    if (nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d]", nlevels, ORBX_MAX_LEVELS);
    for (size_t i = 0; i < 12 * (size_t)K; i++)
        if (!std::isfinite(Tiw[i])) return fail(ORBX_E_INVALID, "Tiw[%zu] is not finite", i);
    for (int i = 0; i < 8; i++)
        if (!std::isfinite(Scw[i])) return fail(ORBX_E_INVALID, "Scw[%d] is not finite", i);
    if (!(Scw[7] > 0)) return fail(ORBX_E_INVALID, "the scale of Scw is %g", Scw[7]);
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    {   // the listed slots: set, and none twice (the store's scratch bits, all zero between calls); the fault at the lower index is reported
        int nOk = 0;
        while (nOk < K && !(rc = orbu_check_slot(s, "slots", nOk, slots[nOk], true))) nOk++;
        const int dup = first_repeated_key(slots, nOk, s->kfSeen);
        if (dup >= 0) return fail(ORBX_E_INVALID, "slots[%d] = %d is repeated within the call", dup, slots[dup]);
        if (rc) return rc;
    }
    if ((rc = orbw_check_ids(p, "skip_ids", skip_ids, n_skip, false))) return rc;
    if ((rc = orbu_check_columns(s, false, true, true))) return rc;
    if ((rc = orbe_blocks_ensure(s, K))) return rc;
    orbe_blocks* b = s->correct;
    Packer pk;
    const size_t oSlots = pk.take((size_t)K * 4), oTiw = pk.take((size_t)K * 48), oScw = pk.take(64), oSkip = pk.take((size_t)n_skip * 4), oSf = pk.take(ORBX_MAX_LEVELS * 4),
                 oHdr = pk.take(orbe::H_INTS * 4), oHdrR = pk.take(orbr::H_INTS * 4), oKf = pk.take((size_t)K * sizeof(OrbeKeyFrame));
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, pk.off))) return rc;
    hipStream_t st = p->stream;
    if ((rc = orbu_next_generation(s, st, &b->dev.gen))) return rc;
    // rule 1: ascending slot
    b->order.resize((size_t)K);
    for (int i = 0; i < K; i++) b->order[(size_t)i] = i;
    std::sort(b->order.begin(), b->order.end(), [=](int32_t x, int32_t y) { return slots[x] < slots[y]; });
    int32_t* hSlots = (int32_t*)(s->h_stage + oSlots);
    float* hTiw = (float*)(s->h_stage + oTiw);
    orbe::Call c{};
    for (int r = 0; r < K; r++) {
        const int i = b->order[(size_t)r];
        hSlots[r] = slots[i];
        memcpy(hTiw + 12 * (size_t)r, Tiw + 12 * (size_t)i, 48);
        if (i == anchor) c.anchorRank = r;
    }
    memcpy(s->h_stage + oScw, Scw, 64);
    if (n_skip) memcpy(s->h_stage + oSkip, skip_ids, (size_t)n_skip * 4);
    memset(s->h_stage + oSf, 0, ORBX_MAX_LEVELS * 4);
    memcpy(s->h_stage + oSf, scale_factors, (size_t)nlevels * 4);
    c.slots = hSlots; c.Tiw = hTiw; c.Scw = (const double*)(s->h_stage + oScw); c.skip = (const int32_t*)(s->h_stage + oSkip);
    c.K = K; c.nSkip = n_skip;
    int32_t* hdr = (int32_t*)(s->h_stage + oHdr);
    int32_t* hdrR = (int32_t*)(s->h_stage + oHdrR);
    const unsigned kfBlocks = (unsigned)((std::max(K, n_skip) + orbe::kThreads - 1) / orbe::kThreads);
    const unsigned rowBlocks = (unsigned)((K + orbe::kWaves - 1) / orbe::kWaves);
    hipLaunchKernelGGL(orbe::k_poses, dim3(kfBlocks), dim3(orbe::kThreads), 0, st, b->dev, c);
    hipLaunchKernelGGL(orbe::k_claim, dim3(rowBlocks), dim3(orbe::kThreads), 0, st, s->dev, b->dev, c);
    hipLaunchKernelGGL(orbe::k_rows, dim3(rowBlocks), dim3(orbe::kThreads), 0, st, s->dev, b->dev, c, 0, 0);
    hipLaunchKernelGGL(orbe::k_scan, dim3(1), dim3(orbe::kThreads), 0, st, b->dev, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hdr, b->dev.hdr, orbe::H_INTS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const int n = hdr[orbe::H_TOTAL];
    if (n < 0 || n > p->cap || (size_t)n > (size_t)K * s->pitch) return fail(ORBX_E_HIP, "the ownership walk counts %d moved points", n);
    if (n > pts_cap) { *n_pts = n; return fail(ORBX_E_CAPACITY, "%d moved points for a buffer of %d", n, pts_cap); }
    if (n) {
        if ((rc = orbe_points_ensure(s, n))) return rc;
        if ((rc = orbr_blocks_ensure(s, n))) return rc;
        orbr_blocks* rb = s->refresh;
        rb->dev.gen = b->dev.gen;
        orbr::Call rcall{};
        rcall.ids = b->dev.ids; rcall.ref = b->dev.ref; rcall.newPos = b->dev.newPos; rcall.sf = (const float*)(s->h_stage + oSf);
        rcall.n = n; rcall.what = ORBR_NORMAL_DEPTH; rcall.nlevels = nlevels;
        const unsigned ptBlocks = (unsigned)((n + orbe::kThreads - 1) / orbe::kThreads);
        hipLaunchKernelGGL(orbe::k_rows, dim3(rowBlocks), dim3(orbe::kThreads), 0, st, s->dev, b->dev, c, 1, n);
        hipLaunchKernelGGL(orbe::k_move, dim3(ptBlocks), dim3(orbe::kThreads), 0, st, b->dev, n, K);
        // rule 5: every centre it reads is the store's present one, which orbr's kernels read; the commit comes behind them
        orbr_issue(s, rb, rcall, st);
        hipLaunchKernelGGL(orbe::k_records, dim3(ptBlocks), dim3(orbe::kThreads), 0, st, b->dev, (const uint32_t*)rb->dev.res, (const int32_t*)hSlots, n, K);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hdrR, rb->dev.hdr, orbr::H_INTS * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if ((rc = orbr_check_header(hdrR, n, rb, "a moved point"))) return rc;
    }
    if (commit) {
        hipLaunchKernelGGL(orbe::k_commit, dim3((unsigned)((std::max(n, K) + orbe::kThreads - 1) / orbe::kThreads)), dim3(orbe::kThreads), 0, st, s->dev, b->dev,
                           (const int32_t*)hSlots, n, K);
        HIPCHK(hipGetLastError());
    }
    OrbeKeyFrame* hKf = (OrbeKeyFrame*)(s->h_stage + oKf);
    HIPCHK(hipMemcpyAsync(hKf, b->dev.kf, (size_t)K * sizeof(OrbeKeyFrame), hipMemcpyDeviceToHost, st));
    if (n) HIPCHK(hipMemcpyAsync(out_pts, b->dev.out, (size_t)n * sizeof(OrbePoint), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    for (int r = 0; r < K; r++) out_kf[b->order[(size_t)r]] = hKf[r];   // (the caller's order)
    *n_pts = n;
    return ORBX_OK;
}
