// orbn_host.inc -- host side of the covisibility entries over a keyframe store (part of orbslamm_hip.hip; kernels:
// orbn_kernels.hip, ABI: include/orbslamm_covis.h, DESIGN.md §8u).
//   the blocks    made at the first orbn call of a store, of fixed size: the pool-sized marks, the chunk's counter matrix and
//                 keys on the device, the chunk's rows in pinned memory; the histograms at the first culling call.  The result
//                 arrays are host vectors that keep their capacity.  This file owns these and nothing of the store's: the octave
//                 column it reads is made by orbu_kf_set_octaves (orbu_host.inc) and freed by orbu_store_destroy
//   a call        targets kChunk at a time, each chunk under a generation tag of its own (the store's counter, shared with
//                 orbu_update_local_map, whose scratch a larger tag leaves valid).  The tag, the slot checks and the writer's
//                 opening: orbx_poolutil.inc

static_assert(ORBN_MAX_OCTAVE_VALUES == orbn::kBins, "orbslamm_covis.h constants");

constexpr int64_t kCovisMaxRowTotal = (int64_t)1 << 28;   // pairs in all rows of one call

struct orbn_blocks {
    uint8_t* d_block = nullptr;     // marks | counter matrix | keys
    uint32_t* d_hist = nullptr;
    uint8_t* h_rows = nullptr;      // pinned, coherent: header | cntKf | cntW | ordKf | ordW of one chunk
    orbn::Dev dev{};
    orbn::ChunkOut out{};
    std::vector<int32_t> status, kfMax, nMax, cntStart, cntKf, cntW, ordStart, ordKf, ordW;
};

static void orbn_release(orbu_store* s)
{
    if (!s->covis) return;
    orbu_marks_drop(s, s->covis->dev.mark);
    if (s->covis->d_block) (void)hipFree(s->covis->d_block);
    if (s->covis->d_hist) (void)hipFree(s->covis->d_hist);
    if (s->covis->h_rows) (void)hipHostFree(s->covis->h_rows);
    delete s->covis;
    s->covis = nullptr;
}

// (the pool's mutex is held)
static int orbn_blocks_ensure(orbu_store* s, bool hist)
{
    orbw_pool* p = s->pool;
    if (!s->covis) {
        orbn_blocks* b = new orbn_blocks();
        const size_t P = (size_t)p->cap, R = (size_t)orbn::kChunk * s->kfcap;
        Packer pk;
        const size_t oMark = pk.take(P * 8), oCnt = pk.take(R * 4), oKeys = pk.take(R * 8), bytes = pk.off;
        Packer hp;
        const size_t hHdr = hp.take((size_t)orbn::kChunk * orbn::C_INTS * 4), hCk = hp.take(R * 4), hCw = hp.take(R * 4), hOk = hp.take(R * 4),
                     hOw = hp.take(R * 4), hbytes = hp.off;
        if (int rc = orbu_block_once(p, b->d_block, bytes, 0)) { delete b; return rc; }
        HIPCHK_OR(hipHostMalloc((void**)&b->h_rows, hbytes, hipHostMallocCoherent), ((void)hipFree(b->d_block), delete b));
        memset(b->h_rows, 0, hbytes);
        b->dev.mark = (unsigned long long*)(b->d_block + oMark); b->dev.cnt = (int32_t*)(b->d_block + oCnt);
        b->dev.keys = (unsigned long long*)(b->d_block + oKeys);
        b->dev.poolFlags = p->dev.flags; b->dev.poolCap = p->cap;
        b->out.hdr = (int32_t*)(b->h_rows + hHdr); b->out.cntKf = (int32_t*)(b->h_rows + hCk); b->out.cntW = (int32_t*)(b->h_rows + hCw);
        b->out.ordKf = (int32_t*)(b->h_rows + hOk); b->out.ordW = (int32_t*)(b->h_rows + hOw);
        p->h->nHostAlloc++;
        s->covis = b; s->marks[s->nMarks++] = {b->dev.mark, P * 8};
    }
    if (hist && !s->covis->d_hist) {
        HIPCHK(hipMalloc((void**)&s->covis->d_hist, (size_t)p->cap * orbn::kBins * 4));
        p->h->nDevAlloc++;
    }
    s->covis->dev.hist = s->covis->d_hist;
    s->covis->dev.oct = s->oct.d;
    return ORBX_OK;
}

// what both entries check alike; 1: K == 0, nothing to do
static int orbn_check_call(orbu_store* s, const int32_t* targets, int K, int th, const void* result, const char* thName)
{
    if (!result) return fail(ORBX_E_INVALID, "null argument");
    if (K < 0) return fail(ORBX_E_INVALID, "negative count");
    if (K == 0) return 1;
    if (!targets) return fail(ORBX_E_INVALID, "null argument");
    if (th < 0) return fail(ORBX_E_INVALID, "%s %d", thName, th);
    if (K > ORBU_MAX_KEYFRAMES) return fail(ORBX_E_UNSUPPORTED, "%d targets: above %d", K, ORBU_MAX_KEYFRAMES);
    return orbu_store_check(s);
}

// (the pool's mutex is held)
static int orbn_check_targets(const orbu_store* s, const int32_t* targets, int K)
{
    int rc = ORBX_OK;
    for (int i = 0; i < K && !rc; i++) rc = orbu_check_slot(s, "targets", i, targets[i], true);
    return rc;
}

extern "C" int orbn_update_connections(orbu_store_t* s, const int32_t* targets, int K, int th, OrbnConnections* result)
{
    int rc = orbn_check_call(s, targets, K, th, result, "th");
    if (rc == 1) { memset(result, 0, sizeof *result); return ORBX_OK; }
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbn_check_targets(s, targets, K))) return rc;
    if ((rc = orbn_blocks_ensure(s, false))) return rc;
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, (size_t)K * 4))) return rc;
    orbn_blocks* b = s->covis;
    hipStream_t st = p->stream;
    memcpy(s->h_stage, targets, (size_t)K * 4);
    const int32_t* tg = (const int32_t*)s->h_stage;
    b->status.resize((size_t)K); b->kfMax.resize((size_t)K); b->nMax.resize((size_t)K);
    b->cntStart.assign((size_t)K + 1, 0); b->ordStart.assign((size_t)K + 1, 0);
    b->cntKf.clear(); b->cntW.clear(); b->ordKf.clear(); b->ordW.clear();
    const unsigned walkBlocks = (unsigned)((s->hi + orbn::kWaves - 1) / orbn::kWaves);
    for (int c0 = 0; c0 < K; c0 += orbn::kChunk) {
        const int nC = std::min(orbn::kChunk, K - c0);
        if ((rc = orbu_next_generation(s, st, &b->dev.gen))) return rc;
        hipLaunchKernelGGL(orbn::k_mark, dim3((unsigned)nC), dim3(orbn::kThreads), 0, st, s->dev, b->dev, tg + c0, 0);
        hipLaunchKernelGGL(orbn::k_conn_walk, dim3(walkBlocks), dim3(orbn::kThreads), 0, st, s->dev, b->dev, tg + c0, nC, s->hi);
        hipLaunchKernelGGL(orbn::k_conn_select, dim3((unsigned)nC), dim3(orbn::kThreads), 0, st, s->dev, b->dev, s->hi, th, b->out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));   // (the rows are the next chunk's)
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        for (int c = 0; c < nC; c++) {
            const int32_t* h = b->out.hdr + c * orbn::C_INTS;
            const int nCnt = h[orbn::C_NCNT], nOrd = h[orbn::C_NORD];
            const size_t r0 = (size_t)c * s->kfcap;
            if (nCnt < 0 || nCnt > s->kfcap || nOrd < 0 || nOrd > s->kfcap) return fail(ORBX_E_HIP, "a row of %d and %d members from a store of %d", nCnt, nOrd, s->kfcap);
            if ((int64_t)b->cntKf.size() + nCnt > kCovisMaxRowTotal)
                return fail(ORBX_E_CAPACITY, "more than %lld connections in one call: give fewer targets", (long long)kCovisMaxRowTotal);
            b->status[c0 + c] = h[orbn::C_STATUS]; b->kfMax[c0 + c] = h[orbn::C_KFMAX]; b->nMax[c0 + c] = h[orbn::C_NMAX];
            b->cntKf.insert(b->cntKf.end(), b->out.cntKf + r0, b->out.cntKf + r0 + nCnt);
            b->cntW.insert(b->cntW.end(), b->out.cntW + r0, b->out.cntW + r0 + nCnt);
            b->ordKf.insert(b->ordKf.end(), b->out.ordKf + r0, b->out.ordKf + r0 + nOrd);
            b->ordW.insert(b->ordW.end(), b->out.ordW + r0, b->out.ordW + r0 + nOrd);
            b->cntStart[c0 + c + 1] = (int32_t)b->cntKf.size(); b->ordStart[c0 + c + 1] = (int32_t)b->ordKf.size();
        }
    }
    result->K = K;
    result->status = b->status.data(); result->kf_max = b->kfMax.data(); result->n_max = b->nMax.data();
    result->cnt_start = b->cntStart.data(); result->cnt_kf = b->cntKf.data(); result->cnt_w = b->cntW.data();
    result->ord_start = b->ordStart.data(); result->ord_kf = b->ordKf.data(); result->ord_w = b->ordW.data();
    return ORBX_OK;
}

extern "C" int orbn_culling_counts(orbu_store_t* s, const int32_t* targets, int K, int th_obs, OrbnCulling* result)
{
    int rc = orbn_check_call(s, targets, K, th_obs, result, "th_obs");
    if (rc == 1) { memset(result, 0, sizeof *result); return ORBX_OK; }
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbn_check_targets(s, targets, K))) return rc;
    if ((rc = orbu_check_columns(s, false, false, true))) return rc;
    if ((rc = orbn_blocks_ensure(s, true))) return rc;
    Packer pk;
    const size_t oTg = pk.take((size_t)K * 4), oBin = pk.take(256), oUpto = pk.take(257), oMps = pk.take((size_t)K * 4), oRed = pk.take((size_t)K * 4),
                 oFlag = pk.take((size_t)K);
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, pk.off))) return rc;
    orbn_blocks* b = s->covis;
    hipStream_t st = p->stream;
    memcpy(s->h_stage + oTg, targets, (size_t)K * 4);
    {   // an octave byte -> its rank among the values the store holds; a level -> the largest rank at or below it
        uint8_t* bin = s->h_stage + oBin;
        int8_t* upto = (int8_t*)(s->h_stage + oUpto);
        int rank = -1;
        for (int v = 0; v < 256; v++) { if (s->octSeen[v]) rank++; bin[v] = (uint8_t)std::max(rank, 0); upto[v] = (int8_t)rank; }
        upto[256] = (int8_t)rank;
    }
    const int32_t* tg = (const int32_t*)(s->h_stage + oTg);
    int32_t* nMps = (int32_t*)(s->h_stage + oMps);
    int32_t* nRed = (int32_t*)(s->h_stage + oRed);
    const unsigned walkBlocks = (unsigned)((s->hi + orbn::kWaves - 1) / orbn::kWaves);
    for (int c0 = 0; c0 < K; c0 += orbn::kChunk) {
        const int nC = std::min(orbn::kChunk, K - c0);
        if ((rc = orbu_next_generation(s, st, &b->dev.gen))) return rc;
        hipLaunchKernelGGL(orbn::k_mark, dim3((unsigned)nC), dim3(orbn::kThreads), 0, st, s->dev, b->dev, tg + c0, 1);
        hipLaunchKernelGGL(orbn::k_hist_walk, dim3(walkBlocks), dim3(orbn::kThreads), 0, st, s->dev, b->dev, (const uint8_t*)(s->h_stage + oBin), s->hi);
        hipLaunchKernelGGL(orbn::k_cull, dim3((unsigned)nC), dim3(orbn::kThreads), 0, st, s->dev, b->dev, tg + c0, th_obs, (const int8_t*)(s->h_stage + oUpto),
                           nMps + c0, nRed + c0);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    uint8_t* red = s->h_stage + oFlag;
    for (int i = 0; i < K; i++) red[i] = (double)nRed[i] > 0.9 * (double)nMps[i] ? 1 : 0;   // LocalMapping.cc:695
    result->K = K; result->n_mps = nMps; result->n_redundant = nRed; result->redundant = red;
    return ORBX_OK;
}
