// orbt_bow_host.inc -- the BoW side of the Tracking-shaped path on a frame set (part of orbslamm_hip.hip):
// Frame::ComputeBoW (Frame.cc:394-402) for a batch of slots in two launches and SearchByBoW(KeyFrame, Frame)
// (ORBmatcher.cc:159-290, Tracking::TrackReferenceKeyFrame, Tracking.cc:805-812) for a batch of slot pairs in two
// launches; FeatureVectors never leave HBM, no node list visits the host, match tables land in pinned host memory.

struct orbm_frameset_bow {
    uint8_t* d_block = nullptr;
    uint32_t *d_word = nullptr, *d_node = nullptr; double* d_w = nullptr;
    uint32_t* d_outWord = nullptr; double* d_outW = nullptr;
    uint32_t* d_fvNode = nullptr; int32_t *d_fvStart = nullptr, *d_fvIdx = nullptr, *d_counts = nullptr;
    uint8_t* d_zero = nullptr; size_t zeroBytes = 0;     // matched[S][C]: cleared before every search
    uint8_t* d_matched = nullptr; int32_t* d_match = nullptr; uint8_t* d_binOf = nullptr;
    uint8_t* h_block = nullptr; int32_t* h_match = nullptr; int32_t* h_n = nullptr;   // pinned, one share per result set
    ResultRing res;   // (searches that write no flags and are never run again)
    int maxNodes = 0, P = 2;
    bool computed = false;
    std::vector<uint64_t> slotVoc;   // per slot: serial of the vocabulary that last transformed it (0: none)
    void* d_gkeys = nullptr;   // sort scratch of the memory form (frames of more than 8192 features)
};

static void frameset_bow_free(orbm_frameset* fs)
{
    orbm_frameset_bow* b = fs->bow;
    if (!b) return;
    if (b->d_block) (void)hipFree(b->d_block);
    if (b->d_gkeys) (void)hipFree(b->d_gkeys);
    if (b->h_block) (void)hipHostFree(b->h_block);
    b->res.destroy();
    delete b;
    fs->bow = nullptr;
}

static int frameset_bow_alloc(orbm_frameset* fs)
{
    if (fs->bow) return ORBX_OK;
    orbm_frameset_bow* b = new orbm_frameset_bow;
    const size_t S = (size_t)fs->slots, C = (size_t)fs->cap;
    Packer pk;
    const size_t oWd = pk.take(S * C * 4), oNd = pk.take(S * C * 4), oW = pk.take(S * C * 8), oOw = pk.take(S * C * 4), oOv = pk.take(S * C * 8);
    const size_t oFn = pk.take(S * C * 4), oFs = pk.take(S * (C + 1) * 4), oFi = pk.take(S * C * 4), oCt = pk.take(S * 8);
    const size_t oMa = pk.take(S * C), oMt = pk.take(S * C * 4), oBn = pk.take(S * C);
    Packer hp;
    const size_t hM = hp.take(ResultRing::kSets * S * C * 4), hN = hp.take(ResultRing::kSets * S * 4);
    if (hipMalloc(&b->d_block, pk.off) != hipSuccess || hipHostMalloc(&b->h_block, hp.off, hipHostMallocDefault) != hipSuccess) {
        if (b->d_block) (void)hipFree(b->d_block);
        delete b;
        return fail(ORBX_E_HIP, "cannot allocate the frame set's BoW arrays");
    }
    uint8_t* d = b->d_block;
    b->d_word = (uint32_t*)(d + oWd); b->d_node = (uint32_t*)(d + oNd); b->d_w = (double*)(d + oW);
    b->d_outWord = (uint32_t*)(d + oOw); b->d_outW = (double*)(d + oOv);
    b->d_fvNode = (uint32_t*)(d + oFn); b->d_fvStart = (int32_t*)(d + oFs); b->d_fvIdx = (int32_t*)(d + oFi); b->d_counts = (int32_t*)(d + oCt);
    b->d_zero = d + oMa; b->zeroBytes = oMt - oMa;
    b->d_matched = d + oMa; b->d_match = (int32_t*)(d + oMt); b->d_binOf = d + oBn;
    b->h_match = (int32_t*)(b->h_block + hM); b->h_n = (int32_t*)(b->h_block + hN);
    while (b->P < fs->cap) b->P <<= 1;
    b->slotVoc.assign(S, 0);
    fs->bow = b;   // (owned by the set from here: a failure below leaves it to orbm_frameset_destroy)
    HIPCHK(hipMemsetAsync(b->d_counts, 0, S * 8, fs->owner->stream));
    return ORBX_OK;
}

// Frame::ComputeBoW for slots (slot0 + i) % slots, i < n; asynchronous.  BowVectors stay in HBM until asked for
// (orbm_frameset_bow_vector: the KeyFrame database and the relocaliser read them), FeatureVectors stay for good.
extern "C" int orbm_frameset_compute_bow(orbm_frameset_t* fs, orbv_t* voc, int slot0, int n, int levelsup)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!voc || voc->device != fs->device) return fail(ORBX_E_INVALID, "vocabulary and frame set must share the device");
    if (slot0 < 0 || slot0 >= fs->slots || n < 0 || n > fs->slots) return fail(ORBX_E_INVALID, "bad argument");
    if ((rc = frameset_bow_alloc(fs))) return rc;
    orbm_frameset_bow* b = fs->bow;
    for (int i = 0; i < n; i++) b->slotVoc[(size_t)((slot0 + i) % fs->slots)] = voc->serial;
    if (n == 0) return ORBX_OK;
    if (voc->nWords == 0) { b->computed = true; return ORBX_OK; }   // an empty vocabulary: empty BowVectors, searches match nothing
    orbm_handle* h = fs->owner;
    const int nidLevel = voc->L - levelsup;
    // (the most over every transform of this set: slots transformed earlier with another levelsup / vocabulary keep their nodes)
    // + 1: in a ragged tree the features whose word is a leaf ABOVE that level keep node id 0 (DBoW2's `*nid = 0`), one more
    // FeatureVector node than the level has -- without it the node with the highest id was never searched (found by
    // tests/soak/fuzz_tracking.py: one match in 420 missing)
    b->maxNodes = std::max(b->maxNodes, std::min(fs->cap, (nidLevel <= 0 ? 1 : (nidLevel < (int)voc->nodesAtLevel.size() ? voc->nodesAtLevel[nidLevel] : 1)) + 1));
    orbv::VocDev v{voc->d_childStart, voc->d_childIdx, voc->d_desc, voc->d_wordId, voc->d_weight, voc->L, voc->scoring, voc->weighting};
    orbv::VocSetArgs a{};
    a.desc = fs->fs.desc; a.n = fs->fs.n; a.cap = fs->cap; a.slot0 = slot0; a.slotMod = fs->slots; a.P = b->P;
    a.word = b->d_word; a.node = b->d_node; a.w = b->d_w; a.outWord = b->d_outWord; a.outW = b->d_outW;
    a.fvNode = b->d_fvNode; a.fvStart = b->d_fvStart; a.fvIdx = b->d_fvIdx; a.counts = b->d_counts;
    hipLaunchKernelGGL(orbv::k_voc_descend_set, dim3((fs->cap + 63) / 64, n), dim3(64), 0, h->stream, v, a, levelsup);
    if (b->P > 8192) {   // frames beyond the LDS form of the sort: scratch in memory, one block per slot (allocated at the first such call)
        if (!b->d_gkeys) HIPCHK(hipMalloc(&b->d_gkeys, (size_t)fs->slots * b->P * 12));
        a.gkeys = (uint64_t*)b->d_gkeys;
        hipLaunchKernelGGL(orbv::k_voc_aggregate_set_mem, dim3(n), dim3(orbv::kAggThreads), 0, h->stream, v, a);
        HIPCHK(hipGetLastError());
        b->computed = true;
        return ORBX_OK;
    }
    const bool accLds = b->P <= 4096;
    const size_t lds = (size_t)b->P * (accLds ? 36 : 12);
    auto kern = accLds ? orbv::k_voc_aggregate_set<true> : orbv::k_voc_aggregate_set<false>;
    if (lds > 48 * 1024 && lds > h->ldsAttr[accLds ? 5 : 6]) {
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        h->ldsAttr[accLds ? 5 : 6] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(n), dim3(orbv::kAggThreads), lds, h->stream, v, a);
    HIPCHK(hipGetLastError());
    b->computed = true;
    return ORBX_OK;
}

// mBowVec of one slot (word id ascending, value) for the host; waits for the slot's transform
extern "C" int orbm_frameset_bow_vector(orbm_frameset_t* fs, int slot, uint32_t* word_id, double* word_value, int cap, int* n_words)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!fs->bow || !fs->bow->computed) return fail(ORBX_E_INVALID, "orbm_frameset_compute_bow has not run");
    if (slot < 0 || slot >= fs->slots || !n_words) return fail(ORBX_E_INVALID, "bad argument");
    orbm_frameset_bow* b = fs->bow;
    hipStream_t s = fs->owner->stream;
    int32_t counts[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(counts, b->d_counts + 2 * slot, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_words = counts[0];
    if (counts[0] > cap) return fail(ORBX_E_CAPACITY, "%d words, caller capacity %d", counts[0], cap);
    if (counts[0] && word_id) HIPCHK(hipMemcpyAsync(word_id, b->d_outWord + (size_t)slot * fs->cap, (size_t)counts[0] * 4, hipMemcpyDeviceToHost, s));
    if (counts[0] && word_value) HIPCHK(hipMemcpyAsync(word_value, b->d_outW + (size_t)slot * fs->cap, (size_t)counts[0] * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

// SearchByBoW(KeyFrame = slot kf[p], Frame = slot fr[p], vpMapPointMatches) for npairs pairs; every KeyFrame feature
// counts as holding a good MapPoint.  Asynchronous; match[p * cap + t] = KeyFrame feature for Frame feature t, or -1.
extern "C" int orbm_bow_frames(orbm_frameset_t* fs, const int32_t* kf_slots, const int32_t* frame_slots, int npairs, float nnratio, int check_ori)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!fs->bow || !fs->bow->computed) return fail(ORBX_E_INVALID, "orbm_frameset_compute_bow has not run");
    if (npairs < 0 || npairs > fs->slots || (npairs && (!kf_slots || !frame_slots))) return fail(ORBX_E_INVALID, "bad argument");
    for (int p = 0; p < npairs; p++)
        if (kf_slots[p] < 0 || kf_slots[p] >= fs->slots || frame_slots[p] < 0 || frame_slots[p] >= fs->slots) return fail(ORBX_E_INVALID, "slot outside the frame set");
    orbm_frameset_bow* b = fs->bow;
    orbm_handle* h = fs->owner;
    const int set = b->res.next();
    if ((rc = b->res.begin(set))) return rc;
    if (npairs) {
        const size_t S = (size_t)fs->slots, C = (size_t)fs->cap;
        HIPCHK(hipMemsetAsync(b->d_zero, 0, b->zeroBytes, h->stream));
        HIPCHK(hipMemsetAsync(b->d_match, 0xFF, (size_t)npairs * C * 4, h->stream));
        orbm::BowSetArgs a{};
        a.desc = fs->fs.desc; a.ang = fs->fs.ang; a.n = fs->fs.n; a.cap = fs->cap;
        a.fvNode = b->d_fvNode; a.fvStart = b->d_fvStart; a.fvIdx = b->d_fvIdx; a.counts = b->d_counts;
        a.nnratio = nnratio; a.thLow = 50; a.checkOri = check_ori;
        for (int p0 = 0; p0 < npairs; p0 += orbm::kBowMaxPairs) {
            const int nb = std::min(orbm::kBowMaxPairs, npairs - p0);
            a.matched = b->d_matched + p0 * C; a.match = b->d_match + p0 * C; a.binOf = b->d_binOf + p0 * C;
            for (int i = 0; i < nb; i++) { a.kf[i] = (int16_t)kf_slots[p0 + i]; a.fr[i] = (int16_t)frame_slots[p0 + i]; }
            hipLaunchKernelGGL(orbm::k_bow_set, dim3(std::max(b->maxNodes, 1), nb), dim3(64), 0, h->stream, a);
            hipLaunchKernelGGL(orbm::k_bow_prune_set, dim3(nb), dim3(256), 0, h->stream, a, b->h_match + (set * S + p0) * C, b->h_n + set * S + p0);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(b->res.rec[set].ev, h->stream));
    b->res.commit(set, ResultRecord::kNone, npairs, 0);
    return ORBX_OK;
}

extern "C" int orbm_bow_results(orbm_frameset_t* fs, int back, const int32_t** match, const int32_t** nmatches, int* npairs, int* cap)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (!fs->bow || back < 0 || back >= ResultRing::kSets) return fail(ORBX_E_INVALID, "bad argument");
    orbm_frameset_bow* b = fs->bow;
    const int set = b->res.back(back);
    const ResultRecord& r = b->res.rec[set];
    if (!r.ev) return fail(ORBX_E_INVALID, "no such search has been issued");
    HIPCHK(hipEventSynchronize(r.ev));
    const size_t S = (size_t)fs->slots, C = (size_t)fs->cap;
    if (match) *match = b->h_match + set * S * C;
    if (nmatches) *nmatches = b->h_n + set * S;
    if (npairs) *npairs = r.pairs;
    if (cap) *cap = fs->cap;
    return ORBX_OK;
}

#ifdef ORBT_PHASE_TIMING
extern "C" int orbv_debug_phase_times(double* us, int n)
{
    unsigned long long t[16];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(t, HIP_SYMBOL(orbv::g_orbvPhase), sizeof t));
    for (int i = 0; i < n && i < 15; i++) us[i] = (double)(t[i + 1] - t[i]) * 0.01;
    return ORBX_OK;
}
#endif
