// orbk_host.inc -- host side of the keyframe database (part of orbslamm_hip.hip; kernels: orbk_kernels.hip, DESIGN.md §8g):
// ORBVocabulary::score, the keyframe pool (BowVectors in HBM + the six query fields of every KeyFrame), databases over a
// pool, DetectRelocalizationCandidates / DetectLoopCandidates, and MultiMapper::DetectLoop's scan as one batch.

// ------------------------------------------------------------------ ORBVocabulary::score (L1 only)
extern "C" int orbv_score(orbv_t* voc, const uint32_t* a_ids, const double* a_vals, int na,
                          const uint32_t* b_ids, const double* b_vals, int nb, double* out)
{
    if (!voc || !out || na < 0 || nb < 0 || (na && (!a_ids || !a_vals)) || (nb && (!b_ids || !b_vals))) return fail(ORBX_E_INVALID, "bad argument");
    if (voc->scoring != 0) return fail(ORBX_E_UNSUPPORTED, "scoring type %d: only L1_NORM (ORBvoc.txt's) is implemented", voc->scoring);
    for (int i = 1; i < na; i++) if (a_ids[i] <= a_ids[i - 1]) return fail(ORBX_E_INVALID, "word ids of v1 not ascending");
    for (int i = 1; i < nb; i++) if (b_ids[i] <= b_ids[i - 1]) return fail(ORBX_E_INVALID, "word ids of v2 not ascending");
    HIPCHK(hipSetDevice(voc->device));
    std::lock_guard<std::mutex> lk(voc->mu);
    Packer pk;
    const size_t oA = pk.take((size_t)na * 4), oAv = pk.take((size_t)na * 8), oB = pk.take((size_t)nb * 4), oBv = pk.take((size_t)nb * 8), oR = pk.take(8);
    int rc = orbv_reserve(voc, SV_SCORE, pk.off);
    if (rc) return rc;
    std::vector<uint8_t> h(pk.off, 0);
    if (na) { memcpy(&h[oA], a_ids, (size_t)na * 4); memcpy(&h[oAv], a_vals, (size_t)na * 8); }
    if (nb) { memcpy(&h[oB], b_ids, (size_t)nb * 4); memcpy(&h[oBv], b_vals, (size_t)nb * 8); }
    uint8_t* d = slot_ptr<uint8_t>(voc, SV_SCORE);
    HIPCHK(hipMemcpyAsync(d, h.data(), oR, hipMemcpyHostToDevice, voc->stream));
    hipLaunchKernelGGL(orbk::k_kf_score_one, dim3(1), dim3(64), 0, voc->stream, (const uint32_t*)(d + oA), (const double*)(d + oAv), na,
                       (const uint32_t*)(d + oB), (const double*)(d + oBv), nb, (double*)(d + oR));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d + oR, 8, hipMemcpyDeviceToHost, voc->stream));
    HIPCHK(hipStreamSynchronize(voc->stream));
    return ORBX_OK;
}

// ------------------------------------------------------------------ pool
constexpr int kKfMaxSlots = 1 << 24;

struct KBuf {   // device scratch that grows; freed only behind a stream sync (queued kernels may read it)
    void* p = nullptr; size_t cap = 0;
};

struct orbk_db;

struct orbk_pool {
    orbv_handle* voc = nullptr;
    int device = 0, nWords = 0;
    uint64_t vocSerial = 0;                      // the vocabulary's orbv_handle::serial
    hipStream_t stream = nullptr;
    hipEvent_t evIn = nullptr, evOut = nullptr;   // hand-over with a frame set's stream
    // every pool and database call holds it for its duration, as ORBVocabulary's transform holds the vocabulary's
    std::mutex mu;
    int n = 0, capSlots = 0;                     // slots in use (highest set + 1), slots allocated
    // per slot, preserved on growth
    int32_t *d_bowOff = nullptr, *d_bowLen = nullptr;
    uint64_t *d_relocQ = nullptr, *d_loopQ = nullptr;
    int32_t *d_relocW = nullptr, *d_loopW = nullptr;
    float *d_relocS = nullptr, *d_loopS = nullptr;
    int32_t *d_cov = nullptr, *d_covN = nullptr, *d_connMark = nullptr, *d_firstIdx = nullptr;
    // the arena of BowVectors
    // (append-only: a slot whose new BowVector fits its range reuses it, a larger one moves to the end and leaves the old
    // range unused; a frame set slot reserves the set's capacity, since its word count is known only on the device)
    uint32_t* d_ids = nullptr; double* d_vals = nullptr; size_t arenaCap = 0, arenaUsed = 0;
    std::vector<int32_t> hOff, hCap;             // per slot: its arena range (-1: none yet)
    // dense word table of the query (epoch-tagged)
    int32_t *d_wEpoch = nullptr, *d_wIdx = nullptr;
    int32_t epoch = 0;
    // scratch of the queries
    KBuf bPar, bMem, bScr, bOut;
    uint8_t* h_stage = nullptr; size_t h_stageCap = 0;   // pinned: parameters up, results down
    std::vector<orbk_db*> dbs;
};

struct orbk_db {
    orbk_pool* pool = nullptr;
    int nKFs = 0;                                // mnNumberOfKFs
    uint32_t nextSeq = 0;                        // insertion sequence of the next add
    std::vector<std::deque<uint32_t>> copies;    // per slot: the sequences of its live copies, earliest first
    bool dirty = true;
    int m = 0;                                   // members (slots with a live copy) in bMem
    KBuf bMem;
    std::vector<int32_t> lastSlots; std::vector<float> lastScores;   // lScoreAndMatch of the last single query
};

// (the stream is drained only where there is an old block that queued kernels may read)
static int kbuf_reserve(orbk_pool* p, KBuf& b, size_t bytes) { return grow_device(b.p, b.cap, bytes, 4096, b.p ? &p->stream : nullptr); }

// (copies from / into the old block may be in flight)
static int kf_stage(orbk_pool* p, size_t bytes) { return grow_pinned(p->h_stage, p->h_stageCap, bytes, false, &p->stream); }

template <class T>
static int kf_grow_array(orbk_pool* p, T*& a, size_t oldN, size_t newN, int fill)
{
    T* na = nullptr;
    HIPCHK(hipMalloc(&na, newN * sizeof(T)));
    HIPCHK(hipMemsetAsync(na, fill, newN * sizeof(T), p->stream));
    if (a && oldN) HIPCHK(hipMemcpyAsync(na, a, oldN * sizeof(T), hipMemcpyDeviceToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (a) HIPCHK(hipFree(a));
    a = na;
    return ORBX_OK;
}

static int kf_grow_slots(orbk_pool* p, int need)
{
    if (need <= p->capSlots) return ORBX_OK;
    const size_t o = (size_t)p->capSlots, c = (size_t)std::max(need, std::max(2 * p->capSlots, 1024));
    int rc;
    HIPCHK(hipStreamSynchronize(p->stream));
    if ((rc = kf_grow_array(p, p->d_bowOff, o, c, 0)) || (rc = kf_grow_array(p, p->d_bowLen, o, c, 0)) ||
        (rc = kf_grow_array(p, p->d_relocQ, o, c, 0)) || (rc = kf_grow_array(p, p->d_loopQ, o, c, 0)) ||
        (rc = kf_grow_array(p, p->d_relocW, o, c, 0)) || (rc = kf_grow_array(p, p->d_loopW, o, c, 0)) ||
        (rc = kf_grow_array(p, p->d_relocS, o, c, 0)) || (rc = kf_grow_array(p, p->d_loopS, o, c, 0)) ||
        (rc = kf_grow_array(p, p->d_cov, o * orbk::kNeigh, c * orbk::kNeigh, 0)) || (rc = kf_grow_array(p, p->d_covN, o, c, 0)) ||
        (rc = kf_grow_array(p, p->d_connMark, o, c, 0)) ||
        (rc = kf_grow_array(p, p->d_firstIdx, o, c, 0x7F)))   // 0x7F7F7F7F: above any list index ("at rest")
        return rc;
    p->capSlots = (int)c;
    return ORBX_OK;
}

static int kf_grow_arena(orbk_pool* p, size_t need)
{
    if (need <= p->arenaCap) return ORBX_OK;
    if (need > (size_t)INT32_MAX) return fail(ORBX_E_CAPACITY, "the pool's BowVector arena is limited to 2^31 entries");
    const size_t c = std::min<size_t>(std::max<size_t>(need, std::max<size_t>(2 * p->arenaCap, 1 << 16)), (size_t)INT32_MAX);
    int rc;
    HIPCHK(hipStreamSynchronize(p->stream));
    if ((rc = kf_grow_array(p, p->d_ids, p->arenaUsed, c, 0)) || (rc = kf_grow_array(p, p->d_vals, p->arenaUsed, c, 0))) return rc;
    p->arenaCap = c;
    return ORBX_OK;
}

static orbk::PoolDev kf_dev(orbk_pool* p)
{
    return {p->d_bowOff, p->d_bowLen, p->d_ids, p->d_vals, p->d_relocQ, p->d_relocW, p->d_relocS, p->d_loopQ, p->d_loopW, p->d_loopS,
            p->d_cov, p->d_covN, p->d_connMark, p->d_firstIdx, p->d_wEpoch, p->d_wIdx};
}

static int kf_next_epoch(orbk_pool* p)
{
    if (p->epoch == INT32_MAX) {   // (2^31 queries) the tags start over on cleared tables
        HIPCHK(hipStreamSynchronize(p->stream));
        HIPCHK(hipMemset(p->d_wEpoch, 0, (size_t)std::max(p->nWords, 1) * 4));
        HIPCHK(hipMemset(p->d_connMark, 0, (size_t)p->capSlots * 4));
        p->epoch = 0;
    }
    return ++p->epoch;
}

static bool kf_slot_in_db(orbk_pool* p, int slot)
{
    for (orbk_db* d : p->dbs) if (slot < (int)d->copies.size() && !d->copies[slot].empty()) return true;
    return false;
}

extern "C" void orbk_pool_destroy(orbk_pool_t* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (orbk_db* d : p->dbs) d->pool = nullptr;   // (databases outliving their pool refuse every call)
    void* ptrs[] = {p->d_bowOff, p->d_bowLen, p->d_relocQ, p->d_loopQ, p->d_relocW, p->d_loopW, p->d_relocS, p->d_loopS, p->d_cov, p->d_covN,
                    p->d_connMark, p->d_firstIdx, p->d_ids, p->d_vals, p->d_wEpoch, p->d_wIdx, p->bPar.p, p->bMem.p, p->bScr.p, p->bOut.p};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    if (p->evIn) (void)hipEventDestroy(p->evIn);
    if (p->evOut) (void)hipEventDestroy(p->evOut);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    live_remove(p);
    delete p;
}

extern "C" int orbk_pool_create(orbv_t* voc, int slots, orbk_pool_t** out)
{
    if (!voc || !out || slots < 0 || slots > kKfMaxSlots) return fail(ORBX_E_INVALID, "bad argument");
    *out = nullptr;
    if (voc->scoring != 0) return fail(ORBX_E_UNSUPPORTED, "scoring type %d: the keyframe database scores with L1_NORM only", voc->scoring);
    orbk_pool* p = new orbk_pool();
    p->voc = voc; p->device = voc->device; p->nWords = voc->nWords; p->vocSerial = voc->serial;
    HIPCHK_OR(hipSetDevice(p->device), orbk_pool_destroy(p));
    HIPCHK_OR(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking), orbk_pool_destroy(p));
    HIPCHK_OR(hipEventCreateWithFlags(&p->evIn, hipEventDisableTiming), orbk_pool_destroy(p));
    HIPCHK_OR(hipEventCreateWithFlags(&p->evOut, hipEventDisableTiming), orbk_pool_destroy(p));
    HIPCHK_OR(hipMalloc(&p->d_wEpoch, (size_t)std::max(p->nWords, 1) * 4), orbk_pool_destroy(p));
    HIPCHK_OR(hipMalloc(&p->d_wIdx, (size_t)std::max(p->nWords, 1) * 4), orbk_pool_destroy(p));
    HIPCHK_OR(hipMemset(p->d_wEpoch, 0, (size_t)std::max(p->nWords, 1) * 4), orbk_pool_destroy(p));
    HIPCHK_OR(hipMemset(p->d_wIdx, 0, (size_t)std::max(p->nWords, 1) * 4), orbk_pool_destroy(p));
    live_add(p);
    int rc = kf_grow_slots(p, std::max(slots, 1));
    if (!rc) rc = kf_grow_arena(p, 1);
    if (rc) { orbk_pool_destroy(p); return rc; }
    *out = p;
    return ORBX_OK;
}

static int kf_pool_check(orbk_pool* p)
{
    if (!p || !live_has(p)) return fail(ORBX_E_INVALID, "null or destroyed pool");
    HIPCHK(hipSetDevice(p->device));
    return ORBX_OK;
}

extern "C" int orbk_pool_size(orbk_pool_t* p, int* n)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    if (!n) return fail(ORBX_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(p->mu);
    *n = p->n;
    return ORBX_OK;
}

// a slot about to receive a BowVector: in range, in no database (its words are fixed while a list holds it)
static int kf_bow_slot(orbk_pool* p, int slot, int lenCap, int32_t* off)
{
    if (slot < 0 || slot >= kKfMaxSlots) return fail(ORBX_E_INVALID, "slot %d out of range", slot);
    if (slot < p->n && kf_slot_in_db(p, slot)) return fail(ORBX_E_INVALID, "slot %d is in a database: its BowVector is fixed until erased", slot);
    int rc;
    if ((rc = kf_grow_slots(p, slot + 1))) return rc;
    if (slot < (int)p->hOff.size() && p->hOff[slot] >= 0 && p->hCap[slot] >= lenCap) {   // the slot's range fits: reused
        *off = p->hOff[slot];
        return ORBX_OK;
    }
    if ((rc = kf_grow_arena(p, p->arenaUsed + (size_t)lenCap))) return rc;
    *off = (int32_t)p->arenaUsed;
    p->arenaUsed += (size_t)lenCap;
    if ((int)p->hOff.size() <= slot) { p->hOff.resize((size_t)slot + 1, -1); p->hCap.resize((size_t)slot + 1, 0); }
    p->hOff[slot] = *off;
    p->hCap[slot] = lenCap;
    p->n = std::max(p->n, slot + 1);
    return ORBX_OK;
}

extern "C" int orbk_pool_set_bow(orbk_pool_t* p, int slot, const uint32_t* ids, const double* vals, int n)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    if (n < 0 || (n && (!ids || !vals))) return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < n; i++)
        if ((int64_t)ids[i] >= p->nWords || (i && ids[i] <= ids[i - 1])) return fail(ORBX_E_INVALID, "word ids must ascend and lie below %d", p->nWords);
    std::lock_guard<std::mutex> lk(p->mu);
    int32_t off = 0;
    if ((rc = kf_bow_slot(p, slot, n, &off))) return rc;
    if (n) {
        HIPCHK(hipMemcpyAsync(p->d_ids + off, ids, (size_t)n * 4, hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipMemcpyAsync(p->d_vals + off, vals, (size_t)n * 8, hipMemcpyHostToDevice, p->stream));
    }
    const int32_t ol[2] = {off, n};
    HIPCHK(hipMemcpyAsync(p->d_bowOff + slot, &ol[0], 4, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_bowLen + slot, &ol[1], 4, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return ORBX_OK;
}

// the frame set's stream has enqueued the slot's BowVector: the pool's stream waits for it, and the frame set's stream
// waits for the pool's copy before anything it enqueues later may overwrite the slot
static int kf_copy_from_frameset(orbk_pool* p, orbm_frameset* fs, int fs_slot, uint32_t* dIds, double* dVals, int32_t* dLen, int cap)
{
    orbm_frameset_bow* b = fs->bow;
    hipStream_t fsS = fs->owner->stream;
    HIPCHK(hipEventRecord(p->evIn, fsS));
    HIPCHK(hipStreamWaitEvent(p->stream, p->evIn, 0));
    hipLaunchKernelGGL(orbk::k_kf_copy_bow, dim3((cap + 255) / 256), dim3(256), 0, p->stream, b->d_outWord + (size_t)fs_slot * fs->cap,
                       b->d_outW + (size_t)fs_slot * fs->cap, b->d_counts + 2 * fs_slot, cap, dIds, dVals, dLen);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->evOut, p->stream));
    HIPCHK(hipStreamWaitEvent(fsS, p->evOut, 0));
    return ORBX_OK;
}

static int kf_frameset_usable(orbk_pool* p, orbm_frameset* fs, int fs_slot)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (fs->device != p->device) return fail(ORBX_E_INVALID, "pool (device %d) and frame set (device %d) live on different devices", p->device, fs->device);
    if (!fs->bow || !fs->bow->computed) return fail(ORBX_E_INVALID, "orbm_frameset_compute_bow has not run");
    if (fs_slot < 0 || fs_slot >= fs->slots) return fail(ORBX_E_INVALID, "frame set slot %d out of range", fs_slot);
    // the slot's word ids index the pool's word table: they must come from the pool's vocabulary
    if (fs->bow->slotVoc[fs_slot] != p->vocSerial)
        return fail(ORBX_E_INVALID, "frame set slot %d was not transformed with the pool's vocabulary", fs_slot);
    return ORBX_OK;
}

extern "C" int orbk_pool_set_bow_from_frameset(orbk_pool_t* p, int slot, orbm_frameset_t* fs, int fs_slot)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    if ((rc = kf_frameset_usable(p, fs, fs_slot))) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    int32_t off = 0;
    if ((rc = kf_bow_slot(p, slot, fs->cap, &off))) return rc;
    HIPCHK(hipMemcpyAsync(p->d_bowOff + slot, &off, 4, hipMemcpyHostToDevice, p->stream));
    if ((rc = kf_copy_from_frameset(p, fs, fs_slot, p->d_ids + off, p->d_vals + off, p->d_bowLen + slot, fs->cap))) return rc;
    HIPCHK(hipStreamSynchronize(p->stream));   // (&off above is on this frame)
    return ORBX_OK;
}

extern "C" int orbk_pool_set_covisibility(orbk_pool_t* p, int slot, const int32_t* best, int n)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    if (n < 0 || n > orbk::kNeigh || (n && !best)) return fail(ORBX_E_INVALID, "bad argument (at most %d neighbours)", orbk::kNeigh);
    std::lock_guard<std::mutex> lk(p->mu);
    if (slot < 0 || slot >= p->n) return fail(ORBX_E_INVALID, "slot %d out of range", slot);
    int32_t row[orbk::kNeigh + 1] = {0};
    for (int i = 0; i < n; i++) {
        if (best[i] < 0 || best[i] >= p->n) return fail(ORBX_E_INVALID, "neighbour slot %d out of range", best[i]);
        row[i] = best[i];
    }
    row[orbk::kNeigh] = n;
    HIPCHK(hipMemcpyAsync(p->d_cov + (size_t)slot * orbk::kNeigh, row, orbk::kNeigh * 4, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_covN + slot, &row[orbk::kNeigh], 4, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return ORBX_OK;
}

extern "C" int orbk_pool_read_state(orbk_pool_t* p, uint64_t* reloc_query, int32_t* reloc_words, float* reloc_score,
                                    uint64_t* loop_query, int32_t* loop_words, float* loop_score, int cap)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(p->mu);
    if (cap < p->n) return fail(ORBX_E_CAPACITY, "%d slots, caller capacity %d", p->n, cap);
    const size_t n = (size_t)p->n;
    if (!n) return ORBX_OK;
    if (reloc_query) HIPCHK(hipMemcpyAsync(reloc_query, p->d_relocQ, n * 8, hipMemcpyDeviceToHost, p->stream));
    if (reloc_words) HIPCHK(hipMemcpyAsync(reloc_words, p->d_relocW, n * 4, hipMemcpyDeviceToHost, p->stream));
    if (reloc_score) HIPCHK(hipMemcpyAsync(reloc_score, p->d_relocS, n * 4, hipMemcpyDeviceToHost, p->stream));
    if (loop_query) HIPCHK(hipMemcpyAsync(loop_query, p->d_loopQ, n * 8, hipMemcpyDeviceToHost, p->stream));
    if (loop_words) HIPCHK(hipMemcpyAsync(loop_words, p->d_loopW, n * 4, hipMemcpyDeviceToHost, p->stream));
    if (loop_score) HIPCHK(hipMemcpyAsync(loop_score, p->d_loopS, n * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return ORBX_OK;
}

// float score = mpORBVocabulary->score(pKF->mBowVec, others[i]->mBowVec) for each i (LoopClosing.cc:127-147, MultiMapper.cc:140-152)
extern "C" int orbk_pool_score(orbk_pool_t* p, int slot, const int32_t* others, int n, float* out)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    if (n < 0 || (n && (!others || !out))) return fail(ORBX_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(p->mu);
    if (slot < 0 || slot >= p->n) return fail(ORBX_E_INVALID, "slot %d out of range", slot);
    for (int i = 0; i < n; i++) if (others[i] < 0 || others[i] >= p->n) return fail(ORBX_E_INVALID, "slot %d out of range", others[i]);
    if (!n) return ORBX_OK;
    Packer pk;
    const size_t oA = pk.take((size_t)n * 4), oB = pk.take((size_t)n * 4), oS = pk.take((size_t)n * 4);
    if ((rc = kbuf_reserve(p, p->bPar, pk.off)) || (rc = kf_stage(p, pk.off))) return rc;
    for (int i = 0; i < n; i++) ((int32_t*)(p->h_stage + oA))[i] = slot;
    memcpy(p->h_stage + oB, others, (size_t)n * 4);
    uint8_t* d = (uint8_t*)p->bPar.p;
    HIPCHK(hipMemcpyAsync(d, p->h_stage, oS, hipMemcpyHostToDevice, p->stream));
    hipLaunchKernelGGL(orbk::k_kf_score_pairs, dim3((n + 3) / 4), dim3(256), 0, p->stream, kf_dev(p), (const int32_t*)(d + oA), (const int32_t*)(d + oB), n, (float*)(d + oS));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(p->h_stage + oS, d + oS, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    memcpy(out, p->h_stage + oS, (size_t)n * 4);
    return ORBX_OK;
}

// ------------------------------------------------------------------ databases
extern "C" int orbk_db_create(orbk_pool_t* p, orbk_db_t** out)
{
    int rc = kf_pool_check(p);
    if (rc) return rc;
    if (!out) return fail(ORBX_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(p->mu);
    orbk_db* d = new orbk_db();
    d->pool = p;
    p->dbs.push_back(d);
    live_add(d);
    *out = d;
    return ORBX_OK;
}

extern "C" void orbk_db_destroy(orbk_db_t* d)
{
    if (!d || !live_has(d)) return;
    orbk_pool* p = d->pool;
    if (p && live_has(p)) {
        std::lock_guard<std::mutex> lk(p->mu);
        (void)hipSetDevice(p->device);
        (void)hipStreamSynchronize(p->stream);
        p->dbs.erase(std::remove(p->dbs.begin(), p->dbs.end(), d), p->dbs.end());
    }
    if (d->bMem.p) (void)hipFree(d->bMem.p);
    live_remove(d);
    delete d;
}

// every call on a database locks its pool
struct KfDbLock {
    orbk_db* d; orbk_pool* p = nullptr; std::unique_lock<std::mutex> lk; int rc = ORBX_OK;
    explicit KfDbLock(orbk_db* d_) : d(d_)
    {
        if (!d || !live_has(d)) { rc = fail(ORBX_E_INVALID, "null or destroyed database"); return; }
        p = d->pool;
        if ((rc = kf_pool_check(p))) return;
        lk = std::unique_lock<std::mutex>(p->mu);
    }
};

static int kf_db_slot(orbk_db* d, int slot)
{
    if (slot < 0 || slot >= d->pool->n) return fail(ORBX_E_INVALID, "slot %d out of range (pool of %d)", slot, d->pool->n);
    if ((int)d->copies.size() <= slot) d->copies.resize((size_t)d->pool->n);
    return ORBX_OK;
}

// void KeyFrameDatabase::add(KeyFrame*) (:41-48): one more copy under every word of the keyframe's BowVector
extern "C" int orbk_db_add(orbk_db_t* d, int slot)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    int rc = kf_db_slot(d, slot);
    if (rc) return rc;
    d->nKFs++;
    d->copies[slot].push_back(d->nextSeq++);
    d->dirty = true;
    return ORBX_OK;
}

// void KeyFrameDatabase::erase(KeyFrame*) (:50-73): the first occurrence per word = the earliest live copy
extern "C" int orbk_db_erase(orbk_db_t* d, int slot)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    int rc = kf_db_slot(d, slot);
    if (rc) return rc;
    if (d->nKFs > 0) d->nKFs--;
    if (!d->copies[slot].empty()) { d->copies[slot].pop_front(); d->dirty = true; }
    return ORBX_OK;
}

// void KeyFrameDatabase::clear() (:75-79): the lists empty, mnNumberOfKFs stays
extern "C" int orbk_db_clear(orbk_db_t* d)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    for (auto& q : d->copies) q.clear();
    d->dirty = true;
    return ORBX_OK;
}

extern "C" int orbk_db_size(orbk_db_t* d, int* n)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    if (!n) return fail(ORBX_E_INVALID, "bad argument");
    *n = d->nKFs;
    return ORBX_OK;
}

extern "C" int orbk_db_empty(orbk_db_t* d, int* empty)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    if (!empty) return fail(ORBX_E_INVALID, "bad argument");
    *empty = d->nKFs == 0;
    return ORBX_OK;
}

extern "C" int orbk_db_last_scored(orbk_db_t* d, int32_t* slots, float* scores, int cap, int* n)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    if (!n) return fail(ORBX_E_INVALID, "bad argument");
    const int k = (int)d->lastSlots.size();
    *n = k;
    if (k > cap) return fail(ORBX_E_CAPACITY, "%d entries, caller capacity %d", k, cap);
    if (k && slots) memcpy(slots, d->lastSlots.data(), (size_t)k * 4);
    if (k && scores) memcpy(scores, d->lastScores.data(), (size_t)k * 4);
    return ORBX_OK;
}

// the member table (slot, live copies, sequence of the earliest) on the device
static int kf_db_members(orbk_db* d)
{
    if (!d->dirty) return ORBX_OK;
    orbk_pool* p = d->pool;
    std::vector<orbk::Member> h;
    for (size_t s = 0; s < d->copies.size(); s++)
        if (!d->copies[s].empty()) h.push_back({(int32_t)s, (int32_t)d->copies[s].size(), d->copies[s].front(), 0});
    int rc;
    if ((rc = kbuf_reserve(p, d->bMem, std::max<size_t>(h.size(), 1) * sizeof(orbk::Member)))) return rc;
    if (!h.empty()) HIPCHK(hipMemcpyAsync(d->bMem.p, h.data(), h.size() * sizeof(orbk::Member), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    d->m = (int)h.size();
    d->dirty = false;
    return ORBX_OK;
}

// per-member and per-entry scratch of one query (m members)
struct KfScr {
    uint64_t *key, *selKey; int32_t *selSlot, *ordSlot, *best; float *selScore, *ordScore, *acc;
};
static int kf_scratch(orbk_pool* p, int m, KfScr& s)
{
    Packer pk;
    const size_t M = (size_t)std::max(m, 1);
    const size_t oK = pk.take(M * 8), oSK = pk.take(M * 8), oSS = pk.take(M * 4), oOS = pk.take(M * 4), oB = pk.take(M * 4);
    const size_t oSc = pk.take(M * 4), oOSc = pk.take(M * 4), oA = pk.take(M * 4);
    int rc = kbuf_reserve(p, p->bScr, pk.off);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)p->bScr.p;
    s = {(uint64_t*)(b + oK), (uint64_t*)(b + oSK), (int32_t*)(b + oSS), (int32_t*)(b + oOS), (int32_t*)(b + oB), (float*)(b + oSc), (float*)(b + oOSc), (float*)(b + oA)};
    return ORBX_OK;
}

// k_kf_prepare .. k_kf_rank of query Q.q on the pool's stream
static void kf_launch_front(orbk_pool* p, const orbk::Query& Q, const orbk_db* d, const KfScr& s)
{
    const orbk::PoolDev P = kf_dev(p);
    const orbk::Member* mem = (const orbk::Member*)d->bMem.p;
    hipLaunchKernelGGL(orbk::k_kf_prepare, dim3(16), dim3(256), 0, p->stream, P, Q);
    if (d->m == 0) return;
    const dim3 gw((d->m + 3) / 4), gt((d->m + 255) / 256);
    hipLaunchKernelGGL(orbk::k_kf_count, gw, dim3(256), 0, p->stream, P, Q, mem, d->m, s.key);
    hipLaunchKernelGGL(orbk::k_kf_score, gw, dim3(256), 0, p->stream, P, Q, mem, d->m, (const uint64_t*)s.key, s.selKey, s.selSlot, s.selScore);
    hipLaunchKernelGGL(orbk::k_kf_rank, gt, dim3(256), 0, p->stream, Q, (const uint64_t*)s.selKey, (const int32_t*)s.selSlot, (const float*)s.selScore, s.ordSlot, s.ordScore);
}

// The single queries: front kernels, the scored list to the host, the neighbours of each scored keyframe from the
// caller (GetBestCovisibilityKeyFrames(10) at this point of the reference) or the pool's table, accumulation, finalize.
struct KfSingle {
    bool loop; uint64_t qid;
    // query BowVector: host arrays, a frame set slot, or a pool slot
    const uint32_t* ids; const double* vals; int n;
    orbm_frameset* fs; int fsSlot;
    int qSlot;
    const int32_t* conn; int nconn; float minScore;
    orbk_neighbours_fn cb; void* user;
    int32_t* out; int cap; int* nOut;
};

static int kf_single(orbk_db* d, const KfSingle& a)
{
    orbk_pool* p = d->pool;
    int rc;
    *a.nOut = 0;
    if (a.cap < 0 || (a.cap && !a.out)) return fail(ORBX_E_INVALID, "bad argument");
    if (a.qSlot >= 0 && a.qSlot >= p->n) return fail(ORBX_E_INVALID, "slot %d out of range", a.qSlot);
    for (int i = 0; i < a.nconn; i++) if (a.conn[i] < 0 || a.conn[i] >= p->n) return fail(ORBX_E_INVALID, "connected slot %d out of range", a.conn[i]);
    if ((rc = kf_db_members(d))) return rc;
    KfScr s;
    if ((rc = kf_scratch(p, d->m, s))) return rc;
    const int qcap = a.fs ? a.fs->cap : a.n;
    // parameters: qid | counters | connStart[2] | connIdx | outTotal | qLen | qIds | qVals
    Packer pk;
    const size_t oQid = pk.take(8), oCnt = pk.take(sizeof(orbk::Counters)), oCs = pk.take(8), oCi = pk.take((size_t)a.nconn * 4), oTot = pk.take(4),
                 oLen = pk.take(4), oIds = pk.take((size_t)qcap * 4), oVals = pk.take((size_t)qcap * 8);
    const size_t upBytes = a.fs ? oIds : pk.off;
    if ((rc = kbuf_reserve(p, p->bPar, pk.off)) || (rc = kf_stage(p, pk.off))) return rc;
    uint8_t* h = p->h_stage;
    uint8_t* dp = (uint8_t*)p->bPar.p;
    memset(h, 0, upBytes);
    *(uint64_t*)(h + oQid) = a.qid;
    ((orbk::Counters*)(h + oCnt))->minScore = a.minScore;
    ((int32_t*)(h + oCs))[1] = a.nconn;
    if (a.nconn) memcpy(h + oCi, a.conn, (size_t)a.nconn * 4);
    if (a.qSlot >= 0) *(int32_t*)(h + oLen) = a.qSlot;
    else if (!a.fs) {
        *(int32_t*)(h + oLen) = a.n;
        if (a.n) { memcpy(h + oIds, a.ids, (size_t)a.n * 4); memcpy(h + oVals, a.vals, (size_t)a.n * 8); }
    }
    HIPCHK(hipMemcpyAsync(dp, h, upBytes, hipMemcpyHostToDevice, p->stream));
    if (a.fs && (rc = kf_copy_from_frameset(p, a.fs, a.fsSlot, (uint32_t*)(dp + oIds), (double*)(dp + oVals), (int32_t*)(dp + oLen), qcap))) return rc;
    orbk::Query Q{};
    Q.qSlot = a.qSlot >= 0 ? (const int32_t*)(dp + oLen) : nullptr;   // (a pool slot as the query: its index in qLen's place)
    Q.qIds = (const uint32_t*)(dp + oIds); Q.qVals = (const double*)(dp + oVals); Q.qLen = (const int32_t*)(dp + oLen);
    Q.qid = (const uint64_t*)(dp + oQid); Q.connStart = (const int32_t*)(dp + oCs); Q.connIdx = (const int32_t*)(dp + oCi);
    Q.cnt = (orbk::Counters*)(dp + oCnt); Q.q = 0; Q.loop = a.loop; Q.epoch = kf_next_epoch(p);
    kf_launch_front(p, Q, d, s);
    HIPCHK(hipGetLastError());
    // the scored list (lScoreAndMatch) down
    const size_t M = (size_t)std::max(d->m, 1);
    Packer dn;
    const size_t hCnt = dn.take(sizeof(orbk::Counters)), hSl = dn.take(M * 4), hSc = dn.take(M * 4);
    if ((rc = kf_stage(p, dn.off))) return rc;
    h = p->h_stage;
    HIPCHK(hipMemcpyAsync(h + hCnt, Q.cnt, sizeof(orbk::Counters), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(h + hSl, s.ordSlot, M * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(h + hSc, s.ordScore, M * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    const int nSel = d->m ? ((orbk::Counters*)(h + hCnt))->nSel : 0;
    d->lastSlots.assign((int32_t*)(h + hSl), (int32_t*)(h + hSl) + nSel);
    d->lastScores.assign((float*)(h + hSc), (float*)(h + hSc) + nSel);
    if (nSel == 0) return ORBX_OK;
    // neighbours at this point
    const int32_t* nbStart = nullptr; const int32_t* nbIdx = nullptr;
    if (a.cb) {
        std::vector<int32_t> st(1, 0), ix;
        ix.reserve((size_t)nSel * orbk::kNeigh);
        int32_t tmp[orbk::kNeigh];
        for (int e = 0; e < nSel; e++) {
            const int k = a.cb(a.user, d->lastSlots[e], tmp);
            if (k < 0 || k > orbk::kNeigh) return fail(ORBX_E_INVALID, "neighbour callback returned %d for slot %d", k, d->lastSlots[e]);
            for (int i = 0; i < k; i++) {
                if (tmp[i] < 0 || tmp[i] >= p->n) return fail(ORBX_E_INVALID, "neighbour slot %d out of range", tmp[i]);
                ix.push_back(tmp[i]);
            }
            st.push_back((int32_t)ix.size());
        }
        if ((rc = kbuf_reserve(p, p->bOut, (st.size() + ix.size()) * 4)) || (rc = kf_stage(p, (st.size() + ix.size()) * 4))) return rc;
        h = p->h_stage;
        memcpy(h, st.data(), st.size() * 4);
        if (!ix.empty()) memcpy(h + st.size() * 4, ix.data(), ix.size() * 4);
        HIPCHK(hipMemcpyAsync(p->bOut.p, h, (st.size() + ix.size()) * 4, hipMemcpyHostToDevice, p->stream));
        nbStart = (const int32_t*)p->bOut.p; nbIdx = nbStart + st.size();
    }
    // the accumulation's outputs and the candidates reuse scratch the front kernels are done with
    float* dAcc = (float*)s.key;
    int32_t* dBest = (int32_t*)s.selKey;
    int32_t* dRes = s.selSlot;
    hipLaunchKernelGGL(orbk::k_kf_acc, dim3((nSel + 255) / 256), dim3(256), 0, p->stream, kf_dev(p), Q, (const int32_t*)s.ordSlot, (const float*)s.ordScore,
                       nbStart, nbIdx, dAcc, dBest);
    hipLaunchKernelGGL(orbk::k_kf_finalize, dim3(1), dim3(orbk::kFinThreads), 0, p->stream, Q, (const float*)dAcc, (const int32_t*)dBest, p->d_firstIdx,
                       dRes, nSel, (int32_t*)(dp + oTot), (int32_t*)nullptr);
    HIPCHK(hipGetLastError());
    Packer rs;
    const size_t rCnt = rs.take(sizeof(orbk::Counters)), rOut = rs.take((size_t)nSel * 4);
    if ((rc = kf_stage(p, rs.off))) return rc;
    h = p->h_stage;
    HIPCHK(hipMemcpyAsync(h + rCnt, Q.cnt, sizeof(orbk::Counters), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(h + rOut, dRes, (size_t)nSel * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    const int k = ((orbk::Counters*)(h + rCnt))->nOut;
    *a.nOut = k;
    memcpy(a.out, h + rOut, (size_t)std::min(k, a.cap) * 4);
    if (k > a.cap) return fail(ORBX_E_CAPACITY, "%d candidates, caller capacity %d", k, a.cap);
    return ORBX_OK;
}

// vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F) (:211-303); F->mBowVec from host arrays
extern "C" int orbk_detect_relocalization_candidates(orbk_db_t* d, uint64_t query_id, const uint32_t* ids, const double* vals, int n,
                                                     orbk_neighbours_fn neighbours, void* user, int32_t* out, int cap, int* n_out)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    if (!n_out || n < 0 || (n && (!ids || !vals))) return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < n; i++)
        if ((int64_t)ids[i] >= L.p->nWords || (i && ids[i] <= ids[i - 1])) return fail(ORBX_E_INVALID, "word ids must ascend and lie below %d", L.p->nWords);
    KfSingle a{false, query_id, ids, vals, n, nullptr, 0, -1, nullptr, 0, 0.f, neighbours, user, out, cap, n_out};
    return kf_single(d, a);
}

// the same with F->mBowVec = a frame set slot's (orbm_frameset_compute_bow), copied device to device
extern "C" int orbk_detect_relocalization_candidates_frameset(orbk_db_t* d, uint64_t query_id, orbm_frameset_t* fs, int fs_slot,
                                                              orbk_neighbours_fn neighbours, void* user, int32_t* out, int cap, int* n_out)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    if (!n_out) return fail(ORBX_E_INVALID, "bad argument");
    int rc = kf_frameset_usable(L.p, fs, fs_slot);
    if (rc) return rc;
    KfSingle a{false, query_id, nullptr, nullptr, 0, fs, fs_slot, -1, nullptr, 0, 0.f, neighbours, user, out, cap, n_out};
    return kf_single(d, a);
}

// vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore) (:97-209); pKF = a pool slot,
// connected = pKF->GetConnectedKeyFrames()
extern "C" int orbk_detect_loop_candidates(orbk_db_t* d, int slot, uint64_t query_id, const int32_t* connected, int nconn, float min_score,
                                           orbk_neighbours_fn neighbours, void* user, int32_t* out, int cap, int* n_out)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    if (!n_out || nconn < 0 || (nconn && !connected)) return fail(ORBX_E_INVALID, "bad argument");
    if (slot < 0) return fail(ORBX_E_INVALID, "slot %d out of range", slot);
    KfSingle a{true, query_id, nullptr, nullptr, 0, nullptr, 0, slot, connected, nconn, min_score, neighbours, user, out, cap, n_out};
    return kf_single(d, a);
}

// MultiMapper::DetectLoop's scan (MultiMapper.cc:117-157) for n keyframes: minScore from each one's covisible keyframes,
// then DetectLoopCandidates(pKF, minScore), the n queries one after another on the stream; neighbours from the pool's table
extern "C" int orbk_detect_loop_batch(orbk_db_t* d, int n, const int32_t* slots, const uint64_t* query_ids,
                                      const int32_t* conn_start, const int32_t* conn_idx, const int32_t* cov_start, const int32_t* cov_idx,
                                      int32_t* out_start, int32_t* out, int cap)
{
    KfDbLock L(d);
    if (L.rc) return L.rc;
    orbk_pool* p = L.p;
    if (n < 0 || !out_start || cap < 0 || (cap && !out) || (n && (!slots || !query_ids || !conn_start || !cov_start)))
        return fail(ORBX_E_INVALID, "bad argument");
    out_start[0] = 0;
    if (n == 0) return ORBX_OK;
    if (conn_start[0] != 0 || cov_start[0] != 0) return fail(ORBX_E_INVALID, "CSR starts must begin at 0");
    for (int q = 0; q < n; q++) {
        if (slots[q] < 0 || slots[q] >= p->n) return fail(ORBX_E_INVALID, "slot %d out of range", slots[q]);
        if (conn_start[q + 1] < conn_start[q] || cov_start[q + 1] < cov_start[q]) return fail(ORBX_E_INVALID, "CSR starts must not decrease");
    }
    const int nc = conn_start[n], nv = cov_start[n];
    if ((nc && !conn_idx) || (nv && !cov_idx)) return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < nc; i++) if (conn_idx[i] < 0 || conn_idx[i] >= p->n) return fail(ORBX_E_INVALID, "connected slot %d out of range", conn_idx[i]);
    for (int i = 0; i < nv; i++) if (cov_idx[i] < 0 || cov_idx[i] >= p->n) return fail(ORBX_E_INVALID, "covisible slot %d out of range", cov_idx[i]);
    int rc;
    if ((rc = kf_db_members(d))) return rc;
    KfScr s;
    if ((rc = kf_scratch(p, d->m, s))) return rc;
    // parameters: qid[n] | qSlot[n] | connStart[n+1] | connIdx | covStart[n+1] | pairA | pairB | outTotal | counters[n] | pairScore | outStart[n+1] | out[cap]
    Packer pk;
    const size_t oQid = pk.take((size_t)n * 8), oSl = pk.take((size_t)n * 4), oCs = pk.take((size_t)(n + 1) * 4), oCi = pk.take((size_t)nc * 4),
                 oVs = pk.take((size_t)(n + 1) * 4), oPa = pk.take((size_t)nv * 4), oPb = pk.take((size_t)nv * 4), oTot = pk.take(4),
                 oCnt = pk.take((size_t)n * sizeof(orbk::Counters)), oPs = pk.take((size_t)nv * 4), oOs = pk.take((size_t)(n + 1) * 4),
                 oOut = pk.take((size_t)std::max(cap, 1) * 4);
    const size_t upBytes = oCnt;
    if ((rc = kbuf_reserve(p, p->bPar, pk.off)) || (rc = kf_stage(p, std::max(upBytes, oOut - oOs)))) return rc;
    uint8_t* h = p->h_stage;
    uint8_t* dp = (uint8_t*)p->bPar.p;
    memcpy(h + oQid, query_ids, (size_t)n * 8);
    memcpy(h + oSl, slots, (size_t)n * 4);
    memcpy(h + oCs, conn_start, (size_t)(n + 1) * 4);
    if (nc) memcpy(h + oCi, conn_idx, (size_t)nc * 4);
    memcpy(h + oVs, cov_start, (size_t)(n + 1) * 4);
    for (int q = 0; q < n; q++) for (int i = cov_start[q]; i < cov_start[q + 1]; i++) ((int32_t*)(h + oPa))[i] = slots[q];
    if (nv) memcpy(h + oPb, cov_idx, (size_t)nv * 4);
    *(int32_t*)(h + oTot) = 0;
    HIPCHK(hipMemcpyAsync(dp, h, upBytes, hipMemcpyHostToDevice, p->stream));
    orbk::Counters* dCnt = (orbk::Counters*)(dp + oCnt);
    const orbk::PoolDev P = kf_dev(p);
    // minScore of every query first: the scores read BowVectors only, which no query changes
    if (nv) hipLaunchKernelGGL(orbk::k_kf_score_pairs, dim3((nv + 3) / 4), dim3(256), 0, p->stream, P, (const int32_t*)(dp + oPa), (const int32_t*)(dp + oPb), nv, (float*)(dp + oPs));
    hipLaunchKernelGGL(orbk::k_kf_min_score, dim3((n + 255) / 256), dim3(256), 0, p->stream, (const float*)(dp + oPs), (const int32_t*)(dp + oVs), n, dCnt);
    float* dAcc = (float*)s.key;
    int32_t* dBest = (int32_t*)s.selKey;
    const dim3 gt((std::max(d->m, 1) + 255) / 256);
    for (int q = 0; q < n; q++) {
        orbk::Query Q{};
        Q.qSlot = (const int32_t*)(dp + oSl); Q.qid = (const uint64_t*)(dp + oQid);
        Q.connStart = (const int32_t*)(dp + oCs); Q.connIdx = (const int32_t*)(dp + oCi);
        Q.cnt = dCnt; Q.q = q; Q.loop = 1; Q.epoch = kf_next_epoch(p);
        kf_launch_front(p, Q, d, s);
        if (d->m) hipLaunchKernelGGL(orbk::k_kf_acc, gt, dim3(256), 0, p->stream, P, Q, (const int32_t*)s.ordSlot, (const float*)s.ordScore,
                                     (const int32_t*)nullptr, (const int32_t*)nullptr, dAcc, dBest);
        hipLaunchKernelGGL(orbk::k_kf_finalize, dim3(1), dim3(orbk::kFinThreads), 0, p->stream, Q, (const float*)dAcc, (const int32_t*)dBest, p->d_firstIdx,
                           (int32_t*)(dp + oOut), cap, (int32_t*)(dp + oTot), (int32_t*)(dp + oOs));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dp + oOs, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    memcpy(out_start, h, (size_t)(n + 1) * 4);
    const int total = out_start[n], k = std::min(total, cap);
    if (k) {
        if ((rc = kf_stage(p, (size_t)k * 4))) return rc;   // (the block was sized for the parameters, not the candidates)
        h = p->h_stage;
        HIPCHK(hipMemcpyAsync(h, dp + oOut, (size_t)k * 4, hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        memcpy(out, h, (size_t)k * 4);
    }
    if (total > cap) return fail(ORBX_E_CAPACITY, "%d candidates, caller capacity %d", total, cap);
    return ORBX_OK;
}
