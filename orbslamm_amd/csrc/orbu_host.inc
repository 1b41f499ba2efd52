// orbu_host.inc -- host side of Tracking::UpdateLocalMap on the device (part of orbslamm_hip.hip; kernels: orbu_kernels.hip,
// ABI: include/orbslamm_localmap.h, DESIGN.md §8r).
//   the store     struct orbu_store, the slot and entry checks, the generation tag, the last-wins staging: orbx_poolutil.inc.
//                 Create and destroy are here, and EVERY setter of the store: the records, and the columns the later families read
//                 (octaves, descriptors, centres, mpRefKF; their scatter kernels are orbr::'s and orbe::'s).  The store owns and frees
//                 the columns; orbn, orbr and orbe free their own blocks in their *_release
//   the call      stamp, vote, select, mark, count, scan, write on the pool's stream, one synchronisation; the kernels leave
//                 the result in the store's pinned block themselves
//   the search    orbw_track (orbw_host.inc) reading the store's S where it lies

static_assert(ORBU_ENTRY_NO_VOTE == orbu::kNoVote && ORBU_MAX_KEYFRAMES == orbu::kMaxKeyFrames && ORBU_MAX_NEIGHBOURS + 2 == orbu::kGraphInts,
              "orbslamm_localmap.h constants");

constexpr size_t kStoreMaxEntries = (size_t)1 << 28;   // kf_capacity * pitch: positions of the point walk fit 32 bits with room
static void orbn_release(orbu_store* s);   // orbn_host.inc
static void orbr_release(orbu_store* s);   // orbr_host.inc
static void orbe_release(orbu_store* s);   // orbe_host.inc

extern "C" int orbu_store_create(orbw_pool_t* pool, int kf_capacity, int stride, int max_children, int max_local_points, orbu_store_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    if (kf_capacity <= 0 || stride <= 0 || max_children < 0 || max_local_points <= 0)
        return fail(ORBX_E_INVALID, "kf_capacity %d, stride %d, max_children %d, max_local_points %d", kf_capacity, stride, max_children, max_local_points);
    const int pitch = (stride + 3) & ~3;
    if (kf_capacity > ORBU_MAX_KEYFRAMES || stride > ORBU_MAX_STRIDE || max_children > ORBU_MAX_CHILDREN || max_local_points > ORBW_POOL_MAX_CAPACITY ||
        (size_t)kf_capacity * pitch > kStoreMaxEntries)
        return fail(ORBX_E_UNSUPPORTED, "kf_capacity %d (at most %d), stride %d (%d), max_children %d (%d), max_local_points %d (%d), kf_capacity x stride at most %zu",
                    kf_capacity, ORBU_MAX_KEYFRAMES, stride, ORBU_MAX_STRIDE, max_children, ORBU_MAX_CHILDREN, max_local_points, ORBW_POOL_MAX_CAPACITY, kStoreMaxEntries);
    int rc = orbw_pool_check(pool);
    if (rc) return rc;
    orbu_store* s = new orbu_store();
    s->pool = pool; s->kfcap = kf_capacity; s->stride = stride; s->pitch = pitch; s->maxc = max_children; s->maxcP = (max_children + 3) & ~3;
    s->maxL = max_local_points;
    const size_t K = (size_t)kf_capacity, P = (size_t)pool->cap, nchunks = (K * pitch + orbu::kChunk - 1) / orbu::kChunk;
    Packer pk;
    const size_t oEnt = pk.take(K * pitch * 4), oFlags = pk.take(K), oGraph = pk.take(K * orbu::kGraphInts * 4), oChild = pk.take(K * s->maxc * 4),
                 oStamp = pk.take(P * 8), oFirst = pk.take(P * 8), oHdr = pk.take(orbu::H_INTS * 4), oList = pk.take(K * 4), oVotes = pk.take(K * 4),
                 oChunk = pk.take(nchunks * 8), oL = pk.take((size_t)s->maxL * 4), oS = pk.take((size_t)s->maxL * 4), bytes = pk.off;
    Packer hp;
    const size_t hHdr = hp.take(orbu::H_INTS * 4), hList = hp.take(K * 4), hVotes = hp.take(K * 4), hL = hp.take((size_t)s->maxL * 4),
                 hSeen = hp.take((size_t)s->maxL), hbytes = hp.off;
    auto bail = [&](int code) { if (s->d_block) (void)hipFree(s->d_block); if (s->h_res) (void)hipHostFree(s->h_res); delete s; return code; };
    std::lock_guard<std::mutex> l(pool->mu);
    HIPCHK_OR(hipMalloc(&s->d_block, bytes), bail(0));
    HIPCHK_OR(hipHostMalloc((void**)&s->h_res, hbytes, hipHostMallocCoherent), bail(0));
    memset(s->h_res, 0, hbytes);
    uint8_t* d = s->d_block;
    // entries -1 (empty), the first-sighting words all ones; the rest zero
    HIPCHK_OR(hipMemsetAsync(d, 0, bytes, pool->stream), bail(0));
    HIPCHK_OR(hipMemsetAsync(d + oEnt, 0xff, K * pitch * 4, pool->stream), bail(0));
    HIPCHK_OR(hipMemsetAsync(d + oFirst, 0xff, P * 8, pool->stream), bail(0));
    HIPCHK_OR(hipStreamSynchronize(pool->stream), bail(0));
    s->dev.entries = (int32_t*)(d + oEnt); s->dev.flags = d + oFlags; s->dev.graph = (int32_t*)(d + oGraph); s->dev.children = (int32_t*)(d + oChild);
    s->dev.kfcap = kf_capacity; s->dev.pitch = pitch; s->dev.maxc = s->maxc;
    s->scr.stamp = (unsigned long long*)(d + oStamp); s->scr.first = (unsigned long long*)(d + oFirst); s->scr.poolFlags = pool->dev.flags; s->scr.poolCap = pool->cap;
    s->out.hdr = (int32_t*)(d + oHdr); s->out.list = (int32_t*)(d + oList); s->out.votes = (int32_t*)(d + oVotes); s->out.chunk = (uint2*)(d + oChunk);
    s->out.L = (int32_t*)(d + oL); s->out.S = (int32_t*)(d + oS);
    s->out.hHdr = (int32_t*)(s->h_res + hHdr); s->out.hList = (int32_t*)(s->h_res + hList); s->out.hVotes = (int32_t*)(s->h_res + hVotes);
    s->out.hL = (int32_t*)(s->h_res + hL); s->out.hSeen = s->h_res + hSeen; s->out.maxL = s->maxL;
    s->kfSet.assign(K, 0); s->oct.has.assign(K, 0); s->desc.has.assign(K, 0); s->ctr.has.assign(K, 0); s->kfSeen.assign((K + 63) / 64, 0); s->idxSeen.assign(((size_t)stride + 63) / 64, 0);
    s->blocks = (unsigned)std::min<size_t>(nchunks, 1024);
    pool->h->refs++;
    pool->h->nDevAlloc++; pool->h->nHostAlloc++;
    live_add(s);
    *out = s;
    return ORBX_OK;
}

extern "C" int orbu_store_destroy(orbu_store_t* s)
{
    if (!s) return ORBX_OK;
    live_remove(s);
    orbm_handle* h = nullptr;
    if (live_has(s->pool)) {
        h = s->pool->h;
        (void)hipSetDevice(h->device);
        std::lock_guard<std::mutex> l(s->pool->mu);
        for (auto& r : s->pool->readers) (void)hipEventSynchronize(r.ev);   // a resident search may still read S
        (void)hipStreamSynchronize(s->pool->stream);
    }
    orbn_release(s);
    orbr_release(s);
    orbe_release(s);
    for (void* d : {(void*)s->oct.d, (void*)s->desc.d, (void*)s->ctr.d, (void*)s->d_refKf, (void*)s->d_block}) (void)hipFree(d);   // (null: no-op)
    (void)hipHostFree(s->h_res);
    if (s->h_stage) (void)hipHostFree(s->h_stage);
    if (h) orbm_release(h);
    delete s;
    return ORBX_OK;
}

// orbu_kf_set (whole = true) and orbu_kf_set_graph
static int orbu_kf_write(orbu_store* s, const OrbuKeyFrames* kfs, bool whole)
{
    if (!kfs) return fail(ORBX_E_INVALID, "null argument");
    const int nkf = kfs->nkf;
    if (nkf == 0) return ORBX_OK;
    if (nkf < 0) return fail(ORBX_E_INVALID, "negative count");
    if (!kfs->slot || !kfs->neigh || !kfs->parent || !kfs->nchildren || (whole && (!kfs->flags || !kfs->n))) return fail(ORBX_E_INVALID, "null argument");
    int64_t nent = 0, nch = 0;
    for (int i = 0; i < nkf; i++) {
        if (kfs->nchildren[i] < 0 || (whole && kfs->n[i] < 0)) return fail(ORBX_E_INVALID, "negative count in record %d", i);
        nch += kfs->nchildren[i];
        if (whole) nent += kfs->n[i];
    }
    if ((nch && !kfs->children) || (nent && !kfs->entries)) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    std::lock_guard<std::mutex> l(s->pool->mu);
    // every id, on the host, before any launch; where record i's entries and children start
    s->eOff.resize((size_t)nkf); s->cOff.resize((size_t)nkf);
    int64_t e0 = 0, c0 = 0;
    for (int i = 0; i < nkf; i++) {
        if ((rc = orbu_check_slot(s, "slot", i, kfs->slot[i], !whole))) return rc;
        if (whole && kfs->n[i] > s->stride) return fail(ORBX_E_UNSUPPORTED, "record %d: %d entries for a stride of %d", i, kfs->n[i], s->stride);
        if (kfs->nchildren[i] > s->maxc) return fail(ORBX_E_UNSUPPORTED, "record %d: %d children, at most %d", i, kfs->nchildren[i], s->maxc);
        for (int e = 0; whole && e < kfs->n[i]; e++)
            if ((rc = orbw_check_id(s->pool, "entries", (int)(e0 + e), kfs->entries[e0 + e], true, true))) return rc;
        for (int j = 0; j < ORBU_MAX_NEIGHBOURS; j++)
            if ((rc = orbu_check_slot(s, "a neighbour of record", i, kfs->neigh[(size_t)i * ORBU_MAX_NEIGHBOURS + j], false, true))) return rc;
        if ((rc = orbu_check_slot(s, "parent", i, kfs->parent[i], false, true))) return rc;
        for (int c = 0; c < kfs->nchildren[i]; c++)
            if ((rc = orbu_check_slot(s, "children", (int)(c0 + c), kfs->children[c0 + c], false))) return rc;
        s->eOff[i] = e0; s->cOff[i] = c0;
        if (whole) e0 += kfs->n[i];
        c0 += kfs->nchildren[i];
    }
    const int maxcP = s->maxcP, pitch = s->pitch, recInts = orbu::kRecHead + maxcP + (whole ? pitch : 0);
    const int perLaunch = (int)std::max<size_t>(1, std::min<size_t>((size_t)nkf, kStoreStageBytes / ((size_t)recInts * 4)));
    if ((rc = orbw_begin_write(s->pool, s->h_stage, s->stageCap, (size_t)perLaunch * recInts * 4))) return rc;
    // (all by value, as orbw_pool_write's: captured by reference, the staged loop reloads them behind every store into the staging)
    int32_t* stage = (int32_t*)s->h_stage;
    const OrbuKeyFrames k = *kfs;
    const int64_t *eOff = s->eOff.data(), *cOff = s->cOff.data();
    auto emit = [=](int i, int m) {
        int32_t* rec = stage + (size_t)m * recInts;
        rec[0] = k.slot[i]; rec[1] = whole ? ((k.flags[i] & ORBU_KF_BAD) | ORBU_KF_SET) : 0;
        for (int j = 0; j < ORBU_MAX_NEIGHBOURS; j++) rec[2 + j] = k.neigh[(size_t)i * ORBU_MAX_NEIGHBOURS + j];
        rec[12] = k.parent[i]; rec[13] = k.nchildren[i]; rec[14] = rec[15] = 0;
        for (int c = 0; c < maxcP; c++) rec[orbu::kRecHead + c] = c < k.nchildren[i] ? k.children[cOff[i] + c] : -1;
        if (whole) {
            int32_t* ent = rec + orbu::kRecHead + maxcP;
            if (k.n[i]) memcpy(ent, k.entries + eOff[i], (size_t)k.n[i] * 4);
            for (int e = k.n[i]; e < pitch; e++) ent[e] = -1;
        }
    };
    auto flush = [=](int m) -> int {
        hipLaunchKernelGGL(orbu::k_kf_scatter, dim3((unsigned)m), dim3(orbu::kThreads), 0, s->pool->stream, s->dev, (const int32_t*)stage, recInts, maxcP, whole ? 0 : 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->pool->stream));
        return ORBX_OK;
    };
    if ((rc = stage_last_wins(k.slot, nkf, nkf, perLaunch, s->kfSeen, emit, flush))) return rc;   // (one window: a slot is staged once however often the call repeats it)
    if (whole)
        for (int i = 0; i < nkf; i++) { s->kfSet[kfs->slot[i]] = 1; s->hi = std::max(s->hi, kfs->slot[i] + 1); }
    return ORBX_OK;
}

extern "C" int orbu_kf_set(orbu_store_t* store, const OrbuKeyFrames* kfs) { return orbu_kf_write(store, kfs, true); }
extern "C" int orbu_kf_set_graph(orbu_store_t* store, const OrbuKeyFrames* kfs) { return orbu_kf_write(store, kfs, false); }

// orbu_kf_set_flags (slot < 0: a = slots, b = flags) and orbu_kf_set_entries (a = idx, b = vals of keyframe `slot`)
static int orbu_pairs_write(orbu_store* s, int slot, const int32_t* a, const int32_t* vals, const uint8_t* flags, int n)
{
    const bool ent = slot >= 0;
    if (n == 0) return ORBX_OK;
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (!a || (ent ? !vals : !flags)) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    std::lock_guard<std::mutex> l(s->pool->mu);
    if (ent && (rc = orbu_check_slot(s, "slot", 0, slot, true))) return rc;
    for (int i = 0; i < n; i++) {
        if (ent) {
            if (a[i] < 0) return fail(ORBX_E_INVALID, "idx[%d] = %d", i, a[i]);
            if (a[i] >= s->stride) return fail(ORBX_E_UNSUPPORTED, "idx[%d] = %d for a stride of %d", i, a[i], s->stride);
            if ((rc = orbw_check_id(s->pool, "vals", i, vals[i], true, true))) return rc;
        } else if ((rc = orbu_check_slot(s, "slots", i, a[i], true))) return rc;
    }
    const int perLaunch = (int)std::min<size_t>((size_t)n, kStoreStageBytes / 8);
    if ((rc = orbw_begin_write(s->pool, s->h_stage, s->stageCap, (size_t)perLaunch * 8))) return rc;
    int2* stage = (int2*)s->h_stage;
    auto emit = [=](int i, int m) { stage[m] = make_int2(a[i], ent ? vals[i] : ((flags[i] & ORBU_KF_BAD) | ORBU_KF_SET)); };   // (by value, as orbw_pool_write's)
    auto flush = [=](int m) -> int {
        hipLaunchKernelGGL(orbu::k_pair_scatter, dim3((unsigned)((m + orbu::kThreads - 1) / orbu::kThreads)), dim3(orbu::kThreads), 0, s->pool->stream,
                           s->dev, (const int2*)stage, m, ent ? slot : 0, ent ? 0 : 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->pool->stream));
        return ORBX_OK;
    };
    return stage_last_wins(a, n, perLaunch, perLaunch, ent ? s->idxSeen : s->kfSeen, emit, flush);
}

extern "C" int orbu_kf_set_flags(orbu_store_t* store, const int32_t* slots, const uint8_t* flags, int n)
{
    return orbu_pairs_write(store, -1, slots, nullptr, flags, n);
}

extern "C" int orbu_kf_set_entries(orbu_store_t* store, int slot, const int32_t* idx, const int32_t* vals, int n)
{
    if (slot < 0) return fail(ORBX_E_INVALID, "keyframe slot %d", slot);
    return orbu_pairs_write(store, slot, idx, vals, nullptr, n);
}

// ---- the columns: each made at the first call of its setter (orbu_block_once), read by orbn, orbr and orbe

extern "C" int orbu_kf_set_octaves(orbu_store_t* s, int slot, const uint8_t* octaves, int n)
{
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (slot < 0) return fail(ORBX_E_INVALID, "keyframe slot %d", slot);
    if (n > 0 && !octaves) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbu_check_slot(s, "slot", 0, slot, true))) return rc;
    if (n > s->stride) return fail(ORBX_E_UNSUPPORTED, "%d octaves for a stride of %d", n, s->stride);
    {   // the distinct values the store has been given: the histograms have a bin for each
        bool seen[256];
        int distinct = 0;
        for (int v = 0; v < 256; v++) { seen[v] = s->octSeen[v]; }
        seen[0] = seen[0] || n < s->stride;
        for (int i = 0; i < n; i++) seen[octaves[i]] = true;
        for (int v = 0; v < 256; v++) distinct += seen[v] ? 1 : 0;
        if (distinct > ORBN_MAX_OCTAVE_VALUES)
            return fail(ORBX_E_UNSUPPORTED, "%d distinct octave values in the store, at most %d", distinct, ORBN_MAX_OCTAVE_VALUES);
    }
    if ((rc = orbu_block_once(p, s->oct.d, (size_t)s->kfcap * s->pitch, 0))) return rc;
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, (size_t)s->pitch))) return rc;
    if (n) memcpy(s->h_stage, octaves, (size_t)n);
    memset(s->h_stage + n, 0, (size_t)(s->pitch - n));
    HIPCHK(hipMemcpyAsync(s->oct.d + (size_t)slot * s->pitch, s->h_stage, (size_t)s->pitch, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (n < s->stride) s->octSeen[0] = 1;
    for (int i = 0; i < n; i++) s->octSeen[octaves[i]] = 1;
    s->oct.has[slot] = 1;
    return ORBX_OK;
}

extern "C" int orbu_kf_set_descriptors(orbu_store_t* s, int slot, const uint8_t* desc, int n)
{
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (slot < 0) return fail(ORBX_E_INVALID, "keyframe slot %d", slot);
    if (!desc) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbu_check_slot(s, "slot", 0, slot, true))) return rc;
    if (n > s->stride) return fail(ORBX_E_UNSUPPORTED, "%d descriptors for a stride of %d", n, s->stride);
    const size_t rowBytes = (size_t)s->pitch * 32;
    if ((rc = orbu_block_once(p, s->desc.d, (size_t)s->kfcap * rowBytes, 0))) return rc;
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, rowBytes))) return rc;
    if (n) memcpy(s->h_stage, desc, (size_t)n * 32);
    memset(s->h_stage + (size_t)n * 32, 0, rowBytes - (size_t)n * 32);
    const int n16 = (int)(rowBytes / 16);
    hipLaunchKernelGGL(orbr::k_desc_scatter, dim3((unsigned)((n16 + orbr::kThreads - 1) / orbr::kThreads)), dim3(orbr::kThreads), 0, p->stream,
                       s->desc.d + (size_t)slot * rowBytes, (const uint4*)s->h_stage, n16);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    s->desc.has[slot] = 1;
    return ORBX_OK;
}

extern "C" int orbu_kf_set_descriptors_frame(orbu_store_t* s, int slot, orbm_frameset_t* fs, int fs_slot)
{
    if (slot < 0) return fail(ORBX_E_INVALID, "keyframe slot %d", slot);
    if (!fs) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    if ((rc = frameset_check(fs))) return rc;
    orbw_pool* p = s->pool;
    if (fs->owner != p->h) return fail(ORBX_E_INVALID, "the frame set and the pool must be on one matcher handle");
    if (fs_slot < 0 || fs_slot >= fs->slots) return fail(ORBX_E_INVALID, "slot %d outside the frame set", fs_slot);
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbu_check_slot(s, "slot", 0, slot, true))) return rc;
    int32_t n = 0;
    hipStream_t fst = fs_stream(fs);
    HIPCHK(hipMemcpyAsync(&n, fs->fs.n + fs_slot, 4, hipMemcpyDeviceToHost, fst));
    HIPCHK(hipStreamSynchronize(fst));   // (the slot's build is complete behind this)
    if (n < 0 || n > fs->cap) return fail(ORBX_E_HIP, "a frame-set slot of %d features, capacity %d", n, fs->cap);
    if (n > s->stride) return fail(ORBX_E_UNSUPPORTED, "%d descriptors for a stride of %d", n, s->stride);
    const size_t rowBytes = (size_t)s->pitch * 32;
    if ((rc = orbu_block_once(p, s->desc.d, (size_t)s->kfcap * rowBytes, 0))) return rc;
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, 16))) return rc;
    uint8_t* dst = s->desc.d + (size_t)slot * rowBytes;
    if (n) HIPCHK(hipMemcpyAsync(dst, fs->fs.desc + (size_t)fs_slot * fs->cap * 32, (size_t)n * 32, hipMemcpyDeviceToDevice, p->stream));
    if (rowBytes > (size_t)n * 32) HIPCHK(hipMemsetAsync(dst + (size_t)n * 32, 0, rowBytes - (size_t)n * 32, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    s->desc.has[slot] = 1;
    return ORBX_OK;
}

extern "C" int orbu_kf_set_centres(orbu_store_t* s, const int32_t* slots, const float* Ow, int n)
{
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (n == 0) return ORBX_OK;
    if (!slots || !Ow) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    for (int i = 0; i < n; i++)
        if ((rc = orbu_check_slot(s, "slots", i, slots[i], true))) return rc;
    if ((rc = orbu_block_once(p, s->ctr.d, (size_t)s->kfcap * 12, 0))) return rc;
    const int perLaunch = (int)std::min<size_t>((size_t)n, kStoreStageBytes / 16);
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, (size_t)perLaunch * 16))) return rc;
    uint4* stage = (uint4*)s->h_stage;
    auto emit = [=](int i, int m) {   // (by value, as orbw_pool_write's)
        uint32_t w[3];
        memcpy(w, Ow + 3 * (size_t)i, 12);
        stage[m] = make_uint4((uint32_t)slots[i], w[0], w[1], w[2]);
    };
    auto flush = [=](int m) -> int {
        hipLaunchKernelGGL(orbr::k_centre_scatter, dim3((unsigned)((m + orbr::kThreads - 1) / orbr::kThreads)), dim3(orbr::kThreads), 0, p->stream,
                           s->ctr.d, s->kfcap, (const uint4*)stage, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(p->stream));
        return ORBX_OK;
    };
    if ((rc = stage_last_wins(slots, n, perLaunch, perLaunch, s->kfSeen, emit, flush))) return rc;
    for (int i = 0; i < n; i++) s->ctr.has[slots[i]] = 1;
    return ORBX_OK;
}

extern "C" int orbu_point_set_ref_kf(orbu_store_t* s, const int32_t* ids, const int32_t* kf_slots, int n)
{
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (n == 0) return ORBX_OK;
    if (!ids || !kf_slots) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbw_check_ids(p, "ids", ids, n, false, false))) return rc;
    for (int i = 0; i < n; i++)
        if ((rc = orbu_check_slot(s, "kf_slots", i, kf_slots[i], false, true))) return rc;
    if ((rc = orbu_block_once(p, s->d_refKf, (size_t)p->cap * 4, 0xff))) return rc;   // every id -1
    const int perLaunch = (int)std::min<size_t>((size_t)n, kStoreStageBytes / 8);
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, (size_t)perLaunch * 8))) return rc;
    int2* stage = (int2*)s->h_stage;
    auto emit = [=](int i, int m) { stage[m] = make_int2(ids[i], kf_slots[i]); };   // (by value, as orbw_pool_write's)
    auto flush = [=](int m) -> int {
        hipLaunchKernelGGL(orbe::k_ref_scatter, dim3((unsigned)((m + orbe::kThreads - 1) / orbe::kThreads)), dim3(orbe::kThreads), 0, p->stream,
                           s->d_refKf, p->cap, (const int2*)stage, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(p->stream));
        return ORBX_OK;
    };
    return stage_last_wins(ids, n, perLaunch, perLaunch, p->seen, emit, flush);
}

extern "C" int orbu_debug_set_generation(orbu_store_t* s, uint32_t generation)
{
    int rc = orbu_store_check(s);
    if (rc) return rc;
    std::lock_guard<std::mutex> l(s->pool->mu);
    if (generation < s->gen) return fail(ORBX_E_INVALID, "the generation tag only moves forward (%u now)", s->gen);
    s->gen = generation;
    return ORBX_OK;
}

// the device-resident S of the last completed update, copied down: what orbw_track_local_map_resident reads, for the tests
extern "C" int orbu_debug_resident_list(orbu_store_t* s, int32_t* out, int cap, int* n)
{
    if (!n || cap < 0 || (cap > 0 && !out)) return fail(ORBX_E_INVALID, "bad argument");
    int rc = orbu_store_check(s);
    if (rc) return rc;
    std::lock_guard<std::mutex> l(s->pool->mu);
    if (!s->updated) return fail(ORBX_E_INVALID, "the store has no completed update");
    *n = s->nS;
    if (s->nS > cap) return fail(ORBX_E_CAPACITY, "%d ids for a buffer of %d", s->nS, cap);
    if (s->nS) {
        HIPCHK(hipMemcpyAsync(out, s->out.S, (size_t)s->nS * 4, hipMemcpyDeviceToHost, s->pool->stream));
        HIPCHK(hipStreamSynchronize(s->pool->stream));
    }
    return ORBX_OK;
}

// both per-frame calls: given = the caller's keyframe list (orbu_local_points)
static int orbu_run(orbu_store* s, bool given, const int32_t* kf_list, int nkf, const int32_t* frame_ids, int n, int max_keyframes, OrbuResult* result)
{
    if (!result || (n > 0 && !frame_ids) || n < 0 || nkf < 0 || (nkf > 0 && !kf_list) || max_keyframes < 0) return fail(ORBX_E_INVALID, "bad argument");
    memset(result, 0, sizeof *result);
    if (n > ORBU_MAX_FRAME_POINTS) return fail(ORBX_E_UNSUPPORTED, "%d frame points: above %d", n, ORBU_MAX_FRAME_POINTS);
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if (given && nkf > s->kfcap) return fail(ORBX_E_INVALID, "%d keyframes for a store of %d", nkf, s->kfcap);
    for (int i = 0; i < nkf; i++)
        if ((rc = orbu_check_slot(s, "kf_list", i, kf_list[i], false))) return rc;
    if ((rc = orbw_check_ids(p, "frame_ids", frame_ids, n, true))) return rc;
    Packer pk;
    const size_t oIds = pk.take((size_t)n * 4), oList = pk.take((size_t)nkf * 4);
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, pk.off + 16))) return rc;   // (a resident search in flight reads S)
    s->updated = false; s->updates++;
    hipStream_t st = p->stream;
    if ((rc = orbu_next_generation(s, st, &s->scr.gen))) return rc;
    if (n) memcpy(s->h_stage + oIds, frame_ids, (size_t)n * 4);
    if (nkf) memcpy(s->h_stage + oList, kf_list, (size_t)nkf * 4);
    const int32_t* ids = (const int32_t*)(s->h_stage + oIds);
    const int32_t* list = given ? (const int32_t*)(s->h_stage + oList) : nullptr;
    const unsigned stampBlocks = (unsigned)std::max(1, (std::max(n, nkf) + orbu::kThreads - 1) / orbu::kThreads);
    hipLaunchKernelGGL(orbu::k_stamp, dim3(stampBlocks), dim3(orbu::kThreads), 0, st, s->scr, ids, n, list, nkf, s->out);
    if (!given) {
        if (s->hi) hipLaunchKernelGGL(orbu::k_vote, dim3((unsigned)((s->hi + orbu::kWaves - 1) / orbu::kWaves)), dim3(orbu::kThreads), 0, st, s->dev, s->scr, s->hi, s->out);
        hipLaunchKernelGGL(orbu::k_select, dim3(1), dim3(orbu::kThreads), 0, st, s->dev, s->hi, max_keyframes, s->out);
    }
    // the walk's grid: any size is correct (the kernels stride over the chunks, whose number only the device knows); it is
    // sized for the list given, or for twice the last update's list and the reference's 80 with its last step's three at the least
    const size_t rows = given ? (size_t)nkf : (size_t)std::min(s->kfcap, std::max(2 * s->lastNkf + 16, 96));
    const unsigned blocks = (unsigned)std::min<size_t>(s->blocks, std::max<size_t>(1, (rows * s->pitch + orbu::kChunk - 1) / orbu::kChunk));
    hipLaunchKernelGGL(orbu::k_points_mark, dim3(blocks), dim3(orbu::kThreads), 0, st, s->dev, s->scr, s->out);
    hipLaunchKernelGGL(orbu::k_points_count, dim3(blocks), dim3(orbu::kThreads), 0, st, s->dev, s->scr, s->out);
    hipLaunchKernelGGL(orbu::k_points_scan, dim3(1), dim3(orbu::kThreads), 0, st, s->dev, s->out);
    hipLaunchKernelGGL(orbu::k_points_write, dim3(blocks), dim3(orbu::kThreads), 0, st, s->dev, s->scr, s->out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const int32_t* h = s->out.hHdr;
    result->status = h[orbu::H_STATUS]; result->kf_max = h[orbu::H_KFMAX];
    if (result->status == ORBU_NO_VOTES) { result->votes = s->out.hVotes; return ORBX_OK; }
    result->nL = h[orbu::H_NL];
    if (result->nL > s->maxL) return fail(ORBX_E_CAPACITY, "%d local points: the store holds max_local_points = %d", result->nL, s->maxL);
    result->nkf = h[orbu::H_NKF]; result->nS = h[orbu::H_NS];
    result->kf = s->out.hList; result->L = s->out.hL; result->seen = s->out.hSeen; result->votes = given ? nullptr : s->out.hVotes;
    s->updated = true; s->nS = result->nS;
    if (!given) s->lastNkf = result->nkf;
    return ORBX_OK;
}

extern "C" int orbu_update_local_map(orbu_store_t* store, const int32_t* frame_ids, int n, int max_keyframes, OrbuResult* result)
{
    return orbu_run(store, false, nullptr, 0, frame_ids, n, max_keyframes, result);
}

extern "C" int orbu_local_points(orbu_store_t* store, const int32_t* kf_list, int nkf, const int32_t* frame_ids, int n, OrbuResult* result)
{
    return orbu_run(store, true, kf_list, nkf, frame_ids, n, INT_MAX, result);
}

extern "C" int orbw_track_local_map_resident(orbm_frameset_t* fs, int slot, orbw_pool_t* pool, orbu_store_t* store, const OrbmProjParams* pp,
                                             const OrbwView* view, float th, const float* scale_factors, const float* level_breaks, int nlevels,
                                             const uint8_t* t_occ)
{
    int rc = orbw_check_args(view, nullptr, 0, scale_factors, level_breaks, nlevels, false);
    if (rc) return rc;
    if (!pp) return fail(ORBX_E_INVALID, "null argument");
    if ((rc = orbu_store_check(store))) return rc;
    if (store->pool != pool) return fail(ORBX_E_INVALID, "the store belongs to another pool");
    int nS;
    uint32_t updates;
    {
        std::lock_guard<std::mutex> l(pool->mu);
        if (!store->updated) return fail(ORBX_E_INVALID, "the store has no completed update");
        nS = store->nS; updates = store->updates;
    }
    return orbw_track(fs, slot, -1, pool, pp, view, nullptr, nS, th, scale_factors, level_breaks, nlevels, t_occ, store->out.S, store, store->serial, updates);
}
