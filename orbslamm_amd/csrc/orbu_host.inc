// orbu_host.inc -- host side of Tracking::UpdateLocalMap on the device (part of orbslamm_hip.hip; kernels: orbu_kernels.hip,
// ABI: include/orbslamm_localmap.h, DESIGN.md §8r).
//   the store     keyframe match lists, flags and graph records in HBM beside ONE map-point pool, whose mutex and stream it
//                 uses; a "set" byte per slot on the host; all blocks of a fixed size made at create, the staging grow-only
//   the call      stamp, vote, select, mark, count, scan, write on the pool's stream, one synchronisation; the kernels leave
//                 the result in the store's pinned block themselves
//   the search    orbw_track (orbw_host.inc) reading the store's S where it lies

static_assert(ORBU_ENTRY_NO_VOTE == orbu::kNoVote && ORBU_MAX_KEYFRAMES == orbu::kMaxKeyFrames && ORBU_MAX_NEIGHBOURS + 2 == orbu::kGraphInts,
              "orbslamm_localmap.h constants");

constexpr size_t kStoreMaxEntries = (size_t)1 << 28;   // kf_capacity * pitch: positions of the point walk fit 32 bits with room
constexpr size_t kStoreStageBytes = (size_t)8 << 20;   // a setter launch's staged records

struct orbn_blocks;                                    // orbn_host.inc: the covisibility entries' blocks, made at their first call
struct orbu_store;
static void orbn_release(orbu_store* s);
static int orbn_clear_marks(orbu_store* s, hipStream_t st);

struct orbu_store {
    uint64_t serial = ++g_poolSerial;
    orbw_pool* pool = nullptr;
    int kfcap = 0, stride = 0, pitch = 0, maxc = 0, maxcP = 0, maxL = 0;
    uint8_t* d_block = nullptr;
    orbu::StoreDev dev{};
    orbu::Scratch scr{};
    orbu::Out out{};
    uint8_t* h_res = nullptr;                          // pinned, coherent: header | list | votes | L | seen
    uint8_t* h_stage = nullptr; size_t stageCap = 0;   // pinned, coherent: a setter's records, or a call's ids and list
    std::vector<uint8_t> kfSet, kfSeen;                // kfSeen: a setter's scratch, all zero between calls
    std::vector<uint8_t> idxSeen;
    std::vector<int64_t> eOff, cOff; std::vector<int> lastOf;   // orbu_kf_write's scratch: they keep their capacity between calls
    int hi = 0;                                        // the highest set slot + 1
    uint32_t gen = 0;
    bool updated = false; int nS = 0;                  // the last update completed: S holds nS ids
    uint32_t updates = 0;                              // updates begun so far: each overwrites S
    unsigned blocks = 1;                               // the point walk's grid at the most: one block a chunk of the whole store, <= 1 024
    int lastNkf = 0;                                   // the local keyframes of the last update: sizes the next update's grid
    orbn_blocks* covis = nullptr;                      // orbn_*: null until the first call
    uint8_t* d_oct = nullptr;                          // orbu_kf_set_octaves: [kfcap * pitch] bytes, null until the first call
    std::vector<uint8_t> kfOct;                        // the slots that have octaves
    uint8_t octSeen[256] = {};                         // the octave values the store has been given
};

static int orbu_store_check(orbu_store* s)
{
    if (!s) return fail(ORBX_E_INVALID, "null store");
    if (!live_has(s)) return fail(ORBX_E_INVALID, "the store was destroyed");
    return orbw_pool_check(s->pool);
}

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
    s->kfSet.assign(K, 0); s->kfSeen.assign(K, 0); s->idxSeen.assign((size_t)stride, 0);
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
    (void)hipFree(s->d_block);
    (void)hipHostFree(s->h_res);
    if (s->h_stage) (void)hipHostFree(s->h_stage);
    if (h) orbm_release(h);
    delete s;
    return ORBX_OK;
}

// (the pool's mutex is held) an entry value: -1, or a pool id that is set, bit 30 aside
static int orbu_check_entry(const orbu_store* s, int32_t v, const char* what, int i)
{
    if (v == -1) return ORBX_OK;
    const int32_t id = v & ~ORBU_ENTRY_NO_VOTE;
    if (v < 0 || id >= s->pool->cap) return fail(ORBX_E_INVALID, "%s[%d] = %d outside the pool of %d", what, i, v, s->pool->cap);
    if (!s->pool->isSet(id)) return fail(ORBX_E_INVALID, "%s[%d]: pool id %d was never set", what, i, id);
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
    // every id, on the host, before any launch
    {
        int64_t e0 = 0, c0 = 0;
        for (int i = 0; i < nkf; i++) {
            const int k = kfs->slot[i];
            if (k < 0 || k >= s->kfcap) return fail(ORBX_E_INVALID, "slot[%d] = %d outside the store of %d", i, k, s->kfcap);
            if (!whole && !s->kfSet[k]) return fail(ORBX_E_INVALID, "slot[%d] = %d was never set", i, k);
            if (whole && kfs->n[i] > s->stride) return fail(ORBX_E_UNSUPPORTED, "record %d: %d entries for a stride of %d", i, kfs->n[i], s->stride);
            if (kfs->nchildren[i] > s->maxc) return fail(ORBX_E_UNSUPPORTED, "record %d: %d children, at most %d", i, kfs->nchildren[i], s->maxc);
            if (whole)
                for (int e = 0; e < kfs->n[i]; e++)
                    if ((rc = orbu_check_entry(s, kfs->entries[e0 + e], "entries", (int)(e0 + e)))) return rc;
            for (int j = 0; j < ORBU_MAX_NEIGHBOURS; j++) {
                const int nb = kfs->neigh[(size_t)i * ORBU_MAX_NEIGHBOURS + j];
                if (nb < -1 || nb >= s->kfcap) return fail(ORBX_E_INVALID, "record %d: neighbour %d outside the store of %d", i, nb, s->kfcap);
            }
            if (kfs->parent[i] < -1 || kfs->parent[i] >= s->kfcap) return fail(ORBX_E_INVALID, "record %d: parent %d outside the store of %d", i, kfs->parent[i], s->kfcap);
            for (int c = 0; c < kfs->nchildren[i]; c++) {
                const int ch = kfs->children[c0 + c];
                if (ch < 0 || ch >= s->kfcap) return fail(ORBX_E_INVALID, "record %d: child %d outside the store of %d", i, ch, s->kfcap);
            }
            if (whole) e0 += kfs->n[i];
            c0 += kfs->nchildren[i];
        }
    }
    const int recInts = orbu::kRecHead + s->maxcP + (whole ? s->pitch : 0);
    const int perLaunch = (int)std::max<size_t>(1, std::min<size_t>((size_t)nkf, kStoreStageBytes / ((size_t)recInts * 4)));
    if ((rc = grow_pinned(s->h_stage, s->stageCap, (size_t)perLaunch * recInts * 4, true, nullptr, &s->pool->h->nHostAlloc))) return rc;
    if ((rc = orbw_wait_readers(s->pool))) return rc;
    // the last record of a repeated slot wins: keep a slot's last sighting
    std::vector<int64_t>&eOff = s->eOff, &cOff = s->cOff;
    eOff.resize((size_t)nkf); cOff.resize((size_t)nkf);
    {
        int64_t e0 = 0, c0 = 0;
        for (int i = 0; i < nkf; i++) { eOff[i] = e0; cOff[i] = c0; if (whole) e0 += kfs->n[i]; c0 += kfs->nchildren[i]; }
    }
    std::vector<int>& lastOf = s->lastOf;
    lastOf.clear();
    for (int i = nkf - 1; i >= 0; i--) { uint8_t& b = s->kfSeen[kfs->slot[i]]; if (!b) { b = 1; lastOf.push_back(i); } }
    for (int i = 0; i < nkf; i++) s->kfSeen[kfs->slot[i]] = 0;
    int m = 0;
    int32_t* stage = (int32_t*)s->h_stage;
    auto flush = [&]() -> int {
        if (!m) return ORBX_OK;
        hipLaunchKernelGGL(orbu::k_kf_scatter, dim3((unsigned)m), dim3(orbu::kThreads), 0, s->pool->stream, s->dev, (const int32_t*)stage, recInts, s->maxcP, whole ? 0 : 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->pool->stream));   // (the staging is the next launch's; the call returns with the update complete)
        m = 0;
        return ORBX_OK;
    };
    for (size_t q = 0; q < lastOf.size(); q++) {
        const int i = lastOf[q];
        int32_t* rec = stage + (size_t)m * recInts;
        rec[0] = kfs->slot[i]; rec[1] = whole ? ((kfs->flags[i] & ORBU_KF_BAD) | ORBU_KF_SET) : 0;
        for (int j = 0; j < ORBU_MAX_NEIGHBOURS; j++) rec[2 + j] = kfs->neigh[(size_t)i * ORBU_MAX_NEIGHBOURS + j];
        rec[12] = kfs->parent[i]; rec[13] = kfs->nchildren[i]; rec[14] = rec[15] = 0;
        for (int c = 0; c < s->maxcP; c++) rec[orbu::kRecHead + c] = c < kfs->nchildren[i] ? kfs->children[cOff[i] + c] : -1;
        if (whole) {
            int32_t* ent = rec + orbu::kRecHead + s->maxcP;
            if (kfs->n[i]) memcpy(ent, kfs->entries + eOff[i], (size_t)kfs->n[i] * 4);
            for (int e = kfs->n[i]; e < s->pitch; e++) ent[e] = -1;
        }
        if (++m == perLaunch && (rc = flush())) return rc;
    }
    if ((rc = flush())) return rc;
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
    if (ent && (slot >= s->kfcap || !s->kfSet[slot])) return fail(ORBX_E_INVALID, "keyframe slot %d is outside the store of %d or was never set", slot, s->kfcap);
    for (int i = 0; i < n; i++) {
        if (ent) {
            if (a[i] < 0) return fail(ORBX_E_INVALID, "idx[%d] = %d", i, a[i]);
            if (a[i] >= s->stride) return fail(ORBX_E_UNSUPPORTED, "idx[%d] = %d for a stride of %d", i, a[i], s->stride);
            if ((rc = orbu_check_entry(s, vals[i], "vals", i))) return rc;
        } else {
            if (a[i] < 0 || a[i] >= s->kfcap) return fail(ORBX_E_INVALID, "slots[%d] = %d outside the store of %d", i, a[i], s->kfcap);
            if (!s->kfSet[a[i]]) return fail(ORBX_E_INVALID, "slots[%d] = %d was never set", i, a[i]);
        }
    }
    const int perLaunch = (int)std::min<size_t>((size_t)n, kStoreStageBytes / 8);
    if ((rc = grow_pinned(s->h_stage, s->stageCap, (size_t)perLaunch * 8, true, nullptr, &s->pool->h->nHostAlloc))) return rc;
    if ((rc = orbw_wait_readers(s->pool))) return rc;
    std::vector<uint8_t>& seen = ent ? s->idxSeen : s->kfSeen;
    int2* stage = (int2*)s->h_stage;
    for (int c0 = 0; c0 < n; c0 += perLaunch) {
        const int c1 = std::min(n, c0 + perLaunch);
        int m = 0;
        for (int i = c1 - 1; i >= c0; i--) {   // the last value of a repeated index wins (later launches land later)
            if (seen[a[i]]) continue;
            seen[a[i]] = 1;
            stage[m++] = make_int2(a[i], ent ? vals[i] : ((flags[i] & ORBU_KF_BAD) | ORBU_KF_SET));
        }
        for (int i = c0; i < c1; i++) seen[a[i]] = 0;
        hipLaunchKernelGGL(orbu::k_pair_scatter, dim3((unsigned)((m + orbu::kThreads - 1) / orbu::kThreads)), dim3(orbu::kThreads), 0, s->pool->stream,
                           s->dev, (const int2*)stage, m, ent ? slot : 0, ent ? 0 : 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->pool->stream));
    }
    return ORBX_OK;
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
        if (kf_list[i] < 0 || kf_list[i] >= s->kfcap) return fail(ORBX_E_INVALID, "kf_list[%d] = %d outside the store of %d", i, kf_list[i], s->kfcap);
    for (int i = 0; i < n; i++) {
        const int id = frame_ids[i];
        if (id == -1) continue;
        if (id < 0 || id >= p->cap) return fail(ORBX_E_INVALID, "frame_ids[%d] = %d outside the pool of %d", i, id, p->cap);
        if (!p->isSet(id)) return fail(ORBX_E_INVALID, "frame_ids[%d] = %d was never set", i, id);
    }
    Packer pk;
    const size_t oIds = pk.take((size_t)n * 4), oList = pk.take((size_t)nkf * 4);
    if ((rc = grow_pinned(s->h_stage, s->stageCap, pk.off + 16, true, nullptr, &p->h->nHostAlloc))) return rc;
    if ((rc = orbw_wait_readers(p))) return rc;   // a resident search in flight reads S
    s->updated = false; s->updates++;
    hipStream_t st = p->stream;
    if (s->gen == 0xffffffffu) {   // the tag wraps: one clear, and the tags start over
        HIPCHK(hipMemsetAsync(s->scr.stamp, 0, (size_t)p->cap * 8, st));
        HIPCHK(hipMemsetAsync(s->scr.first, 0xff, (size_t)p->cap * 8, st));
        if ((rc = orbn_clear_marks(s, st))) return rc;
        s->gen = 0;
    }
    s->scr.gen = ++s->gen;
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
