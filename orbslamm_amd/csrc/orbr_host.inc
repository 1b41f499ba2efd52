// orbr_host.inc -- host side of the map-point refresh over a keyframe store (part of orbslamm_hip.hip; kernels:
// orbr_kernels.hip, ABI: include/orbslamm_refresh.h, DESIGN.md §8w).
//   the store     the columns it reads (descriptors, centres, octaves) are the store's: set in orbu_host.inc, freed by orbu_store_destroy
//   the blocks    the pool-sized marks and the keys (one per entry of the store) at the first refresh, of fixed size; the
//                 per-point arrays grow with the largest n seen.  This file owns these alone
//   a call        orbr_issue (mark, count, segments, place, the two refresh kernels), the header down, one synchronisation;
//                 orbr_check_header; then the commit as a launch of its own, the records down into `out`, the second
//                 synchronisation.  orbe_correct_sim3 (orbe_host.inc) runs the same two functions inside its own block

static_assert(sizeof(OrbrPoint) == 4 * orbr::kRecWords && ORBR_MAX_OBS == orbr::kMaxObs && ORBU_MAX_STRIDE == 1 << orbr::kQBits, "orbslamm_refresh.h layouts");
static_assert(ORBR_ST_NOT_ASKED == orbr::ST_NOT_ASKED && ORBR_ST_DONE == orbr::ST_DONE && ORBR_ST_BAD == orbr::ST_BAD && ORBR_ST_NO_OBSERVATION == orbr::ST_NO_OBSERVATION &&
              ORBR_ST_ALL_KF_BAD == orbr::ST_ALL_KF_BAD && ORBR_ST_NO_REF == orbr::ST_NO_REF && ORBR_ST_LEVEL_RANGE == orbr::ST_LEVEL_RANGE, "orbr status codes");
static_assert(offsetof(OrbrPoint, desc) == 4 * orbr::R_DESC && offsetof(OrbrPoint, n_obs) == 4 * orbr::R_NOBS && offsetof(OrbrPoint, st_descriptor) == 4 * orbr::R_STATUS,
              "OrbrPoint as the kernels write it");

struct orbr_blocks {
    uint8_t* d_block = nullptr;                      // marks | keys | header
    uint8_t* d_pts = nullptr; size_t ptsCap = 0;     // cnt | start | fill | listShort | listLong | res, for the largest n so far
    orbr::Dev dev{};
};

static void orbr_release(orbu_store* s)
{
    if (!s->refresh) return;
    orbu_marks_drop(s, s->refresh->dev.mark);
    if (s->refresh->d_block) (void)hipFree(s->refresh->d_block);
    if (s->refresh->d_pts) (void)hipFree(s->refresh->d_pts);
    delete s->refresh;
    s->refresh = nullptr;
}

extern "C" int orbw_debug_pool_get(orbw_pool_t* p, const int32_t* ids, int n, OrbwPoint* out)
{
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (n == 0) return ORBX_OK;
    if (!ids || !out) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbw_pool_check(p);
    if (rc) return rc;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbw_check_ids(p, "ids", ids, n, false))) return rc;
    const size_t rec = sizeof(orbw::StagedPoint);
    const int chunk = std::min(n, kPoolChunk);
    Packer pk;
    const size_t oRec = pk.take((size_t)chunk * rec), oIds = pk.take((size_t)chunk * 4);
    if ((rc = grow_pinned(p->h_stage, p->stageCap, pk.off, true, &p->stream, &p->h->nHostAlloc))) return rc;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = std::min(chunk, n - c0);
        memcpy(p->h_stage + oIds, ids + c0, (size_t)m * 4);
        hipLaunchKernelGGL(orbr::k_pool_gather, dim3((unsigned)((m + orbr::kThreads - 1) / orbr::kThreads)), dim3(orbr::kThreads), 0, p->stream,
                           p->dev, (const int32_t*)(p->h_stage + oIds), m, (uint4*)(p->h_stage + oRec));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(p->stream));
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const orbw::StagedPoint* sp = (const orbw::StagedPoint*)(p->h_stage + oRec);
        for (int i = 0; i < m; i++) {
            OrbwPoint& o = out[c0 + i];
            o.pos[0] = sp[i].a.x; o.pos[1] = sp[i].a.y; o.pos[2] = sp[i].a.z; o.min_distance = sp[i].a.w;
            o.normal[0] = sp[i].b.x; o.normal[1] = sp[i].b.y; o.normal[2] = sp[i].b.z; o.max_distance = sp[i].b.w;
            memcpy(o.desc, &sp[i].d0, 16); memcpy(o.desc + 16, &sp[i].d1, 16);
            o.flags = (uint8_t)sp[i].flags; o.pad[0] = o.pad[1] = o.pad[2] = 0;
        }
    }
    return ORBX_OK;
}

// (the pool's mutex is held) the fixed blocks, and the per-point arrays for n points
static int orbr_blocks_ensure(orbu_store* s, int n)
{
    orbw_pool* p = s->pool;
    if (!s->refresh) {
        orbr_blocks* b = new orbr_blocks();
        const size_t P = (size_t)p->cap, E = (size_t)s->kfcap * s->pitch;
        Packer pk;
        const size_t oMark = pk.take(P * 8), oKeys = pk.take(E * 4), oHdr = pk.take(orbr::H_INTS * 4), bytes = pk.off;
        if (int rc = orbu_block_once(p, b->d_block, bytes, 0)) { delete b; return rc; }
        b->dev.mark = (unsigned long long*)(b->d_block + oMark); b->dev.keys = (uint32_t*)(b->d_block + oKeys); b->dev.hdr = (int32_t*)(b->d_block + oHdr);
        b->dev.keysCap = (int32_t)E; b->dev.pool = p->dev;
        s->refresh = b; s->marks[s->nMarks++] = {b->dev.mark, P * 8};
    }
    orbr_blocks* b = s->refresh;
    Packer pk;
    const size_t N = (size_t)n;
    const size_t oCnt = pk.take(N * 4), oStart = pk.take(N * 4), oFill = pk.take(N * 4), oShort = pk.take(N * 4), oLong = pk.take(N * 4),
                 oRes = pk.take(N * sizeof(OrbrPoint));
    int rc = grow_device(b->d_pts, b->ptsCap, pk.off, 1 << 16, &p->stream, &p->h->nDevAlloc);
    if (rc) return rc;
    b->dev.cnt = (int32_t*)(b->d_pts + oCnt); b->dev.start = (int32_t*)(b->d_pts + oStart); b->dev.fill = (int32_t*)(b->d_pts + oFill);
    b->dev.listShort = (int32_t*)(b->d_pts + oShort); b->dev.listLong = (int32_t*)(b->d_pts + oLong); b->dev.res = (uint32_t*)(b->d_pts + oRes);
    b->dev.desc = s->desc.d; b->dev.ctr = s->ctr.d; b->dev.oct = s->oct.d;
    return ORBX_OK;
}

// the observation index of c's points and their refresh, on stream st: what orbr_refresh_points and orbe_correct_sim3 launch alike
static void orbr_issue(const orbu_store* s, const orbr_blocks* b, const orbr::Call& c, hipStream_t st)
{
    const int n = c.n;
    const unsigned ptBlocks = (unsigned)((n + orbr::kThreads - 1) / orbr::kThreads);
    const unsigned walkBlocks = (unsigned)((s->hi + orbr::kWaves - 1) / orbr::kWaves);
    hipLaunchKernelGGL(orbr::k_mark, dim3(ptBlocks), dim3(orbr::kThreads), 0, st, b->dev, c);
    if (walkBlocks) hipLaunchKernelGGL(orbr::k_walk, dim3(walkBlocks), dim3(orbr::kThreads), 0, st, s->dev, b->dev, n, s->hi, 0);
    hipLaunchKernelGGL(orbr::k_segments, dim3(ptBlocks), dim3(orbr::kThreads), 0, st, b->dev, n);
    if (walkBlocks) hipLaunchKernelGGL(orbr::k_walk, dim3(walkBlocks), dim3(orbr::kThreads), 0, st, s->dev, b->dev, n, s->hi, 1);
    // (any grid is correct: the refresh kernels stride over their lists, whose lengths only the device knows)
    hipLaunchKernelGGL(orbr::k_refresh_short, dim3(std::min(4096u, (unsigned)((n + orbr::kGroups - 1) / orbr::kGroups))), dim3(orbr::kThreads), 0, st, s->dev, b->dev, c);
    hipLaunchKernelGGL(orbr::k_refresh_long, dim3(std::min(1024u, (unsigned)n)), dim3(orbr::kThreads), 0, st, s->dev, b->dev, c);
}

// the header words of orbr_issue as they came down.  whose: "a listed point", "a moved point"
static int orbr_check_header(const int32_t* hdr, int n, const orbr_blocks* b, const char* whose)
{
    if (hdr[orbr::H_ERR]) return fail(ORBX_E_UNSUPPORTED, "%s has more than %d observations", whose, ORBR_MAX_OBS);
    if (hdr[orbr::H_NSHORT] + hdr[orbr::H_NLONG] != n || hdr[orbr::H_TOTAL] < 0 || hdr[orbr::H_TOTAL] > b->dev.keysCap)
        return fail(ORBX_E_HIP, "the observation index holds %d + %d of %d points and %d keys", hdr[orbr::H_NSHORT], hdr[orbr::H_NLONG], n, hdr[orbr::H_TOTAL]);
    return ORBX_OK;
}

extern "C" int orbr_refresh_points(orbu_store_t* s, const int32_t* ids, const int32_t* ref_kf, const float* new_pos, int n, int what,
                                   const float* scale_factors, int nlevels, int commit, OrbrPoint* out)
{
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (n == 0) return ORBX_OK;
    if (!ids || !ref_kf || !scale_factors || !out) return fail(ORBX_E_INVALID, "null argument");
    if (what == 0 || (what & ~(ORBR_DESCRIPTOR | ORBR_NORMAL_DEPTH))) return fail(ORBX_E_INVALID, "what = %d", what);
    if (nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d]", nlevels, ORBX_MAX_LEVELS);
    if (new_pos)
        for (size_t i = 0; i < 3 * (size_t)n; i++)
            if (!std::isfinite(new_pos[i])) return fail(ORBX_E_INVALID, "new_pos[%zu] is not finite", i);
    int rc = orbu_store_check(s);
    if (rc) return rc;
    orbw_pool* p = s->pool;
    std::lock_guard<std::mutex> l(p->mu);
    if (n > p->cap) return fail(ORBX_E_UNSUPPORTED, "%d points for a pool of %d", n, p->cap);
    if ((rc = orbw_check_ids(p, "ids", ids, n, false))) return rc;
    const int dup = first_repeated_key(ids, n, p->seen);   // (the pool's scratch bits, all zero between calls)
    if (dup >= 0) return fail(ORBX_E_INVALID, "ids[%d] = %d is repeated within the call", dup, ids[dup]);
    for (int i = 0; i < n; i++)
        if ((rc = orbu_check_slot(s, "ref_kf", i, ref_kf[i], true, true))) return rc;
    if ((rc = orbu_check_columns(s, what & ORBR_DESCRIPTOR, what & ORBR_NORMAL_DEPTH, what & ORBR_NORMAL_DEPTH))) return rc;
    if ((rc = orbr_blocks_ensure(s, n))) return rc;
    Packer pk;
    const size_t oIds = pk.take((size_t)n * 4), oRef = pk.take((size_t)n * 4), oPos = pk.take(new_pos ? (size_t)n * 12 : 0), oSf = pk.take(ORBX_MAX_LEVELS * 4),
                 oHdr = pk.take(orbr::H_INTS * 4);
    if ((rc = orbw_begin_write(p, s->h_stage, s->stageCap, pk.off))) return rc;
    orbr_blocks* b = s->refresh;
    hipStream_t st = p->stream;
    if ((rc = orbu_next_generation(s, st, &b->dev.gen))) return rc;
    memcpy(s->h_stage + oIds, ids, (size_t)n * 4);
    memcpy(s->h_stage + oRef, ref_kf, (size_t)n * 4);
    if (new_pos) memcpy(s->h_stage + oPos, new_pos, (size_t)n * 12);
    memset(s->h_stage + oSf, 0, ORBX_MAX_LEVELS * 4);
    memcpy(s->h_stage + oSf, scale_factors, (size_t)nlevels * 4);
    orbr::Call c{};
    c.ids = (const int32_t*)(s->h_stage + oIds); c.ref = (const int32_t*)(s->h_stage + oRef);
    c.newPos = new_pos ? (const float*)(s->h_stage + oPos) : nullptr; c.sf = (const float*)(s->h_stage + oSf);
    c.n = n; c.what = what; c.nlevels = nlevels;
    int32_t* hdr = (int32_t*)(s->h_stage + oHdr);
    orbr_issue(s, b, c, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hdr, b->dev.hdr, orbr::H_INTS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if ((rc = orbr_check_header(hdr, n, b, "a listed point"))) return rc;
    if (commit) {
        hipLaunchKernelGGL(orbr::k_commit, dim3((unsigned)((n + orbr::kThreads - 1) / orbr::kThreads)), dim3(orbr::kThreads), 0, st, b->dev, c);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, b->dev.res, (size_t)n * sizeof(OrbrPoint), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ORBX_OK;
}
