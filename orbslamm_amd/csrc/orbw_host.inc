// orbw_host.inc -- host side of the map-point pool and of the two tracking searches that run from it (part of
// orbslamm_hip.hip; kernels: orbw_kernels.hip, ABI: include/orbslamm_mappool.h, DESIGN.md §8q).
//   the pool      struct orbw_pool, its checks, the reader / writer steps and the last-wins staging: orbx_poolutil.inc
//   the searches  orbm_track_local_points / orbm_track_frame_projected (orbt_host.inc: track_queries) with the query block
//                 made by k_view_project instead of uploaded: the same result ring, the same two search launches

static_assert(sizeof(OrbwPoint) == 68 && sizeof(OrbwView) == 96, "orbslamm_mappool.h layouts");
static_assert(sizeof(orbw::StagedPoint) == 80, "a staged record is five 16-byte pieces");
static_assert(ORBW_ST_BAD == orbw::ST_BAD && ORBW_ST_DEPTH == orbw::ST_DEPTH && ORBW_ST_OUT_OF_IMAGE == orbw::ST_OUT_OF_IMAGE &&
              ORBW_ST_DISTANCE == orbw::ST_DISTANCE && ORBW_ST_VIEW_ANGLE == orbw::ST_VIEW_ANGLE && ORBW_ST_LEVEL_RANGE == orbw::ST_LEVEL_RANGE &&
              ORBW_ST_IN_VIEW == orbw::ST_IN_VIEW && ORBW_ST_NO_POINT == orbw::ST_NO_POINT, "orbw status codes");

extern "C" int orbw_pool_create(orbm_t* h, int capacity, orbw_pool_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    if (capacity <= 0) return fail(ORBX_E_INVALID, "capacity %d", capacity);
    if (capacity > ORBW_POOL_MAX_CAPACITY) return fail(ORBX_E_UNSUPPORTED, "capacity %d: above %d", capacity, ORBW_POOL_MAX_CAPACITY);
    int rc = orbm_check(h);
    if (rc) return rc;
    orbw_pool* p = new orbw_pool();
    p->cap = capacity;
    const size_t C = ((size_t)capacity + 3) & ~(size_t)3;
    const size_t bytes = C * (16 + 16 + 4 + 32);
    auto bail = [&](int code) { if (p->stream) (void)hipStreamDestroy(p->stream); if (p->d_block) (void)hipFree(p->d_block); delete p; return code; };
    HIPCHK_OR(hipMalloc(&p->d_block, bytes), bail(0));
    HIPCHK_OR(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking), bail(0));
    HIPCHK_OR(hipMemsetAsync(p->d_block, 0, bytes, p->stream), bail(0));
    HIPCHK_OR(hipStreamSynchronize(p->stream), bail(0));
    p->dev.a = (float4*)p->d_block; p->dev.b = p->dev.a + C; p->dev.desc = (uint4*)(p->dev.b + C); p->dev.flags = (uint32_t*)(p->dev.desc + 2 * C);
    p->dev.cap = capacity;
    p->setBits.assign(((size_t)capacity + 63) / 64, 0);
    p->seen.assign(p->setBits.size(), 0);
    p->h = h; h->refs++;
    h->nDevAlloc++;
    live_add(p);
    *out = p;
    return ORBX_OK;
}

extern "C" int orbw_pool_destroy(orbw_pool_t* p)
{
    if (!p) return ORBX_OK;
    live_remove(p);
    (void)hipSetDevice(p->h->device);
    {
        std::lock_guard<std::mutex> l(p->mu);
        for (auto& r : p->readers) { (void)hipEventSynchronize(r.ev); (void)hipEventDestroy(r.ev); }
        (void)hipStreamSynchronize(p->stream);
        (void)hipStreamDestroy(p->stream);
        (void)hipFree(p->d_block);
        if (p->h_stage) (void)hipHostFree(p->h_stage);
    }
    orbm_release(p->h);
    delete p;
    return ORBX_OK;
}

// both setters: pts != null writes whole records, else flags alone
static int orbw_pool_write(orbw_pool* p, const int32_t* ids, const OrbwPoint* pts, const uint8_t* flags, int n)
{
    if (n == 0) return ORBX_OK;
    if (n < 0) return fail(ORBX_E_INVALID, "negative count");
    if (!ids || (!pts && !flags)) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbw_pool_check(p);
    if (rc) return rc;
    std::lock_guard<std::mutex> l(p->mu);
    if ((rc = orbw_check_ids(p, "ids", ids, n, false, !pts))) return rc;
    const size_t rec = pts ? sizeof(orbw::StagedPoint) : sizeof(uint2);
    if ((rc = orbw_begin_write(p, p->h_stage, p->stageCap, (size_t)std::min(n, kPoolChunk) * rec))) return rc;
    // (captured by value: the staged loop keeps the pointers in registers across its byte copies)
    uint8_t* const stage = p->h_stage; const orbw::PoolDev dev = p->dev; hipStream_t const st = p->stream;
    auto emit = [=](int i, int m) {
        if (pts) {
            orbw::StagedPoint& s = ((orbw::StagedPoint*)stage)[m];
            const OrbwPoint& P = pts[i];
            s.a = make_float4(P.pos[0], P.pos[1], P.pos[2], P.min_distance);
            s.b = make_float4(P.normal[0], P.normal[1], P.normal[2], P.max_distance);
            memcpy(&s.d0, P.desc, 16); memcpy(&s.d1, P.desc + 16, 16);
            s.flags = P.flags; s.id = (uint32_t)ids[i]; s.pad[0] = s.pad[1] = 0;
        } else
            ((uint2*)stage)[m] = make_uint2((uint32_t)ids[i], flags[i]);
    };
    auto flush = [=](int m) -> int {
        hipLaunchKernelGGL(orbw::k_pool_scatter, dim3((unsigned)((m + orbw::kThreads - 1) / orbw::kThreads)), dim3(orbw::kThreads), 0, st,
                           dev, (const void*)stage, m, pts ? 0 : 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        return ORBX_OK;
    };
    if ((rc = stage_last_wins(ids, n, kPoolChunk, kPoolChunk, p->seen, emit, flush))) return rc;
    if (pts) for (int i = 0; i < n; i++) p->setBits[(size_t)ids[i] >> 6] |= 1ull << (ids[i] & 63);
    return ORBX_OK;
}

extern "C" int orbw_pool_set(orbw_pool_t* pool, const int32_t* ids, const OrbwPoint* pts, int n)
{
    if (n > 0 && !pts) return fail(ORBX_E_INVALID, "null argument");
    return orbw_pool_write(pool, ids, pts, nullptr, n);
}

extern "C" int orbw_pool_set_flags(orbw_pool_t* pool, const int32_t* ids, const uint8_t* flags, int n)
{
    if (n > 0 && !flags) return fail(ORBX_E_INVALID, "null argument");
    return orbw_pool_write(pool, ids, nullptr, flags, n);
}

// what needs neither a handle nor a GPU: the view record, the tables and the count of a projection
static int orbw_check_args(const OrbwView* view, const int32_t* ids, int nq, const float* scale_factors, const float* level_breaks, int nlevels, bool frame)
{
    if (nq < 0) return fail(ORBX_E_INVALID, "negative query count");
    if (!view || (nq && !ids) || !scale_factors || (!frame && !level_breaks)) return fail(ORBX_E_INVALID, "null argument");
    if (nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d]", nlevels, ORBX_MAX_LEVELS);
    if (!frame)
        for (int j = 0; j < nlevels; j++)
            if (!(level_breaks[j] < level_breaks[j + 1])) return fail(ORBX_E_INVALID, "the break table does not ascend strictly at %d", j);
    return ORBX_OK;
}

static orbw::ViewArgs orbw_view_args(const OrbwView* v, float th, const float* scale_factors, const float* level_breaks, int nlevels, bool frame)
{
    orbw::ViewArgs V{};
    memcpy(V.Rcw, v->Rcw, sizeof V.Rcw); memcpy(V.tcw, v->tcw, sizeof V.tcw); memcpy(V.Ow, v->Ow, sizeof V.Ow);
    V.fx = v->K[0]; V.fy = v->K[1]; V.cx = v->K[2]; V.cy = v->K[3];
    V.minX = v->min_x; V.maxX = v->max_x; V.minY = v->min_y; V.maxY = v->max_y; V.cosLimit = v->viewing_cos_limit;
    V.th = th; V.nlevels = nlevels; V.frame = frame ? 1 : 0;
    for (int l = 0; l < nlevels; l++) V.scale[l] = scale_factors[l];
    if (!frame) for (int l = 0; l <= nlevels; l++) V.breaks[l] = level_breaks[l];
    return V;
}

static inline unsigned orbw_blocks(int nq, size_t head16) { return (unsigned)((nq + orbw::kThreads - 1) / orbw::kThreads + (head16 + orbw::kThreads - 1) / orbw::kThreads); }

// the projection kernel alone on handle h's stream `st`, synchronous: ids up, the four arrays down.  lastKeys / lastN: the
// resident LastFrame of the frame/frame gate set, else null
static int orbw_project_sync(orbm_handle* h, hipStream_t st, orbw_pool* pool, const orbw::ViewArgs& V, const int32_t* ids, int nq,
                             const orbm::KeyDev* lastKeys, const int32_t* lastN, float* out_uvr, int8_t* out_lvl, float* out_viewcos, uint8_t* out_status)
{
    int rc;
    Packer pk;
    const size_t oIds = pk.take((size_t)nq * 4), up = pk.off;
    const size_t oUvr = pk.take((size_t)nq * 12), oLvl = pk.take((size_t)nq * 2), oCos = pk.take((size_t)nq * 4), oSt = pk.take((size_t)nq),
                 oQv = pk.take((size_t)nq), oQo = pk.take((size_t)nq), work = pk.off;
    const size_t down = oQv - oUvr;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(up, down)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    memcpy(hs, ids, (size_t)nq * 4);
    std::lock_guard<std::mutex> l(pool->mu);
    if ((rc = orbw_check_ids(pool, "ids", ids, nq, V.frame != 0))) return rc;
    orbw::ProjectArgs a{};
    a.pool = pool->dev; a.ids = (const int32_t*)(d + oIds); a.nq = nq; a.lastKeys = lastKeys; a.lastN = lastN;
    a.quvr = (float*)(d + oUvr); a.qlvl = (int8_t*)(d + oLvl); a.qdesc = nullptr; a.qvalid = d + oQv; a.qobs = d + oQo;
    a.viewcos = (float*)(d + oCos); a.status = d + oSt;
    HIPCHK(hipMemcpyAsync(d, hs, up, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(orbw::k_view_project, dim3(orbw_blocks(nq, 0)), dim3(orbw::kThreads), 0, st, a, V);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oUvr, down, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));   // (under the pool's mutex: no setter runs before the kernel has read the pool)
    if (out_uvr) memcpy(out_uvr, hs, (size_t)nq * 12);
    if (out_lvl) memcpy(out_lvl, hs + (oLvl - oUvr), (size_t)nq * 2);
    if (out_viewcos) memcpy(out_viewcos, hs + (oCos - oUvr), (size_t)nq * 4);
    if (out_status) memcpy(out_status, hs + (oSt - oUvr), (size_t)nq);
    return ORBX_OK;
}

extern "C" int orbw_view_project(orbm_t* h, orbw_pool_t* pool, const OrbwView* view, const int32_t* ids, int nq, float th,
                                 const float* scale_factors, const float* level_breaks, int nlevels, float* out_uvr, int8_t* out_lvl,
                                 float* out_viewcos, uint8_t* out_status)
{
    if (nq == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbw_check_args(view, ids, nq, scale_factors, level_breaks, nlevels, false);
    if (rc) return rc;
    if ((rc = orbm_check(h)) || (rc = orbw_pool_check(pool))) return rc;
    if (pool->h->device != h->device) return fail(ORBX_E_INVALID, "the pool and the handle must share the device");
    if (nq > ORBW_POOL_MAX_CAPACITY) return fail(ORBX_E_UNSUPPORTED, "%d queries: above %d", nq, ORBW_POOL_MAX_CAPACITY);
    return orbw_project_sync(h, h->stream, pool, orbw_view_args(view, th, scale_factors, level_breaks, nlevels, false), ids, nq, nullptr, nullptr,
                             out_uvr, out_lvl, out_viewcos, out_status);
}

extern "C" int orbw_view_project_frame(orbm_frameset_t* fs, int last_slot, orbw_pool_t* pool, const OrbwView* view, const int32_t* last_ids,
                                       int nq, float th, const float* scale_factors, float* out_uvr, int8_t* out_lvl, uint8_t* out_status)
{
    if (nq == 0) return ORBX_OK;
    int rc = orbw_check_args(view, last_ids, nq, scale_factors, nullptr, 1, true);
    if (rc) return rc;
    if ((rc = frameset_check(fs)) || (rc = orbw_pool_check(pool))) return rc;
    if (pool->h->device != fs->owner->device) return fail(ORBX_E_INVALID, "the pool and the frame set must share the device");
    if (last_slot < 0 || last_slot >= fs->slots) return fail(ORBX_E_INVALID, "slot %d outside the frame set", last_slot);
    if (nq > fs->cap) return fail(ORBX_E_INVALID, "%d ids for a frame of at most %d features", nq, fs->cap);
    return orbw_project_sync(fs->owner, fs_stream(fs), pool, orbw_view_args(view, th, scale_factors, nullptr, fs->nlevels, true), last_ids, nq,
                             fs->fs.keysUn + (size_t)last_slot * fs->cap, fs->fs.n + last_slot, out_uvr, out_lvl, nullptr, out_status);
}

// track_queries (orbt_host.inc) with the query block made on the device: the set's staging holds pair record | occupancy (the
// head, brought up by the projection kernel's last workgroups) | ids (read where they lie); the device twin holds the query
// block behind them; the status bytes go straight into the pinned share.  qslot >= 0: the frame/frame gate set.  devIds: the
// ids lie on the device already (a keyframe store's S, orbu_host.inc: made there from set slots, so not checked again); `ids`
// is then null and nothing per query goes up; store / storeUpdates name that store and its update in the search's record
static int orbw_track(orbm_frameset_t* fs, int slot, int qslot, orbw_pool* pool, const OrbmProjParams* pp, const OrbwView* view, const int32_t* ids,
                      int nq, float th, const float* scale_factors, const float* level_breaks, int nlevels, const uint8_t* t_occ,
                      const int32_t* devIds = nullptr, const void* store = nullptr, uint64_t storeSerial = 0, uint32_t storeUpdates = 0)
{
    const bool frame = qslot >= 0;
    int rc = orbw_check_args(view, devIds ? devIds : ids, nq, scale_factors, level_breaks, frame ? 1 : nlevels, frame);
    if (rc) return rc;
    if (!pp) return fail(ORBX_E_INVALID, "null argument");
    if ((rc = frameset_check(fs)) || (rc = orbw_pool_check(pool))) return rc;
    if (pool->h->device != fs->owner->device) return fail(ORBX_E_INVALID, "the pool and the frame set must share the device");
    if (pp->mode < 3 || pp->mode > 6) return fail(ORBX_E_INVALID, "mode must be 3 .. 6");
    if (slot < 0 || slot >= fs->slots || qslot >= fs->slots) return fail(ORBX_E_INVALID, "slot outside the frame set");
    if (frame) nlevels = fs->nlevels;
    if (frame && nq > fs->cap) return fail(ORBX_E_INVALID, "%d ids for a frame of at most %d features", nq, fs->cap);
    const size_t C = (size_t)fs->cap, S = (size_t)fs->slots;
    if ((size_t)nq > S * C || nq > orbt::kMaxQueryIters * orbt::kThreads)
        return fail(ORBX_E_UNSUPPORTED, "%d queries: the set's scratch holds slots x cap = %zu", nq, S * C);
    if (!devIds) {   // (set bits are never cleared: ids good now are good at the launch below)
        std::lock_guard<std::mutex> l(pool->mu);
        if ((rc = orbw_check_ids(pool, "ids", ids, nq, frame))) return rc;
    }
    const int set = fs->res.next();
    ResultRecord& r = fs->res.rec[set];
    Packer pk;
    const size_t oPair = pk.take(sizeof(orbt::ProjPair)), oOcc = t_occ ? pk.take(C) : 0, head = pk.off;
    const size_t oIds = pk.take(devIds ? 0 : (size_t)nq * 4);
    const size_t oUvr = pk.take((size_t)nq * 12), oLvl = pk.take((size_t)nq * 2), oQd = frame ? 0 : pk.take((size_t)nq * 32);
    const size_t oQv = pk.take((size_t)nq), oQo = pk.take((size_t)nq), oSt = pk.take((size_t)nq);
    const size_t total = pk.off;
    if ((rc = query_block_take(fs, set, total))) return rc;
    if ((rc = fs->res.begin(set))) return rc;
    ProjPlan& pl = r.plan;
    if ((rc = proj_lds_plan(fs->cap, nq, fs->ncell, pl))) return rc;
    orbt::ProjCommon& c = pl.c;
    c.mode = pp->mode; c.nnratio = pp->nnratio; c.thDist = pp->th_dist;
    c.checkOri = frame ? pp->check_ori : 0;
    proj_plan_queries(c, 1);
    uint8_t* hs = fs->h_q + (size_t)set * fs->qBytes;
    uint8_t* ds = fs->d_q + (size_t)set * fs->qBytes;
    if (nq && !devIds) memcpy(hs + oIds, ids, (size_t)nq * 4);
    if (t_occ) memcpy(hs + oOcc, t_occ, C);
    const SetTables t = set_tables(fs, set);
    orbt::ProjPair P{};
    orbt::proj_train(P, orbt::train_side(fs->fs, slot, fs->gd));
    P.quvr = (const float*)(ds + oUvr); P.qlvl = (const int8_t*)(ds + oLvl);
    P.qdesc = frame ? fs->fs.desc + (int64_t)qslot * C * 32 : ds + oQd;
    P.qang = frame ? fs->fs.ang + (int64_t)qslot * C : nullptr;
    P.qvalid = ds + oQv; P.qobs = ds + oQo;
    P.nqPtr = frame ? fs->fs.n + qslot : nullptr; P.nq = nq;
    P.toccIn = t_occ ? ds + oOcc : nullptr; P.toccOut = fs->d_occ;
    P.assign = t.assign; P.initAssign = 1; P.nmatch = t.nmatch; P.stats = t.stats; P.flag = t.flag; P.flagValue = fs->seq + 1;
    P.total = fs->d_total; P.candOff = fs->d_candOff; P.candCnt = fs->d_candCnt; query_arena(fs, P);
    P.qres = fs->d_qres; P.qscr = fs->d_qscr; P.tscr = c.big ? fs->d_tscr : nullptr;
    memcpy(hs + oPair, &P, sizeof P);
    r.pp = *pp; r.builds = fs->builds; r.slot = slot; r.qslot = qslot; r.nq = nq; r.total = head; r.qEpoch = fs->qEpoch;
    r.fromPool = true; r.oStatus = oSt; r.pool = pool; r.poolSerial = pool->serial; r.oIds = oIds; r.store = store; r.storeSerial = storeSerial; r.storeUpdates = storeUpdates;
    orbw::ProjectArgs a{};
    a.pool = pool->dev; a.ids = devIds ? devIds : (const int32_t*)(hs + oIds); a.nq = nq;
    a.lastKeys = frame ? fs->fs.keysUn + (size_t)qslot * C : nullptr; a.lastN = frame ? fs->fs.n + qslot : nullptr;
    a.quvr = (float*)(ds + oUvr); a.qlvl = (int8_t*)(ds + oLvl); a.qdesc = frame ? nullptr : (uint4*)(ds + oQd); a.qvalid = ds + oQv; a.qobs = ds + oQo;
    a.viewcos = nullptr; a.status = hs + oSt;
    a.headSrc = (const uint4*)hs; a.headDst = (uint4*)ds; a.head16 = (int32_t)(head / 16);
    const orbw::ViewArgs V = orbw_view_args(view, th, scale_factors, level_breaks, nlevels, frame);
    hipStream_t st = fs_stream(fs);
    {
        std::lock_guard<std::mutex> l(pool->mu);
        hipLaunchKernelGGL(orbw::k_view_project, dim3(orbw_blocks(nq, head / 16)), dim3(orbw::kThreads), 0, st, a, V);
        HIPCHK(hipGetLastError());
        if ((rc = orbw_mark_reader(pool, st))) return rc;
    }
    if ((rc = proj_launch(fs->owner, (const orbt::ProjPair*)ds, 1, nq, pl, st))) return rc;
    HIPCHK(hipEventRecord(r.ev, st));
    fs->res.commit(set, ResultRecord::kQueries, 1, ++fs->seq);
    return ORBX_OK;
}

extern "C" int orbw_track_local_map(orbm_frameset_t* fs, int slot, orbw_pool_t* pool, const OrbmProjParams* pp, const OrbwView* view,
                                    const int32_t* ids, int nq, float th, const float* scale_factors, const float* level_breaks, int nlevels,
                                    const uint8_t* t_occ)
{
    return orbw_track(fs, slot, -1, pool, pp, view, ids, nq, th, scale_factors, level_breaks, nlevels, t_occ);
}

extern "C" int orbw_track_frame_pose(orbm_frameset_t* fs, int cur_slot, int last_slot, orbw_pool_t* pool, const OrbmProjParams* pp,
                                     const OrbwView* view, const int32_t* last_ids, int nq, float th, const float* scale_factors, const uint8_t* t_occ)
{
    if (last_slot < 0) return fail(ORBX_E_INVALID, "bad argument");
    return orbw_track(fs, cur_slot, last_slot, pool, pp, view, last_ids, nq, th, scale_factors, nullptr, 1, t_occ);
}

extern "C" int orbw_track_status(orbm_frameset_t* fs, int back, const uint8_t** status, int* nq)
{
    if (!status || !nq) return fail(ORBX_E_INVALID, "null argument");
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (back < 0 || back >= ResultRing::kSets) return fail(ORBX_E_INVALID, "back must be 0 .. %d", ResultRing::kSets - 1);
    const int set = fs->res.back(back);
    const ResultRecord& r = fs->res.rec[set];
    if (!r.ev || r.kind != ResultRecord::kQueries || !r.fromPool) return fail(ORBX_E_INVALID, "that search was not issued from a map-point pool");
    if (r.qEpoch != fs->qEpoch) return fail(ORBX_E_CAPACITY, "a larger query search issued behind it reallocated the search's staging");
    if (!flags_raised(r, set_tables(fs, set).flag)) HIPCHK(hipEventSynchronize(r.ev));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    *status = fs->h_q + (size_t)set * fs->qBytes + r.oStatus;
    *nq = r.nq;
    return ORBX_OK;
}
