// orbq_reloc_host.inc -- host side of Tracking::Relocalization behind PnPsolver::iterate (part of orbslamm_hip.hip; kernels:
// orbq_reloc_kernels.hip, ABI: include/orbslamm_reloc.h, DESIGN.md §8y).  One call = the checks, one packed upload (the job records |
// the jobs' ids), nine launches on the handle's stream whatever the jobs do (stage, and twice: project, candidates, resolve, stage),
// one copy down (outlier bytes | ids | results | status bytes | the jobs' state words, as they lie in the block), one synchronise.  A search that overflowed
// its share of the arena: the arena grows to the largest need and the whole call runs again, at most twice.

static_assert(sizeof(OrbqRelocJob) == 112 && sizeof(OrbqRelocResult) == 616, "orbslamm_reloc.h layouts");
static_assert(offsetof(OrbqRelocResult, opt) == 0, "orbq_drain reads rounds from the OrboResult at a record's head");
static_assert(sizeof(orbq::RelocJobDev) == 224, "the per-job upload size DESIGN.md section 8y states");
static_assert(ORBQ_RELOC_REJECTED == orbq::RELOC_REJECTED && ORBQ_RELOC_FIRST == orbq::RELOC_FIRST && ORBQ_RELOC_WIDE_SHORT == orbq::RELOC_WIDE_SHORT &&
              ORBQ_RELOC_SECOND == orbq::RELOC_SECOND && ORBQ_RELOC_NARROW_SHORT == orbq::RELOC_NARROW_SHORT && ORBQ_RELOC_THIRD == orbq::RELOC_THIRD &&
              ORBQ_RELOC_KEEP == orbq::kRelocKeep, "orbq exits");
static_assert(ORBQ_RELOC_ST_NOT_RUN == orbq::RST_NOT_RUN && ORBQ_RELOC_ST_NO_POINT == orbq::RST_NO_POINT && ORBQ_RELOC_ST_BAD == orbq::RST_BAD &&
              ORBQ_RELOC_ST_FOUND == orbq::RST_FOUND && ORBQ_RELOC_ST_OUT_OF_IMAGE == orbq::RST_OUT_OF_IMAGE && ORBQ_RELOC_ST_DISTANCE == orbq::RST_DISTANCE &&
              ORBQ_RELOC_ST_LEVEL_RANGE == orbq::RST_LEVEL_RANGE && ORBQ_RELOC_ST_IN_VIEW == orbq::RST_IN_VIEW, "orbq projection status codes");

extern "C" int orbq_debug_reloc_arena(orbm_t* h, int entries_per_job, int* last_runs) { return orbq_debug_arena(h, &orbm_handle::relocArena, entries_per_job, last_runs); }

// this entry's own argument checks, behind the shared ones (which have seen nlevels in range and the three level tables there)
static int orbq_reloc_check_args(const void* h, const void* pool, const void* store, const OrbqRelocJob* jobs, int n_jobs, int check_ori,
                                 const float* level_breaks, int nlevels)
{
    if (check_ori != 0 && check_ori != 1) return fail(ORBX_E_INVALID, "check_ori is 0 or 1");
    for (int l = 0; l < nlevels; l++)
        if (!(level_breaks[l] < level_breaks[l + 1])) return fail(ORBX_E_INVALID, "the break table does not ascend strictly at %d", l);
    for (int j = 0; j < n_jobs; j++) {
        const OrbqRelocJob& J = jobs[j];
        if (J.kf_slot < 0 || J.slot < 0 || J.kf < 0) return fail(ORBX_E_INVALID, "job %d: negative slot", j);
        if (J.n && !J.ids) return fail(ORBX_E_INVALID, "job %d: null array", j);
    }
    if (!h || !pool || !store) return fail(ORBX_E_INVALID, "null handle, pool or store");
    return ORBX_OK;
}

extern "C" int orbq_relocalize(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const OrbqRelocJob* jobs, int n_jobs, int check_ori,
                               const float* inv_level_sigma2, const float* scale_factors, const float* level_breaks, int nlevels,
                               OrbqRelocResult* out, int32_t* const* ids_out, uint8_t* const* outlier_out, uint8_t* const* status_out)
{
    if (n_jobs == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbq_check_shared(jobs, n_jobs, out, ids_out, outlier_out, inv_level_sigma2 && scale_factors && level_breaks, nlevels, "no level table", "null array");
    if (rc || (rc = orbq_reloc_check_args(h, pool, store, jobs, n_jobs, check_ori, level_breaks, nlevels))) return rc;
    if ((rc = orbm_check(h)) || (rc = orbw_pool_check(pool)) || (rc = orbu_store_check(store))) return rc;
    if (pool->h->device != h->device) return fail(ORBX_E_INVALID, "the pool and the handle must share the device");
    if (store->pool != pool) return fail(ORBX_E_INVALID, "the store stands beside another pool");
    const size_t stride = (size_t)store->stride, nj = (size_t)n_jobs;
    size_t total = 0, sumCap = 0, sumTab = 0;
    int maxCap = 0, maxCell = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbqRelocJob& J = jobs[j];
        if ((rc = orbq_check_frameset(h, J.fs, j, J.kf_slot, J.slot, J.n, /* no second count */ -1, sumCap))) return rc;
        if (store->stride > J.fs->cap) return fail(ORBX_E_INVALID, "job %d: the store's stride %d is above the frame set's cap %d", j, store->stride, J.fs->cap);
        if ((rc = orbu_check_slot(store, "kf of job", j, J.kf, false))) return rc;   // (kfcap never changes; the set byte: under the mutex, below)
        total += (size_t)J.n;
        sumTab += 2 * (size_t)pow2ceil(std::max(J.n, 1));
        maxCap = std::max(maxCap, J.fs->cap); maxCell = std::max(maxCell, J.fs->ncell);
    }
    ProjPlan pl{};
    if ((rc = proj_lds_plan(maxCap, store->stride, maxCell, pl))) return rc;
    orbt::ProjCommon& c = pl.c;
    c.mode = 5; c.nnratio = 0.f; c.checkOri = check_ori; c.thDist = 100;
    proj_plan_queries(c, n_jobs);
    Packer pk;
    const size_t oJobs = pk.take(nj * sizeof(orbq::RelocJobDev)), oIdsIn = pk.take(total * 4), upBytes = pk.off;
    // cleared to -1 / 0xff in one piece: the sFound tables | the outlier bytes (ORBQ_RELOC_KEEP)
    const size_t oTab = pk.take(sumTab * 4), oOutl = pk.take(total), oFF = pk.off;
    const size_t oIds = pk.take(total * 4);
    // cleared to 0 in one piece: results | status | state | need | bad | the searches' candidate counters
    const size_t oOut = pk.take(nj * sizeof(OrbqRelocResult)), oStatus = pk.take(nj * 2 * stride), oState = pk.take(nj * 4), oNeed = pk.take(nj * 8),
                 oBad = pk.take(nj * 4), oTotal = pk.take(nj * 4), oZero = pk.off;
    // (what goes down lies in one piece: outlier bytes | ids | the zero-cleared head)
    const size_t downBytes = oZero - oOutl;
    const size_t oPw = pk.take(total * sizeof(float4)), oUv = pk.take(total * sizeof(float2)), oFlags = pk.take(total);
    const size_t oTocc = pk.take(sumCap), oToccOut = pk.take(sumCap), oAssign = pk.take(sumCap * 4);
    const size_t oUvr = pk.take(nj * stride * 12), oLvl = pk.take(nj * stride * 2), oQd = pk.take(nj * stride * 32), oQv = pk.take(nj * stride);
    const size_t oCandOff = pk.take(nj * stride * 4), oCandCnt = pk.take(nj * stride * 4), oQres = pk.take(nj * stride * 4), oQscr = pk.take(nj * stride * 12);
    const size_t oTscr = c.big ? pk.take(nj * (size_t)c.tCap * 12) : 0, oNm = pk.take(nj * 4), oPairs = pk.take(nj * sizeof(orbt::ProjPair)), work = pk.off;
    const size_t hOutl = 0, hIds = oIds - oOutl, hHead = oOut - oOutl;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    std::lock_guard<std::mutex> l(pool->mu);   // (held to the synchronise: no setter and no store update runs under the reads)
    for (int j = 0; j < n_jobs; j++) {
        if ((rc = orbu_check_slot(store, "kf of job", j, jobs[j].kf, true))) return rc;
        if ((rc = orbw_check_ids(pool, "ids", jobs[j].ids, jobs[j].n, true))) return fail(rc, "job %d: %s", j, std::string(g_err).c_str());
    }
    hipStream_t s = h->stream;
    for (int attempt = 0;; attempt++) {
        size_t arena;
        if ((rc = orbq_arena_reserve(h, h->relocArena, S_RELOC_ARENA, attempt, nj, std::max<size_t>(8 * stride, 2048), arena))) return rc;
        uint8_t* hs = (uint8_t*)h->h_stage;
        uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
        orbq::RelocJobDev* hj = (orbq::RelocJobDev*)(hs + oJobs);
        size_t f0 = 0, c0 = 0, tab0 = 0;
        for (int j = 0; j < n_jobs; j++) {
            const OrbqRelocJob& J = jobs[j];
            const orbm_frameset* fs = J.fs;
            const int64_t C = fs->cap;
            orbq::RelocJobDev& D = hj[j];
            memset(&D, 0, sizeof D);
            memcpy(D.Tcw, J.frame.Tcw, sizeof D.Tcw);
            memcpy(D.K, J.frame.K, sizeof D.K);
            memcpy(D.bounds, fs->bounds, sizeof D.bounds);
            D.cur = orbt::train_side(fs->fs, J.slot, fs->gd);
            D.kfAng = fs->fs.ang + J.kf_slot * C; D.nKf = fs->fs.n + J.kf_slot;
            D.entries = store->dev.entries + (size_t)J.kf * store->pitch;
            D.ids = (const int32_t*)(d + oIdsIn) + f0;
            D.n = J.n; D.f0 = (int32_t)f0; D.cap = fs->cap; D.c0 = (int32_t)c0;
            const int tabWords = 2 * pow2ceil(std::max(J.n, 1));
            D.tab0 = (int32_t)tab0; D.tabMask = tabWords - 1;
            D.t0 = (int32_t)((size_t)j * c.tCap * 3);
            if (J.n) memcpy(hs + oIdsIn + f0 * 4, J.ids, (size_t)J.n * 4);
            f0 += (size_t)J.n; c0 += (size_t)C; tab0 += (size_t)tabWords;
        }
        orbq::RelocArgs a{};
        orbq_fill_solver(a.q, pool, d, oPw, oUv, oFlags, oIds, oIds, oOutl, inv_level_sigma2, nlevels);   // (merged and idsOut: ONE array, the frame's point list)
        a.jobs = (const orbq::RelocJobDev*)(d + oJobs);
        a.out = (OrbqRelocResult*)(d + oOut);
        a.state = (int32_t*)(d + oState); a.need = (int32_t*)(d + oNeed); a.bad = (int32_t*)(d + oBad); a.table = (int32_t*)(d + oTab);
        a.tocc = d + oTocc; a.toccOut = d + oToccOut; a.assign = (int32_t*)(d + oAssign);
        a.quvr = (float*)(d + oUvr); a.qlvl = (int8_t*)(d + oLvl); a.qdesc = (uint4*)(d + oQd); a.qvalid = d + oQv; a.status = d + oStatus;
        a.candOff = (int32_t*)(d + oCandOff); a.candCnt = (int32_t*)(d + oCandCnt); a.qres = (int32_t*)(d + oQres); a.qscr = (int32_t*)(d + oQscr);
        a.tscr = c.big ? (int32_t*)(d + oTscr) : nullptr; a.total = (int32_t*)(d + oTotal); a.nmatch = (int32_t*)(d + oNm);
        a.cand = slot_ptr<uint2>(h, S_RELOC_ARENA); a.candCap = (int32_t)arena;
        a.pairs = (orbt::ProjPair*)(d + oPairs);
        a.stride = store->stride;
        for (int lv = 0; lv < ORBX_MAX_LEVELS; lv++) a.scale[lv] = lv < nlevels ? scale_factors[lv] : 0.f;
        for (int lv = 0; lv <= ORBX_MAX_LEVELS; lv++) a.breaks[lv] = lv <= nlevels ? level_breaks[lv] : 0.f;
        HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(d + oTab, 0xFF, oFF - oTab, s));
        HIPCHK(hipMemsetAsync(d + oOut, 0, oZero - oOut, s));   // (the records' padding too: the same bytes every call)
        const dim3 gProj((unsigned)((stride + orbq::kRelocThreads - 1) / orbq::kRelocThreads), (unsigned)n_jobs);
        hipLaunchKernelGGL(orbq::k_reloc_stage, dim3((unsigned)n_jobs), dim3(orbq::kLanes), 0, s, a, n_jobs, (int)orbq::RELOC_BEGIN);
        for (int search = 0; search < 2; search++) {
            c.thDist = search == 0 ? 100 : 64;                          // Tracking.cc:1515 / :1529
            hipLaunchKernelGGL(orbq::k_reloc_project, gProj, dim3(orbq::kRelocThreads), 0, s, a, search, search == 0 ? 10.f : 3.f);
            if ((rc = proj_launch(h, a.pairs, n_jobs, store->stride, pl, s))) {
                (void)hipStreamSynchronize(s);   // (the kernels in flight read the pool: they end before the mutex is let go)
                return rc;
            }
            hipLaunchKernelGGL(orbq::k_reloc_stage, dim3((unsigned)n_jobs), dim3(orbq::kLanes), 0, s, a, n_jobs, (int)orbq::RELOC_MIDDLE + search);
        }
        const uint8_t* head = hs + hHead;   // (the zero-cleared head as it came down: results | status | state | need | bad)
        if ((rc = orbq_drain("orbq_relocalize", pool, s, hs, d + oOutl, downBytes, head, sizeof(OrbqRelocResult), n_jobs, nlevels, ""))) return rc;
        const int32_t* bad = (const int32_t*)(head + (oBad - oOut));
        for (int j = 0; j < n_jobs; j++)
            if (bad[j]) return fail(ORBX_E_INVALID, "job %d: a row entry at or above the keyframe slot's device count holds a point", j);
        bool again;
        if ((rc = orbq_arena_grow(h->relocArena, attempt, (const int32_t*)(head + (oNeed - oOut)), n_jobs, again))) return rc;
        if (again) continue;
        orbq_hand_back(jobs, n_jobs, out, head, sizeof(OrbqRelocResult), hs + hIds, hs + hOutl, ids_out, outlier_out);
        for (int j = 0; j < n_jobs; j++)
            if (status_out && status_out[j]) memcpy(status_out[j], head + (oStatus - oOut) + (size_t)j * 2 * stride, 2 * stride);
        return ORBX_OK;
    }
}
