// orbq_motion_host.inc -- host side of Tracking::TrackWithMotionModel from the predicted pose to the counts (part of
// orbslamm_hip.hip; kernels: orbq_motion_kernels.hip, ABI: include/orbslamm_motion.h, DESIGN.md §8z).  One call = the checks, one
// packed upload (the job records | the jobs' last_ids), nine launches on the handle's stream whatever the jobs do (stage, and
// twice: project, candidates, resolve, stage), one copy down (outlier bytes | ids | tables | status bytes | results | the jobs'
// state words, as they lie in the block), one synchronise.  A search that overflowed its share of the arena: the arena grows to
// the largest need and the whole call runs again, at most twice.

static_assert(sizeof(OrbqMotionJob) == 176 && sizeof(OrbqMotionResult) == 264, "orbslamm_motion.h layouts");
static_assert(offsetof(OrbqMotionResult, track) == 0, "orbq_drain reads rounds from the OrboResult at a record's head");
static_assert(sizeof(orbq::MotionJobDev) == 288, "the per-job upload size DESIGN.md section 8z states");
static_assert(ORBQ_MM_TRACKED == orbq::MM_TRACKED && ORBQ_MM_TOO_FEW == orbq::MM_TOO_FEW && ORBQ_MM_ST_NOT_RUN == orbq::kMotionNotRun, "orbq motion codes");

extern "C" int orbq_debug_motion_arena(orbm_t* h, int entries_per_job, int* last_runs) { return orbq_debug_arena(h, &orbm_handle::motionArena, entries_per_job, last_runs); }

// this entry's own argument checks, behind the shared ones
static int orbq_motion_check_args(const void* h, const void* pool, const OrbqMotionJob* jobs, int n_jobs, float th, int min_matches, int check_ori)
{
    if (check_ori != 0 && check_ori != 1) return fail(ORBX_E_INVALID, "check_ori is 0 or 1");
    if (min_matches < 0) return fail(ORBX_E_INVALID, "negative min_matches");
    if (!std::isfinite(th) || !(th > 0.f)) return fail(ORBX_E_INVALID, "th must be finite and above 0");
    for (int j = 0; j < n_jobs; j++) {
        const OrbqMotionJob& J = jobs[j];
        if (J.nq < 0) return fail(ORBX_E_INVALID, "job %d: negative feature count", j);
        if (J.cur_slot < 0 || J.last_slot < 0) return fail(ORBX_E_INVALID, "job %d: negative slot", j);
        if (J.nq && !J.last_ids) return fail(ORBX_E_INVALID, "job %d: null array", j);
    }
    if (!h || !pool) return fail(ORBX_E_INVALID, "null handle or pool");
    return ORBX_OK;
}

extern "C" int orbq_track_motion_model(orbm_t* h, orbw_pool_t* pool, const OrbqMotionJob* jobs, int n_jobs, float th, int min_matches,
                                       int check_ori, const float* inv_level_sigma2, const float* scale_factors, int nlevels,
                                       OrbqMotionResult* out, int32_t* const* ids_out, uint8_t* const* outlier_out,
                                       int32_t* const* assign_out, uint8_t* const* status_out)
{
    if (n_jobs == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbq_check_shared(jobs, n_jobs, out, ids_out, outlier_out, inv_level_sigma2 && scale_factors, nlevels, "no level table", "null array");
    if (rc || (rc = orbq_motion_check_args(h, pool, jobs, n_jobs, th, min_matches, check_ori))) return rc;
    if ((rc = orbm_check(h)) || (rc = orbw_pool_check(pool))) return rc;
    if (pool->h->device != h->device) return fail(ORBX_E_INVALID, "the pool and the handle must share the device");
    const size_t nj = (size_t)n_jobs;
    size_t total = 0, totalQ = 0, sumCap = 0;
    int maxCap = 0, maxCell = 0, maxNq = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbqMotionJob& J = jobs[j];
        if ((rc = orbq_check_frameset(h, J.fs, j, J.cur_slot, J.last_slot, J.n, J.nq, sumCap))) return rc;
        total += (size_t)J.n; totalQ += (size_t)J.nq;
        maxCap = std::max(maxCap, J.fs->cap); maxCell = std::max(maxCell, J.fs->ncell); maxNq = std::max(maxNq, J.nq);
    }
    ProjPlan pl{};
    if ((rc = proj_lds_plan(maxCap, maxNq, maxCell, pl))) return rc;
    orbt::ProjCommon& c = pl.c;
    c.mode = 4; c.nnratio = 0.9f; c.checkOri = check_ori; c.thDist = 100;   // ORBmatcher.cc:1420 TH_HIGH; mode 4 has no ratio test
    proj_plan_queries(c, n_jobs);
    Packer pk;
    const size_t oJobs = pk.take(nj * sizeof(orbq::MotionJobDev)), oIdsIn = pk.take(totalQ * 4), upBytes = pk.off;
    // cleared to 0xff in one piece: both searches' tables (-1) | the status bytes (ORBQ_MM_ST_NOT_RUN).  What goes down starts at the
    // status bytes: status | outlier bytes | ids | the table that stands | the zero-cleared head
    const size_t oAssign = pk.take(2 * sumCap * 4), oStatus = pk.take(2 * sumCap), oFF = pk.off;
    const size_t oOutl = pk.take(total), oIds = pk.take(total * 4), oAsgOut = pk.take(total * 4);
    // cleared to 0 in one piece: results | state | need | the searches' candidate counters
    const size_t oOut = pk.take(nj * sizeof(OrbqMotionResult)), oState = pk.take(nj * 4), oNeed = pk.take(nj * 8), oTotal = pk.take(nj * 4), oZero = pk.off;
    const size_t downBytes = oZero - oStatus;
    const size_t oPw = pk.take(total * sizeof(float4)), oUv = pk.take(total * sizeof(float2)), oFlags = pk.take(total), oMerged = pk.take(total * 4);
    const size_t oTocc = pk.take(sumCap), oToccOut = pk.take(sumCap);
    const size_t oUvr = pk.take(sumCap * 12), oLvl = pk.take(sumCap * 2), oQv = pk.take(sumCap), oQo = pk.take(sumCap);
    const size_t oCandOff = pk.take(sumCap * 4), oCandCnt = pk.take(sumCap * 4), oQres = pk.take(sumCap * 4), oQscr = pk.take(sumCap * 12);
    const size_t oTscr = c.big ? pk.take(nj * (size_t)c.tCap * 12) : 0, oNm = pk.take(nj * 8), oPairs = pk.take(nj * sizeof(orbt::ProjPair)), work = pk.off;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    std::lock_guard<std::mutex> l(pool->mu);   // (held to the synchronise: no setter runs under the reads)
    for (int j = 0; j < n_jobs; j++)
        if ((rc = orbw_check_ids(pool, "last_ids", jobs[j].last_ids, jobs[j].nq, true))) return fail(rc, "job %d: %s", j, std::string(g_err).c_str());
    hipStream_t s = h->stream;
    for (int attempt = 0;; attempt++) {
        size_t arena;
        if ((rc = orbq_arena_reserve(h, h->motionArena, S_MOTION_ARENA, attempt, nj, std::max<size_t>(16 * (size_t)maxNq, 2048), arena))) return rc;
        uint8_t* hs = (uint8_t*)h->h_stage;
        uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
        orbq::MotionJobDev* hj = (orbq::MotionJobDev*)(hs + oJobs);
        size_t f0 = 0, q0 = 0, c0 = 0;
        for (int j = 0; j < n_jobs; j++) {
            const OrbqMotionJob& J = jobs[j];
            const orbm_frameset* fs = J.fs;
            const int64_t C = fs->cap;
            orbq::MotionJobDev& D = hj[j];
            memset(&D, 0, sizeof D);
            memcpy(D.V, J.velocity, sizeof D.V); memcpy(D.T, J.last_Tcw, sizeof D.T);
            memcpy(D.K, J.K, sizeof D.K);
            memcpy(D.bounds, fs->bounds, sizeof D.bounds);
            D.cur = orbt::train_side(fs->fs, J.cur_slot, fs->gd);
            D.lastKeys = fs->fs.keysUn + J.last_slot * C; D.nLast = fs->fs.n + J.last_slot;
            D.lastAng = fs->fs.ang + J.last_slot * C; D.lastDesc = fs->fs.desc + J.last_slot * C * 32;
            D.ids = (const int32_t*)(d + oIdsIn) + q0;
            D.n = J.n; D.nq = J.nq; D.f0 = (int32_t)f0; D.cap = fs->cap; D.c0 = (int32_t)c0;
            D.t0 = (int32_t)((size_t)j * c.tCap * 3);
            if (J.nq) memcpy(hs + oIdsIn + q0 * 4, J.last_ids, (size_t)J.nq * 4);
            f0 += (size_t)J.n; q0 += (size_t)J.nq; c0 += (size_t)C;
        }
        orbq::MotionArgs a{};
        orbq_fill_solver(a.q, pool, d, oPw, oUv, oFlags, oMerged, oIds, oOutl, inv_level_sigma2, nlevels);
        a.jobs = (const orbq::MotionJobDev*)(d + oJobs);
        a.out = (OrbqMotionResult*)(d + oOut);
        a.state = (int32_t*)(d + oState); a.need = (int32_t*)(d + oNeed); a.assignOut = (int32_t*)(d + oAsgOut);
        a.tocc = d + oTocc; a.toccOut = d + oToccOut; a.assign = (int32_t*)(d + oAssign);
        a.quvr = (float*)(d + oUvr); a.qlvl = (int8_t*)(d + oLvl); a.qvalid = d + oQv; a.qobs = d + oQo; a.status = d + oStatus;
        a.candOff = (int32_t*)(d + oCandOff); a.candCnt = (int32_t*)(d + oCandCnt); a.qres = (int32_t*)(d + oQres); a.qscr = (int32_t*)(d + oQscr);
        a.tscr = c.big ? (int32_t*)(d + oTscr) : nullptr; a.total = (int32_t*)(d + oTotal); a.nmatch = (int32_t*)(d + oNm);
        a.cand = slot_ptr<uint2>(h, S_MOTION_ARENA); a.candCap = (int32_t)arena;
        a.pairs = (orbt::ProjPair*)(d + oPairs);
        a.sumCap = (int32_t)sumCap; a.minMatches = min_matches; a.th = th;
        // (the octave's factor is read clamped to [0, 15], as the pool's projection reads it)
        for (int lv = 0; lv < ORBX_MAX_LEVELS; lv++) a.scale[lv] = lv < nlevels ? scale_factors[lv] : 0.f;
        HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(d + oAssign, 0xFF, oFF - oAssign, s));
        HIPCHK(hipMemsetAsync(d + oOutl, 0, oZero - oOutl, s));   // (the records' padding too: the same bytes every call)
        const dim3 gProj((unsigned)std::max(1, (maxNq + orbq::kMotionThreads - 1) / orbq::kMotionThreads), (unsigned)n_jobs);
        hipLaunchKernelGGL(orbq::k_motion_stage, dim3((unsigned)n_jobs), dim3(orbq::kLanes), 0, s, a, n_jobs, (int)orbq::MM_BEGIN);
        for (int pass = 0; pass < 2; pass++) {
            hipLaunchKernelGGL(orbq::k_motion_project, gProj, dim3(orbq::kMotionThreads), 0, s, a, pass);
            if ((rc = proj_launch(h, a.pairs, n_jobs, maxNq, pl, s))) {
                (void)hipStreamSynchronize(s);   // (the kernels in flight read the pool: they end before the mutex is let go)
                return rc;
            }
            hipLaunchKernelGGL(orbq::k_motion_stage, dim3((unsigned)n_jobs), dim3(orbq::kLanes), 0, s, a, n_jobs, (int)orbq::MM_MIDDLE + pass);
        }
        const size_t hOutl = oOutl - oStatus, hIds = oIds - oStatus, hAsg = oAsgOut - oStatus;
        const uint8_t* head = hs + (oOut - oStatus);   // (the zero-cleared head as it came down: results | state | need)
        if ((rc = orbq_drain("orbq_track_motion_model", pool, s, hs, d + oStatus, downBytes, head, sizeof(OrbqMotionResult), n_jobs, nlevels, ""))) return rc;
        bool again;
        if ((rc = orbq_arena_grow(h->motionArena, attempt, (const int32_t*)(head + (oNeed - oOut)), n_jobs, again))) return rc;
        if (again) continue;
        orbq_hand_back(jobs, n_jobs, out, head, sizeof(OrbqMotionResult), hs + hIds, hs + hOutl, ids_out, outlier_out);
        f0 = 0; c0 = 0;
        for (int j = 0; j < n_jobs; j++) {   // the tables asked for
            const size_t n = (size_t)jobs[j].n, nq = (size_t)jobs[j].nq;
            if (n && assign_out && assign_out[j]) memcpy(assign_out[j], hs + hAsg + f0 * 4, n * 4);
            if (nq && status_out && status_out[j]) memcpy(status_out[j], hs + 2 * c0, 2 * nq);
            f0 += n; c0 += (size_t)jobs[j].fs->cap;
        }
        return ORBX_OK;
    }
}
