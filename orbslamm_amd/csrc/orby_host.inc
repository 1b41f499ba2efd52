// orby_host.inc -- host side of LoopClosing::ComputeSim3's chain behind the Sim3Solver (part of orbslamm_hip.hip; kernels:
// orby_kernels.hip, ABI: include/orbslamm_computesim3.h, DESIGN.md §8v).  One call = the checks, one packed upload (job records |
// the entering match arrays | the two sigma tables), three launches for all jobs on the handle's stream (k_sim3_marks,
// k_sim3_search, k_compute_sim3), one copy down (results | findings | match tables | ids | removed bytes | and, where asked for, the
// status bytes and the vnMatch tables), one synchronise.  The pool's and the store's checks, the id and slot checkers, the reader
// mark: orbx_poolutil.inc.  The packed block is S_BLOCK: the call nests in none of its other users.

static_assert(sizeof(OrbyJob) == 336 && sizeof(OrbyResult) == 136, "orbslamm_computesim3.h layouts");
static_assert(sizeof(orby::JobDev) == 488, "the per-job upload size DESIGN.md §8v states");
static_assert(ORBW_FLAG_BAD == 1, "k_sim3_search and k_compute_sim3 read the bad bit");
static_assert(ORBY_ST_FOUND == orby::ST_FOUND && ORBY_ST_DEPTH == orby::ST_DEPTH && ORBY_ST_LEVEL_RANGE == orby::ST_LEVEL_RANGE, "ORBY_ST_*");

static inline bool orby_pos_finite(float v) { return v > 0.f && v <= FLT_MAX; }

// what needs neither a handle nor a GPU.  Zero jobs are settled by the caller before this
static int orby_check_args(const void* h, const void* pool, const void* store, const OrbyJob* jobs, int n_jobs, const float* sf1, const float* sf2,
                           const float* br1, const float* br2, const float* sig1, const float* sig2, int nlevels, const OrbyResult* out,
                           int32_t* const* match_out, int32_t* const* ids_out)
{
    if (n_jobs < 0) return fail(ORBX_E_INVALID, "negative job count");
    if (n_jobs > ORBZ_MAX_PROBLEMS) return fail(ORBX_E_UNSUPPORTED, "%d jobs: above %d", n_jobs, ORBZ_MAX_PROBLEMS);
    if (!jobs || !out || !match_out || !ids_out) return fail(ORBX_E_INVALID, "null argument");
    if (!sf1 || !sf2 || !br1 || !br2 || !sig1 || !sig2 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS)
        return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d] or a null level table", nlevels, ORBX_MAX_LEVELS);
    int rc;
    if ((rc = orbf_check_breaks(br1, nlevels)) || (rc = orbf_check_breaks(br2, nlevels))) return rc;
    int64_t total = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbyJob& J = jobs[j];
        if (!J.fs) return fail(ORBX_E_INVALID, "job %d: null frame set", j);
        if (J.n1 < 0 || J.n2 < 0) return fail(ORBX_E_INVALID, "job %d: negative feature count", j);
        if (J.n1 > ORBZ_MAX_CORR || J.n2 > ORBZ_MAX_CORR) return fail(ORBX_E_UNSUPPORTED, "job %d: %d or %d features: above %d", j, J.n1, J.n2, ORBZ_MAX_CORR);
        if (J.slot1 < 0 || J.slot2 < 0 || J.kf1 < 0 || J.kf2 < 0) return fail(ORBX_E_INVALID, "job %d: negative slot", j);
        if (!orby_pos_finite(J.prob.th2)) return fail(ORBX_E_INVALID, "job %d: th2 %g is not a finite positive number", j, (double)J.prob.th2);
        if (!orby_pos_finite(J.th)) return fail(ORBX_E_INVALID, "job %d: th %g is not a finite positive number", j, (double)J.th);
        if (!orby_pos_finite(J.s12)) return fail(ORBX_E_INVALID, "job %d: s12 %g is not a finite positive number", j, (double)J.s12);
        if ((J.m12_id == nullptr) != (J.m12_idx2 == nullptr)) return fail(ORBX_E_INVALID, "job %d: m12_id and m12_idx2 come together", j);
        if (J.n1 && (!match_out[j] || !ids_out[j])) return fail(ORBX_E_INVALID, "job %d: null output array", j);
        if (J.m12_idx2)
            for (int i = 0; i < J.n1; i++)
                if (J.m12_idx2[i] < -1 || J.m12_idx2[i] >= J.n2) return fail(ORBX_E_INVALID, "job %d: m12_idx2[%d] = %d outside [-1, %d)", j, i, J.m12_idx2[i], J.n2);
        total += (int64_t)J.n1 + J.n2;
        if (total > ORBZ_MAX_CALL_CORR) return fail(ORBX_E_UNSUPPORTED, "more than %d features in one call (reached at job %d)", ORBZ_MAX_CALL_CORR, j);
    }
    if (!h || !pool || !store) return fail(ORBX_E_INVALID, "null handle, pool or store");
    return ORBX_OK;
}

// ORBmatcher.cc:1121-1123 in the adapter's cvsem arithmetic (include/ORBmatcher_hip.hpp:791-793): sR12 = s12*R12 and sR21 =
// (1.0/s12)*R12.t() through convertTo with a double scale, t21 = -sR21*t12 as gemm's small branch (float sums) times -1.0
static void orby_sim3_pair(const OrbyJob& J, orby::JobDev& D)
{
    const double s = (double)J.s12, inv = 1.0 / J.s12;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            D.sR[0][3 * r + c] = (float)((double)J.R12[3 * c + r] * inv);
            D.sR[1][3 * r + c] = (float)((double)J.R12[3 * r + c] * s);
        }
    for (int r = 0; r < 3; r++) {
        const float* A = D.sR[0] + 3 * r;
        const float m = A[0] * J.t12[0] + A[1] * J.t12[1] + A[2] * J.t12[2];
        D.t[0][r] = (float)((double)m * -1.0);
        D.t[1][r] = J.t12[r];
    }
}

extern "C" int orby_compute_sim3(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const OrbyJob* jobs, int n_jobs,
                                 const float* scale_factors1, const float* scale_factors2, const float* level_breaks1, const float* level_breaks2,
                                 const float* inv_level_sigma2_1, const float* inv_level_sigma2_2, int nlevels, OrbyResult* out,
                                 int32_t* const* match_out, int32_t* const* ids_out, uint8_t* const* removed_out, uint8_t* const* status_out,
                                 int32_t* const* vnmatch_out)
{
    if (n_jobs == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orby_check_args(h, pool, store, jobs, n_jobs, scale_factors1, scale_factors2, level_breaks1, level_breaks2, inv_level_sigma2_1,
                             inv_level_sigma2_2, nlevels, out, match_out, ids_out);
    if (rc) return rc;
    if ((rc = orbm_check(h)) || (rc = orbw_pool_check(pool)) || (rc = orbu_store_check(store))) return rc;
    if (pool->h->device != h->device) return fail(ORBX_E_INVALID, "the pool and the handle must share the device");
    if (store->pool != pool) return fail(ORBX_E_INVALID, "the store stands beside another pool");
    size_t t1 = 0, t2 = 0;
    int max1 = 0, maxN = 0;
    bool debug = false;
    for (int j = 0; j < n_jobs; j++) {
        const OrbyJob& J = jobs[j];
        if ((rc = frameset_check(J.fs))) return rc;
        if (J.fs->owner != h) return fail(ORBX_E_INVALID, "job %d: the frame set belongs to another handle", j);
        if (J.slot1 >= J.fs->slots || J.slot2 >= J.fs->slots) return fail(ORBX_E_INVALID, "job %d: slot %d or %d outside the frame set", j, J.slot1, J.slot2);
        if (J.n1 > J.fs->cap || J.n2 > J.fs->cap) return fail(ORBX_E_INVALID, "job %d: %d or %d features for a frame of at most %d", j, J.n1, J.n2, J.fs->cap);
        if ((rc = orbu_check_slot(store, "kf1 of job", j, J.kf1, false)) || (rc = orbu_check_slot(store, "kf2 of job", j, J.kf2, false))) return rc;
        // (a set that builds on a stream of its own: the slots' builds may still run there)
        if (fs_stream(J.fs) != h->stream) HIPCHK(hipStreamSynchronize(fs_stream(J.fs)));
        t1 += (size_t)J.n1; t2 += (size_t)J.n2;
        max1 = std::max(max1, J.n1); maxN = std::max(maxN, std::max(J.n1, J.n2));
        debug |= (status_out && status_out[j]) || (vnmatch_out && vnmatch_out[j]);
    }
    const size_t t12 = t1 + t2;
    Packer pk;
    const size_t oJobs = pk.take((size_t)n_jobs * sizeof(orby::JobDev)), oId = pk.take(t1 * 4), oIdx = pk.take(t1 * 4),
                 oSigma = pk.take(2 * ORBX_MAX_LEVELS * sizeof(float)), upBytes = pk.off;
    const size_t oAlready = pk.take(t2), oMatch = pk.take(t1 * 4), oId2 = pk.take(t1 * 4), oCorrOf = pk.take(t1 * 4);
    const size_t oPw = pk.take(2 * t1 * sizeof(float4)), oUv = pk.take(2 * t1 * sizeof(float2)), oOff = pk.take(2 * t1);
    const size_t oOut = pk.take((size_t)n_jobs * sizeof(OrbyResult)), oBad = pk.take((size_t)n_jobs * 4), oMatchOut = pk.take(t1 * 4),
                 oIdsOut = pk.take(t1 * 4), oRemoved = pk.take(t1), plain = pk.off, oStatus = pk.take(t12), oVn = pk.take(t12 * 4), work = pk.off;
    const size_t downBytes = (debug ? work : plain) - oOut;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orby::JobDev* hj = (orby::JobDev*)(hs + oJobs);
    int32_t* hId = (int32_t*)(hs + oId);
    int32_t* hIdx = (int32_t*)(hs + oIdx);
    std::lock_guard<std::mutex> l(pool->mu);   // (held to the synchronise: no setter and no store update runs under the reads)
    size_t f1 = 0, f2 = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbyJob& J = jobs[j];
        if ((rc = orbu_check_slot(store, "kf1 of job", j, J.kf1, true)) || (rc = orbu_check_slot(store, "kf2 of job", j, J.kf2, true))) return rc;
        if (J.m12_id) {
            if ((rc = orbw_check_ids(pool, "m12_id", J.m12_id, J.n1, true))) return fail(rc, "job %d: %s", j, std::string(g_err).c_str());
            if (J.n1) { memcpy(hId + f1, J.m12_id, (size_t)J.n1 * 4); memcpy(hIdx + f1, J.m12_idx2, (size_t)J.n1 * 4); }
        } else if (J.n1) { memset(hId + f1, 0xFF, (size_t)J.n1 * 4); memset(hIdx + f1, 0xFF, (size_t)J.n1 * 4); }
        orby::JobDev& D = hj[j];
        memset(&D, 0, sizeof D);
        D.p = J.prob;
        const float deltaHuber = std::sqrt(J.prob.th2);   // Optimizer.cc:1398: the float square root of the float
        D.delta = (double)deltaHuber;
        const orbt::FrameSetDev& F = J.fs->fs;
        for (int k = 0; k < 2; k++) {
            const int slot = k ? J.slot2 : J.slot1;
            orby::SideDev& S = D.kf[k];
            S.keys = F.keysUn + (size_t)slot * F.cap; S.desc = F.desc + (size_t)slot * F.cap * 32;
            S.cellStart = F.cellStart + (size_t)slot * (F.ncell + 1); S.cellIdx = F.cellIdx + (size_t)slot * F.cap;
            S.nKeys = F.n + slot;
            S.entries = store->dev.entries + (size_t)(k ? J.kf2 : J.kf1) * store->pitch;
            memcpy(S.bounds, k ? J.bounds2 : J.bounds1, sizeof S.bounds);
            S.n = k ? J.n2 : J.n1;
        }
        D.grid = J.fs->gd;
        orby_sim3_pair(J, D);
        D.th = J.th;
        D.f1 = (int32_t)f1; D.f2 = (int32_t)f2; D.f12 = (int32_t)(f1 + f2);
        f1 += (size_t)J.n1; f2 += (size_t)J.n2;
    }
    float* hsig = (float*)(hs + oSigma);
    for (int lv = 0; lv < ORBX_MAX_LEVELS; lv++) {
        hsig[lv] = lv < nlevels ? inv_level_sigma2_1[lv] : 0.f;
        hsig[ORBX_MAX_LEVELS + lv] = lv < nlevels ? inv_level_sigma2_2[lv] : 0.f;
    }
    orby::Args a{};
    a.z.pw = (float4*)(d + oPw); a.z.uv = (float2*)(d + oUv); a.z.off = d + oOff; a.z.removed = d + oRemoved;
    a.z.invSigma2 = (const float*)(d + oSigma); a.z.nlevels = nlevels;
    a.jobs = (const orby::JobDev*)(d + oJobs);
    a.pool = pool->dev;
    a.m12Id = (const int32_t*)(d + oId); a.m12Idx2 = (const int32_t*)(d + oIdx);
    a.already2 = d + oAlready;
    a.vn = (int32_t*)(d + oVn); a.status = d + oStatus;
    a.match = (int32_t*)(d + oMatch); a.id2 = (int32_t*)(d + oId2); a.corrOf = (int32_t*)(d + oCorrOf);
    a.matchOut = (int32_t*)(d + oMatchOut); a.idsOut = (int32_t*)(d + oIdsOut);
    a.out = (OrbyResult*)(d + oOut); a.bad = (int32_t*)(d + oBad);
    orbf_fill_tables(scale_factors1, level_breaks1, nlevels, a.sf[0], a.breaks[0]);
    orbf_fill_tables(scale_factors2, level_breaks2, nlevels, a.sf[1], a.breaks[1]);
    a.stride = store->stride;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    if (t2) HIPCHK(hipMemsetAsync(d + oAlready, 0, t2, s));
    HIPCHK(hipMemsetAsync(d + oOut, 0, oMatchOut - oOut, s));   // the records (their padding too: the same bytes every call) and the findings
    if (t1) HIPCHK(hipMemsetAsync(d + oRemoved, 0, t1, s));     // (behind a job's n_corr the removed bytes are zero)
    if (max1) hipLaunchKernelGGL(orby::k_sim3_marks, dim3((unsigned)((max1 + 255) / 256), (unsigned)n_jobs), dim3(256), 0, s, a);
    if (maxN) hipLaunchKernelGGL(orby::k_sim3_search, dim3((unsigned)((maxN + orby::kLanes - 1) / orby::kLanes), 2u, (unsigned)n_jobs), dim3(orby::kLanes), 0, s, a);
    hipLaunchKernelGGL(orby::k_compute_sim3, dim3((unsigned)n_jobs), dim3(orby::kLanes), 0, s, a, n_jobs);
    HIPCHK(hipGetLastError());
    if ((rc = orbw_mark_reader(pool, s))) return rc;
    HIPCHK(hipMemcpyAsync(hs, d + oOut, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int32_t* hbad = (const int32_t*)(hs + (oBad - oOut));
    for (int j = 0; j < n_jobs; j++)
        if (hbad[j])
            return fail(ORBX_E_INVALID, "job %d: an edge's octave lies outside [0, %d), a matched feature lies at or above its slot's device count, or a pass matched a feature at or above the job's n",
                        j, nlevels);
    memcpy(out, hs, (size_t)n_jobs * sizeof(OrbyResult));
    f1 = 0; f2 = 0;
    for (int j = 0; j < n_jobs; j++) {
        const size_t n1 = (size_t)jobs[j].n1, n12 = n1 + (size_t)jobs[j].n2;
        if (n1) {
            memcpy(match_out[j], hs + (oMatchOut - oOut) + f1 * 4, n1 * 4);
            memcpy(ids_out[j], hs + (oIdsOut - oOut) + f1 * 4, n1 * 4);
            if (removed_out && removed_out[j]) memcpy(removed_out[j], hs + (oRemoved - oOut) + f1, n1);
        }
        if (n12 && status_out && status_out[j]) memcpy(status_out[j], hs + (oStatus - oOut) + f1 + f2, n12);
        if (n12 && vnmatch_out && vnmatch_out[j]) memcpy(vnmatch_out[j], hs + (oVn - oOut) + (f1 + f2) * 4, n12 * 4);
        f1 += n1; f2 += (size_t)jobs[j].n2;
    }
    return ORBX_OK;
}
