// orbq_host.inc -- host side of PoseOptimization fed from the map-point pool (part of orbslamm_hip.hip; kernel:
// orbq_kernels.hip, ABI: include/orbslamm_trackpose.h, DESIGN.md §8s).  One call = the checks, one packed upload (job records |
// the frames' ids before the search), ONE launch for all jobs on the handle's stream, one copy down (results | ids | outlier
// bytes), one synchronise.  The searches' tables and ids are read where the searches left them: nothing per match goes up.
// The pool's and the store's checks, the id and slot checkers, the reader mark: orbx_poolutil.inc.  What this entry shares with
// orbq_track_reference (below), orbq_relocalize and orbq_track_motion_model: orbq_scaffold.inc.

static_assert(sizeof(OrbqJob) == 112 && sizeof(OrbqResult) == 184, "orbslamm_trackpose.h layouts");
static_assert(ORBW_FLAG_OBSERVED == 2, "k_track_pose reads the observed bit");
static_assert(sizeof(orbq::JobDev) == 136 && sizeof(orbo::FrameIn) == 104, "the per-frame upload sizes tools/trackpose_bench.py computes with");

// this entry's own argument checks, behind the shared ones
static int orbq_check_args(const OrbqJob* jobs, int n_jobs)
{
    for (int j = 0; j < n_jobs; j++) {
        const OrbqJob& J = jobs[j];
        if (J.back < -1 || J.back >= ResultRing::kSets) return fail(ORBX_E_INVALID, "job %d: back %d outside [-1, %d]", j, J.back, ResultRing::kSets - 1);
        if (J.discard != 0 && J.discard != 1) return fail(ORBX_E_INVALID, "job %d: discard is 0 or 1", j);
    }
    return ORBX_OK;
}

// (the pool's mutex is held) job j's search can still be read: its record, then where its table and its ids lie
static int orbq_job_source(orbw_pool* pool, const OrbqJob& J, int j, orbq::JobDev& D)
{
    orbm_frameset* fs = J.fs;
    D.assign = nullptr; D.ids = nullptr; D.nq = 0;
    if (J.back < 0) return ORBX_OK;
    const int set = fs->res.back(J.back);
    const ResultRecord& r = fs->res.rec[set];
    if (!r.ev || r.kind != ResultRecord::kQueries || !r.fromPool) return fail(ORBX_E_INVALID, "job %d: that search was not issued from a map-point pool", j);
    if (r.slot != J.slot) return fail(ORBX_E_INVALID, "job %d: that search ran against slot %d, not %d", j, r.slot, J.slot);
    if (r.pool != pool || r.poolSerial != pool->serial) return fail(ORBX_E_INVALID, "job %d: that search was issued from another pool", j);
    if (!r.accepted) return fail(ORBX_E_INVALID, "job %d: that search has not been received through orbm_track_results", j);
    if (r.qEpoch != fs->qEpoch) return fail(ORBX_E_CAPACITY, "job %d: a larger query search issued behind it reallocated the search's staging", j);
    if (fs->slotBuilt[(size_t)J.slot] > r.builds) return fail(ORBX_E_CAPACITY, "job %d: slot %d has been rebuilt since the search was issued", j, J.slot);
    if (r.store) {
        const orbu_store* s = (const orbu_store*)r.store;
        if (!live_has(s) || s->serial != r.storeSerial) return fail(ORBX_E_CAPACITY, "job %d: the keyframe store whose list the search read was destroyed", j);
        if (s->updates != r.storeUpdates) return fail(ORBX_E_CAPACITY, "job %d: the keyframe store completed another update since the search was issued", j);
        D.ids = s->out.S;
    } else
        D.ids = (const int32_t*)(fs->h_q + (size_t)set * fs->qBytes + r.oIds);
    D.assign = set_tables(fs, set).assign;
    D.nq = r.nq;
    return ORBX_OK;
}

extern "C" int orbq_track_pose(orbm_t* h, orbw_pool_t* pool, const OrbqJob* jobs, int n_jobs, const float* inv_level_sigma2, int nlevels,
                               OrbqResult* out, int32_t* const* ids_out, uint8_t* const* outlier_out)
{
    if (n_jobs == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbq_check_shared(jobs, n_jobs, out, ids_out, outlier_out, inv_level_sigma2 != nullptr, nlevels, "no sigma table", "null output array");
    if (rc || (rc = orbq_check_args(jobs, n_jobs))) return rc;
    if ((rc = orbm_check(h)) || (rc = orbw_pool_check(pool))) return rc;
    if (pool->h->device != h->device) return fail(ORBX_E_INVALID, "the pool and the handle must share the device");
    size_t total = 0, nBase = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbqJob& J = jobs[j];
        // (this entry's own text, not orbq_check_frameset, and its own tail below: with the shared ones the many-job rows of
        // tools/trackpose_bench.py left the parent's band, docs/experiments.md)
        if ((rc = frameset_check(J.fs))) return rc;
        if (J.fs->owner != h) return fail(ORBX_E_INVALID, "job %d: the frame set belongs to another handle", j);
        if (J.slot < 0 || J.slot >= J.fs->slots) return fail(ORBX_E_INVALID, "job %d: slot %d outside the frame set", j, J.slot);
        if (J.n > J.fs->cap) return fail(ORBX_E_INVALID, "job %d: %d features for a frame of at most %d", j, J.n, J.fs->cap);
        // no search to stand behind: the slot's build may still run on the set's own stream
        if (J.back < 0 && fs_stream(J.fs) != h->stream) HIPCHK(hipStreamSynchronize(fs_stream(J.fs)));
        total += (size_t)J.n;
        if (J.base_ids) nBase += (size_t)J.n;
    }
    Packer pk;
    const size_t oJobs = pk.take((size_t)n_jobs * sizeof(orbq::JobDev)), oBase = pk.take(nBase * 4), upBytes = pk.off;
    const size_t oPw = pk.take(total * sizeof(float4)), oUv = pk.take(total * sizeof(float2)), oFlags = pk.take(total), oMerged = pk.take(total * 4);
    const size_t oOut = pk.take((size_t)n_jobs * sizeof(OrbqResult)), oIds = pk.take(total * 4), oOutl = pk.take(total), work = pk.off;
    const size_t downBytes = work - oOut;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orbq::JobDev* hj = (orbq::JobDev*)(hs + oJobs);
    std::lock_guard<std::mutex> l(pool->mu);   // (held to the synchronise: no setter and no store update runs under the gather)
    size_t f0 = 0, b0 = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbqJob& J = jobs[j];
        orbq::JobDev& D = hj[j];
        if ((rc = orbq_job_source(pool, J, j, D))) return rc;
        if (J.base_ids) {
            if ((rc = orbw_check_ids(pool, "base_ids", J.base_ids, J.n, true))) return fail(rc, "job %d: %s", j, g_err.c_str());
            if (J.n) memcpy(hs + oBase + b0 * 4, J.base_ids, (size_t)J.n * 4);
        }
        memcpy(D.Tcw, J.frame.Tcw, sizeof D.Tcw);
        memcpy(D.K, J.frame.K, sizeof D.K);
        D.keys = J.fs->fs.keysUn + (size_t)J.slot * J.fs->cap;
        D.nKeys = J.fs->fs.n + J.slot;
        D.base = J.base_ids ? (const int32_t*)(d + oBase) + b0 : nullptr;
        D.n = J.n; D.f0 = (int32_t)f0; D.discard = J.discard;
        f0 += (size_t)J.n;
        if (J.base_ids) b0 += (size_t)J.n;
    }
    orbq::Args a{};
    orbq_fill_solver(a, pool, d, oPw, oUv, oFlags, oMerged, oIds, oOutl, inv_level_sigma2, nlevels);
    a.jobs = (const orbq::JobDev*)(d + oJobs);
    a.out = (OrbqResult*)(d + oOut);
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d + oOut, 0, (size_t)n_jobs * sizeof(OrbqResult), s));   // (the records' padding word too: the same bytes every call)
    hipLaunchKernelGGL(orbq::k_track_pose, dim3((unsigned)n_jobs), dim3(orbq::kLanes), 0, s, a, n_jobs);
    // (an error from here on: the kernel in flight reads the pool, so the stream is drained before the mutex is let go)
    HIPCHK_OR(hipGetLastError(), (void)hipStreamSynchronize(s));
    if ((rc = orbw_mark_reader(pool, s))) { (void)hipStreamSynchronize(s); return rc; }
    HIPCHK_OR(hipMemcpyAsync(hs, d + oOut, downBytes, hipMemcpyDeviceToHost, s), (void)hipStreamSynchronize(s));
    HIPCHK(hipStreamSynchronize(s));
    const OrbqResult* hr = (const OrbqResult*)hs;
    for (int j = 0; j < n_jobs; j++)
        if (hr[j].opt.rounds < 0)
            return fail(ORBX_E_INVALID, "job %d: an edge's octave lies outside [0, %d), or a feature at or above the slot's device count (or a match without a point of the pool) holds a point",
                        j, nlevels);
    memcpy(out, hr, (size_t)n_jobs * sizeof(OrbqResult));
    f0 = 0;
    for (int j = 0; j < n_jobs; j++) {
        const size_t n = (size_t)jobs[j].n;
        if (n) { memcpy(ids_out[j], hs + (oIds - oOut) + f0 * 4, n * 4); memcpy(outlier_out[j], hs + (oOutl - oOut) + f0, n); }
        f0 += n;
    }
    return ORBX_OK;
}

// ------------------------------------------------------------------ Tracking::TrackReferenceKeyFrame (DESIGN.md §8t)
// One call = the checks, one packed upload (the job records), per run of jobs on one frame set the set search with the validity
// block (k_ref_valid, k_bow_set, k_bow_prune_set into device memory), ONE k_track_reference launch for all jobs, one copy down
// (results | ids | outlier bytes | the match tables asked for), one synchronise.

static_assert(sizeof(OrbqRefJob) == 112 && sizeof(OrbqRefResult) == 192, "orbslamm_trackpose.h layouts");
static_assert(offsetof(OrbqRefResult, track) == 0 && offsetof(OrbqResult, opt) == 0, "orbq_drain reads rounds from the OrboResult at a record's head");
static_assert(ORBW_FLAG_BAD == 1, "k_ref_valid reads the bad bit");
static_assert(sizeof(orbq::RefJobDev) == 152, "the per-job upload size tools/trackref_bench.py computes with");

// this entry's own argument checks, behind the shared ones
static int orbq_ref_check_args(const void* h, const void* pool, const void* store, const OrbqRefJob* jobs, int n_jobs, int min_matches)
{
    if (min_matches < 0) return fail(ORBX_E_INVALID, "min_matches %d is negative", min_matches);
    for (int j = 0; j < n_jobs; j++) {
        const OrbqRefJob& J = jobs[j];
        if (J.solve != 0 && J.solve != 1) return fail(ORBX_E_INVALID, "job %d: solve is 0 or 1", j);
        if (J.kf_slot < 0 || J.slot < 0 || J.kf < 0) return fail(ORBX_E_INVALID, "job %d: negative slot", j);
    }
    if (!h || !pool || !store) return fail(ORBX_E_INVALID, "null handle, pool or store");
    return ORBX_OK;
}

extern "C" int orbq_track_reference(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const OrbqRefJob* jobs, int n_jobs,
                                    float nnratio, int check_ori, int min_matches, const float* inv_level_sigma2, int nlevels,
                                    OrbqRefResult* out, int32_t* const* ids_out, uint8_t* const* outlier_out, int32_t* const* match_out)
{
    if (n_jobs == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbq_check_shared(jobs, n_jobs, out, ids_out, outlier_out, inv_level_sigma2 != nullptr, nlevels, "no sigma table", "null output array");
    if (rc || (rc = orbq_ref_check_args(h, pool, store, jobs, n_jobs, min_matches))) return rc;
    if ((rc = orbm_check(h)) || (rc = orbw_pool_check(pool)) || (rc = orbu_store_check(store))) return rc;
    if (pool->h->device != h->device) return fail(ORBX_E_INVALID, "the pool and the handle must share the device");
    if (store->pool != pool) return fail(ORBX_E_INVALID, "the store stands beside another pool");
    size_t total = 0, sumCap = 0, nAsked = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbqRefJob& J = jobs[j];
        if ((rc = orbq_check_frameset(h, J.fs, j, J.kf_slot, J.slot, J.n, /* no second count */ -1, sumCap))) return rc;
        if (!J.fs->bow || !J.fs->bow->computed) return fail(ORBX_E_INVALID, "job %d: orbm_frameset_compute_bow has not run", j);
        if ((rc = orbu_check_slot(store, "kf of job", j, J.kf, false))) return rc;   // (kfcap never changes; the set byte: under the mutex, below)
        total += (size_t)J.n;
        if (match_out && match_out[j]) nAsked += (size_t)J.n;
    }
    Packer pk;
    const size_t oJobs = pk.take((size_t)n_jobs * sizeof(orbq::RefJobDev)), upBytes = pk.off;
    const size_t oMatched = pk.take(sumCap), oValid = pk.take(sumCap), oBin = pk.take(sumCap), oRaw = pk.take(sumCap * 4), oTable = pk.take(sumCap * 4),
                 oNBow = pk.take((size_t)n_jobs * 4);
    const size_t oPw = pk.take(total * sizeof(float4)), oUv = pk.take(total * sizeof(float2)), oFlags = pk.take(total), oMerged = pk.take(total * 4);
    const size_t oOut = pk.take((size_t)n_jobs * sizeof(OrbqRefResult)), oIds = pk.take(total * 4), oOutl = pk.take(total), oMatch = pk.take(nAsked * 4), work = pk.off;
    const size_t downBytes = work - oOut;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orbq::RefJobDev* hj = (orbq::RefJobDev*)(hs + oJobs);
    std::lock_guard<std::mutex> l(pool->mu);   // (held to the synchronise: no setter and no store update runs under the reads)
    size_t f0 = 0, c0 = 0, m0 = 0;
    int maxCap = 0;
    for (int j = 0; j < n_jobs; j++) {
        const OrbqRefJob& J = jobs[j];
        if ((rc = orbu_check_slot(store, "kf of job", j, J.kf, true))) return rc;
        orbq::RefJobDev& D = hj[j];
        memset(&D, 0, sizeof D);
        memcpy(D.Tcw, J.frame.Tcw, sizeof D.Tcw);
        memcpy(D.K, J.frame.K, sizeof D.K);
        D.keys = J.fs->fs.keysUn + (size_t)J.slot * J.fs->cap;
        D.nKeys = J.fs->fs.n + J.slot;
        D.entries = store->dev.entries + (size_t)J.kf * store->pitch;
        D.valid = d + oValid + c0;
        D.table = (const int32_t*)(d + oTable) + c0;
        D.nBow = (const int32_t*)(d + oNBow) + j;
        D.n = J.n; D.f0 = (int32_t)f0; D.solve = J.solve; D.cap = J.fs->cap;
        const bool asked = match_out && match_out[j];
        D.matchAt = asked ? (int32_t)m0 : -1;
        f0 += (size_t)J.n; c0 += (size_t)J.fs->cap;
        if (asked) m0 += (size_t)J.n;
        maxCap = std::max(maxCap, J.fs->cap);
    }
    orbq::RefArgs a{};
    orbq_fill_solver(a.q, pool, d, oPw, oUv, oFlags, oMerged, oIds, oOutl, inv_level_sigma2, nlevels);
    a.jobs = (const orbq::RefJobDev*)(d + oJobs);
    a.out = (OrbqRefResult*)(d + oOut);
    a.matchOut = (int32_t*)(d + oMatch);
    a.stride = store->stride; a.minMatches = min_matches;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d + oMatched, 0, sumCap, s));
    HIPCHK(hipMemsetAsync(d + oRaw, 0xFF, oNBow - oRaw, s));   // the raw and the pruned tables: -1
    HIPCHK(hipMemsetAsync(d + oOut, 0, (size_t)n_jobs * sizeof(OrbqRefResult), s));   // (the records' padding too: the same bytes every call)
    hipLaunchKernelGGL(orbq::k_ref_valid, dim3((unsigned)((maxCap + 255) / 256), (unsigned)n_jobs), dim3(256), 0, s, a.jobs, pool->dev, store->stride);
    // the set search of orbm_bow_frames, per run of consecutive jobs on one frame set, in batches of kBowMaxPairs
    c0 = 0;
    for (int j0 = 0; j0 < n_jobs;) {
        orbm_frameset* fs = jobs[j0].fs;
        int nb = 1;
        while (j0 + nb < n_jobs && nb < orbm::kBowMaxPairs && jobs[j0 + nb].fs == fs) nb++;
        const orbm_frameset_bow* b = fs->bow;
        orbm::BowSetArgs ba{};
        ba.desc = fs->fs.desc; ba.ang = fs->fs.ang; ba.n = fs->fs.n; ba.cap = fs->cap;
        ba.fvNode = b->d_fvNode; ba.fvStart = b->d_fvStart; ba.fvIdx = b->d_fvIdx; ba.counts = b->d_counts;
        ba.matched = d + oMatched + c0; ba.match = (int32_t*)(d + oRaw) + c0; ba.binOf = d + oBin + c0; ba.qvalid = d + oValid + c0;
        ba.nnratio = nnratio; ba.thLow = 50; ba.checkOri = check_ori;
        for (int i = 0; i < nb; i++) { ba.kf[i] = (int16_t)jobs[j0 + i].kf_slot; ba.fr[i] = (int16_t)jobs[j0 + i].slot; }
        hipLaunchKernelGGL(orbm::k_bow_set, dim3((unsigned)std::max(b->maxNodes, 1), (unsigned)nb), dim3(64), 0, s, ba);
        hipLaunchKernelGGL(orbm::k_bow_prune_set, dim3((unsigned)nb), dim3(256), 0, s, ba, (int32_t*)(d + oTable) + c0, (int32_t*)(d + oNBow) + j0);
        c0 += (size_t)nb * fs->cap;
        j0 += nb;
    }
    hipLaunchKernelGGL(orbq::k_track_reference, dim3((unsigned)n_jobs), dim3(orbq::kLanes), 0, s, a, n_jobs);
    if ((rc = orbq_drain("orbq_track_reference", pool, s, hs, d + oOut, downBytes, hs, sizeof(OrbqRefResult), n_jobs, nlevels, " (or a match without a point of the pool)"))) return rc;
    orbq_hand_back(jobs, n_jobs, out, hs, sizeof(OrbqRefResult), hs + (oIds - oOut), hs + (oOutl - oOut), ids_out, outlier_out);
    m0 = 0;
    for (int j = 0; j < n_jobs; j++) {   // the match tables asked for
        const size_t n = (size_t)jobs[j].n;
        if (!match_out || !match_out[j]) continue;
        if (n) memcpy(match_out[j], hs + (oMatch - oOut) + m0 * 4, n * 4);
        m0 += n;
    }
    return ORBX_OK;
}
