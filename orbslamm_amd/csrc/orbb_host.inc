// orbb_host.inc -- host side of the device initial map (part of orbslamm_hip.hip; kernel: orbb_kernels.hip, ABI:
// include/orbslamm_initmap.h, DESIGN.md §8aa).  One call = the checks, one packed upload (problem records | matches | positions |
// with host arrays both frames' keys), ONE launch for all problems, one copy of the results and the point records down, one
// synchronise.  The points' scratch (kSlotWords binary64 words a feature of the initial frames, and the compaction's words) is
// part of the same packed block, which grows only.

static_assert(sizeof(OrbbProblem) == 136 && sizeof(OrbbResult) == 224 && sizeof(OrbbPoint) == 48, "orbslamm_initmap.h layouts");
static_assert(orbb::kMaxFeatures == ORBB_MAX_FEATURES && orbb::kMaxProblems == ORBB_MAX_PROBLEMS && orbb::kMaxCallFeatures == ORBB_MAX_CALL_FEATURES &&
              orbg::kBaIterations == ORBB_MAX_ITERATIONS, "orbb limits");
static_assert(ORBB_OK == 0 && ORBB_RESET_DEPTH == 1 && ORBB_RESET_TRACKED == 2 && ORBB_RESET_NONFINITE == 3, "the kernel's verdicts");
static_assert(ORBB_STOP_ITERATIONS == orbg::kStopIterations && ORBB_STOP_TRIALS == orbg::kStopTrials && ORBB_STOP_RHO_ZERO == orbg::kStopRhoZero &&
              ORBB_STOP_FLAT == orbg::kStopFlat && ORBR_ST_DONE == 1, "the kernel's stop reasons and status");

static bool orbb_finite(const float* v, int n) { for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

// what needs neither the handle nor a GPU; feat0[p]: the problem's first feature among the call's.  Zero problems are settled by the
// callers before this
static int orbb_check_args(const OrbbProblem* problems, int n_problems, const int32_t* const* matches12, const float* const* P3D,
                           const float* inv_level_sigma2, const float* scale_factors, int nlevels, const OrbbResult* out, OrbbPoint* const* points,
                           std::vector<int32_t>& feat0)
{
    if (n_problems < 0) return fail(ORBX_E_INVALID, "negative problem count");
    if (n_problems > ORBB_MAX_PROBLEMS) return fail(ORBX_E_UNSUPPORTED, "%d problems: above %d", n_problems, ORBB_MAX_PROBLEMS);
    if (!inv_level_sigma2 || !scale_factors || nlevels < 1 || nlevels > ORBX_MAX_LEVELS)
        return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d] or no level table", nlevels, ORBX_MAX_LEVELS);
    if (!orbb_finite(inv_level_sigma2, nlevels) || !orbb_finite(scale_factors, nlevels)) return fail(ORBX_E_INVALID, "a level table entry is not finite");
    if (!problems || !matches12 || !P3D || !out || !points) return fail(ORBX_E_INVALID, "null argument");
    std::vector<uint8_t> seen;
    try { feat0.assign((size_t)n_problems + 1, 0); }
    catch (const std::bad_alloc&) { return fail(ORBX_E_CAPACITY, "no host memory for %d problems", n_problems); }
    for (int p = 0; p < n_problems; p++) {
        const OrbbProblem& pr = problems[p];
        if (pr.n1 < 0 || pr.n2 < 0) return fail(ORBX_E_INVALID, "problem %d: negative feature count", p);
        if (pr.n1 > ORBB_MAX_FEATURES || pr.n2 > ORBB_MAX_FEATURES)
            return fail(ORBX_E_UNSUPPORTED, "problem %d: %d features in a frame: above %d", p, std::max(pr.n1, pr.n2), ORBB_MAX_FEATURES);
        if ((int64_t)feat0[(size_t)p] + pr.n1 > ORBB_MAX_CALL_FEATURES)
            return fail(ORBX_E_UNSUPPORTED, "more than %d features of initial frames in one call (reached at problem %d)", ORBB_MAX_CALL_FEATURES, p);
        feat0[(size_t)p + 1] = feat0[(size_t)p] + pr.n1;
        if (pr.iterations < 0 || pr.iterations > ORBB_MAX_ITERATIONS)
            return fail(ORBX_E_INVALID, "problem %d: iterations %d outside [0, %d]", p, pr.iterations, ORBB_MAX_ITERATIONS);
        if (pr.fixed_first && pr.fixed_second) return fail(ORBX_E_INVALID, "problem %d: both poses fixed", p);
        if (!orbb_finite(pr.Tcw1, 12) || !orbb_finite(pr.Tcw2, 12) || !orbb_finite(pr.K, 4)) return fail(ORBX_E_INVALID, "problem %d: a pose or camera entry is not finite", p);
        if (pr.n1 && (!matches12[p] || !P3D[p] || !points[p])) return fail(ORBX_E_INVALID, "problem %d: null argument", p);
        try { seen.assign((size_t)pr.n2, 0); }
        catch (const std::bad_alloc&) { return fail(ORBX_E_CAPACITY, "no host memory for %d features", pr.n2); }
        for (int i = 0; i < pr.n1; i++) {
            const int m = matches12[p][i];
            if (m < 0) continue;   // (-1 in the reference; any negative is no match)
            if (m >= pr.n2) return fail(ORBX_E_INVALID, "problem %d: feature %d is matched to %d, outside the second frame's [0, %d)", p, i, m, pr.n2);
            if (seen[(size_t)m]) return fail(ORBX_E_INVALID, "problem %d: feature %d of the second frame is matched twice (again by feature %d)", p, m, i);
            seen[(size_t)m] = 1;
            if (!orbb_finite(P3D[p] + 3 * (size_t)i, 3)) return fail(ORBX_E_INVALID, "problem %d: the position of feature %d is not finite", p, i);
        }
    }
    return ORBX_OK;
}

// resident1 / resident2: the frames' device keys, or null: keys1 / keys2 hold them on the host
static int orbb_core(orbm_handle* h, const OrbbProblem* problems, int n_problems, const OrbxKeyPoint* const* keys1, const OrbxKeyPoint* const* keys2,
                     orbm_frame* const* resident1, orbm_frame* const* resident2, const int32_t* const* matches12, const float* const* P3D,
                     const float* inv_level_sigma2, const float* scale_factors, int nlevels, OrbbResult* out, OrbbPoint* const* points,
                     const std::vector<int32_t>& feat0)
{
    int rc;
    const size_t total = (size_t)feat0[(size_t)n_problems], slots = std::max<size_t>(total, 1);
    std::vector<size_t> k1off((size_t)n_problems, 0), k2off((size_t)n_problems, 0);
    Packer pk;
    const size_t oProbs = pk.take((size_t)n_problems * sizeof(orbb::ProbIn)), oMatch = pk.take(total * sizeof(int32_t)), oP3d = pk.take(total * 3 * sizeof(float));
    if (!resident1)
        for (int p = 0; p < n_problems; p++) {
            k1off[(size_t)p] = pk.take((size_t)problems[p].n1 * sizeof(OrbxKeyPoint));
            k2off[(size_t)p] = pk.take((size_t)problems[p].n2 * sizeof(OrbxKeyPoint));
        }
    const size_t upBytes = pk.off;
    const size_t oScr = pk.take(slots * orbb::kSlotWords * sizeof(double)), oOb = pk.take(2 * slots * sizeof(float4)), oFeat = pk.take(slots * sizeof(int32_t)),
                 oLvl = pk.take(slots * sizeof(int32_t)), oDepth = pk.take(slots * sizeof(float));
    const size_t oOut = pk.take((size_t)n_problems * sizeof(OrbbResult)), oPts = pk.take(total * sizeof(OrbbPoint)), work = pk.off;
    const size_t downBytes = work - oOut;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orbb::ProbIn* hp = (orbb::ProbIn*)(hs + oProbs);
    for (int p = 0; p < n_problems; p++) {
        const OrbbProblem& pr = problems[p];
        memcpy(hp[p].Tcw[0], pr.Tcw1, sizeof pr.Tcw1);
        memcpy(hp[p].Tcw[1], pr.Tcw2, sizeof pr.Tcw2);
        memcpy(hp[p].K, pr.K, sizeof pr.K);
        hp[p].fixed0 = pr.fixed_first; hp[p].fixed1 = pr.fixed_second; hp[p].iterations = pr.iterations; hp[p].robust = pr.robust;
        hp[p].n1 = pr.n1; hp[p].n2 = pr.n2;
        hp[p].keys1 = resident1 ? resident1[p]->d_keysUn : (const orbm::KeyDev*)(d + k1off[(size_t)p]);
        hp[p].keys2 = resident2 ? resident2[p]->d_keysUn : (const orbm::KeyDev*)(d + k2off[(size_t)p]);
        hp[p].off = feat0[(size_t)p]; hp[p].pad = 0;
        if (pr.n1) {
            memcpy(hs + oMatch + (size_t)feat0[(size_t)p] * sizeof(int32_t), matches12[p], (size_t)pr.n1 * sizeof(int32_t));
            memcpy(hs + oP3d + (size_t)feat0[(size_t)p] * 3 * sizeof(float), P3D[p], (size_t)pr.n1 * 3 * sizeof(float));
        }
        if (!resident1) {
            if (pr.n1) memcpy(hs + k1off[(size_t)p], keys1[p], (size_t)pr.n1 * sizeof(OrbxKeyPoint));
            if (pr.n2) memcpy(hs + k2off[(size_t)p], keys2[p], (size_t)pr.n2 * sizeof(OrbxKeyPoint));
        }
    }
    orbb::Args a{};
    a.probs = (const orbb::ProbIn*)(d + oProbs); a.matches = (const int32_t*)(d + oMatch); a.p3d = (const float*)(d + oP3d);
    a.out = (OrbbResult*)(d + oOut); a.pts = (OrbbPoint*)(d + oPts); a.scr = (double*)(d + oScr); a.ob = (float4*)(d + oOb);
    a.feat = (int32_t*)(d + oFeat); a.lvl = (int32_t*)(d + oLvl); a.depth = (float*)(d + oDepth);
    a.total = (int32_t)slots; a.nlevels = nlevels;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) { a.invSigma2[l] = l < nlevels ? inv_level_sigma2[l] : 0.f; a.sf[l] = l < nlevels ? scale_factors[l] : 1.f; }
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d + oOut, 0, downBytes, s));   // (the records' padding and the unmatched features' records: the same bytes every call)
    hipLaunchKernelGGL(orbb::k_initial_map, dim3((unsigned)n_problems), dim3(orbb::kLanes), 0, s, a, n_problems);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oOut, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const OrbbResult* hr = (const OrbbResult*)hs;
    for (int p = 0; p < n_problems; p++)
        if (hr[p].verdict < 0) return fail(ORBX_E_INVALID, "problem %d: a matched key's octave lies outside [0, %d) or its position is not finite", p, nlevels);
    memcpy(out, hr, (size_t)n_problems * sizeof(OrbbResult));
    const OrbbPoint* hpts = (const OrbbPoint*)(hs + (oPts - oOut));
    for (int p = 0; p < n_problems; p++)
        if (problems[p].n1) memcpy(points[p], hpts + feat0[(size_t)p], (size_t)problems[p].n1 * sizeof(OrbbPoint));
    return ORBX_OK;
}

extern "C" int orbb_initial_map(orbm_t* h, const OrbbProblem* problems, int n_problems, const OrbxKeyPoint* const* keys_un1,
                                const OrbxKeyPoint* const* keys_un2, const int32_t* const* matches12, const float* const* P3D,
                                const float* inv_level_sigma2, const float* scale_factors, int nlevels, OrbbResult* out, OrbbPoint* const* points)
{
    if (n_problems == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    std::vector<int32_t> feat0;
    int rc = orbb_check_args(problems, n_problems, matches12, P3D, inv_level_sigma2, scale_factors, nlevels, out, points, feat0);
    if (rc) return rc;
    if (!keys_un1 || !keys_un2) return fail(ORBX_E_INVALID, "null key arrays");
    for (int p = 0; p < n_problems; p++) {
        const OrbbProblem& pr = problems[p];
        if ((pr.n1 && !keys_un1[p]) || (pr.n2 && !keys_un2[p])) return fail(ORBX_E_INVALID, "problem %d: null key array", p);
        for (int i = 0; i < pr.n1; i++) {
            const int m = matches12[p][i];
            if (m < 0) continue;
            const OrbxKeyPoint &k1 = keys_un1[p][i], &k2 = keys_un2[p][m];
            if (k1.octave < 0 || k1.octave >= nlevels) return fail(ORBX_E_INVALID, "problem %d: octave %d of feature %d outside [0, %d)", p, k1.octave, i, nlevels);
            if (k2.octave < 0 || k2.octave >= nlevels)
                return fail(ORBX_E_INVALID, "problem %d: octave %d of the second frame's feature %d outside [0, %d)", p, k2.octave, m, nlevels);
            if (!std::isfinite(k1.x) || !std::isfinite(k1.y) || !std::isfinite(k2.x) || !std::isfinite(k2.y))
                return fail(ORBX_E_INVALID, "problem %d: a key of the match of feature %d is not finite", p, i);
        }
    }
    if ((rc = orbm_check(h))) return rc;
    return orbb_core(h, problems, n_problems, keys_un1, keys_un2, nullptr, nullptr, matches12, P3D, inv_level_sigma2, scale_factors, nlevels, out, points, feat0);
}

extern "C" int orbb_initial_map_frames(orbm_t* h, const OrbbProblem* problems, int n_problems, orbm_frame_t* const* frames1, orbm_frame_t* const* frames2,
                                       const int32_t* const* matches12, const float* const* P3D, const float* inv_level_sigma2,
                                       const float* scale_factors, int nlevels, OrbbResult* out, OrbbPoint* const* points)
{
    if (n_problems == 0) return ORBX_OK;
    std::vector<int32_t> feat0;
    int rc = orbb_check_args(problems, n_problems, matches12, P3D, inv_level_sigma2, scale_factors, nlevels, out, points, feat0);
    if (rc) return rc;
    if (!frames1 || !frames2) return fail(ORBX_E_INVALID, "null frame");
    for (int p = 0; p < n_problems; p++) {
        if (!frames1[p] || !frames1[p]->owner || !frames2[p] || !frames2[p]->owner) return fail(ORBX_E_INVALID, "null frame");
        if (frames1[p]->n != problems[p].n1 || frames2[p]->n != problems[p].n2)
            return fail(ORBX_E_INVALID, "problem %d: n1 / n2 are %d / %d, the frames hold %d / %d features", p, problems[p].n1, problems[p].n2, frames1[p]->n,
                        frames2[p]->n);
    }
    if ((rc = orbm_check(h))) return rc;
    for (int p = 0; p < n_problems; p++) if ((rc = frame_usable(h, frames1[p])) || (rc = frame_usable(h, frames2[p]))) return rc;
    return orbb_core(h, problems, n_problems, nullptr, nullptr, frames1, frames2, matches12, P3D, inv_level_sigma2, scale_factors, nlevels, out, points, feat0);
}
