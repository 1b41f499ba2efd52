// orbz_host.inc -- host side of the device OptimizeSim3 (part of orbslamm_hip.hip; kernel: orbz_kernels.hip, ABI:
// include/orbslamm_sim3opt.h, DESIGN.md §8p).  One call = the checks, one packed upload (problem records | correspondences | the two level tables),
// ONE launch for all problems, one copy of the results and the removed bytes down, one synchronise.

static_assert(sizeof(OrbzProblem) == 200 && sizeof(OrbzCorr) == 52 && sizeof(OrbzResult) == 128, "orbslamm_sim3opt.h layouts");
static_assert(orbz::kMaxCorr == ORBZ_MAX_CORR && orbz::kMaxProblems == ORBZ_MAX_PROBLEMS, "orbz limits");
static_assert(ORBZ_MAX_CALL_CORR < INT32_MAX / 128, "a call's correspondence total and its byte offsets per correspondence stay small");

// what needs neither the handle nor a GPU.  Zero problems are settled by the caller before this: ORBX_OK, nothing read
static int orbz_check_args(const OrbzProblem* problems, int n_problems, const int32_t* corr_start, const OrbzCorr* corrs, const float* sigma1,
                           const float* sigma2, int nlevels, const OrbzResult* out, const uint8_t* removed)
{
    if (n_problems < 0) return fail(ORBX_E_INVALID, "negative problem count");
    if (n_problems > ORBZ_MAX_PROBLEMS) return fail(ORBX_E_UNSUPPORTED, "%d problems: above %d", n_problems, ORBZ_MAX_PROBLEMS);
    if (!sigma1 || !sigma2 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS)
        return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d] or no sigma table", nlevels, ORBX_MAX_LEVELS);
    if (!corr_start) return fail(ORBX_E_INVALID, "null corr_start");
    if (corr_start[0] != 0) return fail(ORBX_E_INVALID, "corr_start[0] = %d: it starts at 0", corr_start[0]);
    for (int p = 0; p < n_problems; p++) {
        if (corr_start[p + 1] < corr_start[p]) return fail(ORBX_E_INVALID, "corr_start descends at problem %d", p);
        if (corr_start[p + 1] - corr_start[p] > ORBZ_MAX_CORR)
            return fail(ORBX_E_UNSUPPORTED, "%d correspondences in problem %d: above %d", corr_start[p + 1] - corr_start[p], p, ORBZ_MAX_CORR);
        if (corr_start[p + 1] > ORBZ_MAX_CALL_CORR)
            return fail(ORBX_E_UNSUPPORTED, "more than %d correspondences in one call (reached at problem %d)", ORBZ_MAX_CALL_CORR, p);
    }
    if (!problems || !out) return fail(ORBX_E_INVALID, "null argument");
    if (corr_start[n_problems] && (!corrs || !removed)) return fail(ORBX_E_INVALID, "null argument");
    for (int p = 0; p < n_problems; p++) {
        const float th2 = problems[p].th2;
        if (!(th2 > 0.f) || !(th2 <= FLT_MAX)) return fail(ORBX_E_INVALID, "problem %d: th2 %g is not a finite positive number", p, (double)th2);
        for (int c = corr_start[p]; c < corr_start[p + 1]; c++) {
            if (corrs[c].oct1 < 0 || corrs[c].oct1 >= nlevels)
                return fail(ORBX_E_INVALID, "correspondence %d: octave %d of keyframe 1 outside [0, %d)", c, corrs[c].oct1, nlevels);
            if (corrs[c].oct2 < 0 || corrs[c].oct2 >= nlevels)
                return fail(ORBX_E_INVALID, "correspondence %d: octave %d of keyframe 2 outside [0, %d)", c, corrs[c].oct2, nlevels);
        }
    }
    return ORBX_OK;
}

extern "C" int orbz_optimize_sim3(orbm_t* h, const OrbzProblem* problems, int n_problems, const int32_t* corr_start, const OrbzCorr* corrs,
                                  const float* inv_level_sigma2_1, const float* inv_level_sigma2_2, int nlevels, OrbzResult* out, uint8_t* removed)
{
    if (n_problems == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbz_check_args(problems, n_problems, corr_start, corrs, inv_level_sigma2_1, inv_level_sigma2_2, nlevels, out, removed);
    if (rc) return rc;
    if ((rc = orbm_check(h))) return rc;
    const size_t total = (size_t)corr_start[n_problems];
    Packer pk;
    const size_t oProb = pk.take((size_t)n_problems * sizeof(orbz::ProblemIn)), oCorr = pk.take(total * sizeof(OrbzCorr)),
                 oSigma = pk.take(2 * ORBX_MAX_LEVELS * sizeof(float)), upBytes = pk.off;
    const size_t oPw = pk.take(2 * total * sizeof(float4)), oUv = pk.take(2 * total * sizeof(float2)), oOff = pk.take(2 * total);
    const size_t oOut = pk.take((size_t)n_problems * sizeof(OrbzResult)), oFlags = pk.take(total), work = pk.off;
    const size_t downBytes = work - oOut;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orbz::ProblemIn* hp = (orbz::ProblemIn*)(hs + oProb);
    for (int p = 0; p < n_problems; p++) {
        memset(&hp[p], 0, sizeof hp[p]);
        hp[p].p = problems[p];
        const float deltaHuber = std::sqrt(problems[p].th2);   // :1398: the float square root of the float
        hp[p].delta = (double)deltaHuber;
        hp[p].c0 = corr_start[p]; hp[p].n = corr_start[p + 1] - corr_start[p];
    }
    if (total) memcpy(hs + oCorr, corrs, total * sizeof(OrbzCorr));
    orbz::Args a{};
    a.problems = (const orbz::ProblemIn*)(d + oProb); a.corrs = (const OrbzCorr*)(d + oCorr);
    a.pw = (float4*)(d + oPw); a.uv = (float2*)(d + oUv); a.off = d + oOff; a.out = (OrbzResult*)(d + oOut); a.removed = d + oFlags;
    float* hsig = (float*)(hs + oSigma);
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) {
        hsig[l] = l < nlevels ? inv_level_sigma2_1[l] : 0.f;
        hsig[ORBX_MAX_LEVELS + l] = l < nlevels ? inv_level_sigma2_2[l] : 0.f;
    }
    a.invSigma2 = (const float*)(d + oSigma);
    a.nlevels = nlevels;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d + oOut, 0, (size_t)n_problems * sizeof(OrbzResult), s));
    hipLaunchKernelGGL(orbz::k_sim3_optimize, dim3((unsigned)n_problems), dim3(orbz::kLanes), 0, s, a, n_problems);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oOut, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out, hs, (size_t)n_problems * sizeof(OrbzResult));
    if (total) memcpy(removed, hs + (oFlags - oOut), total);
    return ORBX_OK;
}
