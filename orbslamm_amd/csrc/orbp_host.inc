// orbp_host.inc -- host side of the device PnPsolver (part of orbslamm_hip.hip; kernels: orbp_kernels.hip, DESIGN.md §8j).
// orbp_run is one chain for all solvers of a frame: fit, score, records, Refine of every record, the table down.
// orbp_iterate replays the reference's iterate over the per-hypothesis table with the solver's state, on integers; the
// mask it hands back is recomputed on the device for the returned pose.

struct orbp_solver : orbm_ransac_base<OrbpHypothesis> {  // (a batch's transit buffers, d_work and h_stage, live in its first solver)
    orbp_solver() { minInliers = 8; }
    int nAll = 0;
    float K[4] = {0};
    std::vector<int32_t> idx;            // mvKeyPointIndices
    float4* d_pts = nullptr;             // (P3Dw, sigma2)
    float2* d_uv = nullptr;              // P2D
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // SetRansacParameters / iterate's state beyond the base's
    float eps = 0.4f, th2 = 5.991f;
    int bestHyp = -1;
    float bestTcw[16] = {0};
};

static_assert(sizeof(OrbpHypothesis) == sizeof(orbp::Hyp) && sizeof(OrbpHypothesis) == 208, "OrbpHypothesis layout");
static_assert(sizeof(OrbpResult) == 160, "OrbpResult layout");
static_assert(orbp::kMaxPoints == ORBP_MAX_POINTS && orbp::kMaxIterations == ORBP_MAX_ITERATIONS, "orbp limits");

static void orbp_free(orbp_solver* s)
{
    if (!s) return;
    if (s->h) (void)hipSetDevice(s->h->device);
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    s->release({s->d_pts, s->d_uv, s->d_mask});
    delete s;
}

extern "C" void orbp_destroy(orbp_t* s) { orbp_free(s); }

// SetRansacParameters (PnPsolver.cc:121-157) on a copy of the parameters: epsilon is given, and raised to the inlier share
static void orbp_ransac_parameters(int N, double probability, int& minInliers, int& maxIts, int minSet, float& epsilon)
{
    int nMinInliers = (int)(N * epsilon);
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    minInliers = nMinInliers;
    if (epsilon < (float)minInliers / N) epsilon = (float)minInliers / N;
    maxIts = ransac_iterations(N, probability, minInliers, maxIts, epsilon);
}

extern "C" int orbp_set_ransac(orbp_t* s, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2)
{
    if (!s) return fail(ORBX_E_INVALID, "null argument");
    if (min_set != 4) return fail(ORBX_E_UNSUPPORTED, "min_set %d: EPnP's RANSAC draws sets of 4", min_set);
    int mi = min_inliers, its = max_iterations;
    float e = epsilon;
    orbp_ransac_parameters(s->n, probability, mi, its, min_set, e);
    if (its > ORBP_MAX_ITERATIONS) return fail(ORBX_E_UNSUPPORTED, "%d iterations: above %d", its, ORBP_MAX_ITERATIONS);
    s->prob = probability; s->minInliers = mi; s->maxIts = its; s->eps = e; s->th2 = th2;
    s->tableValid = false;
    return ORBX_OK;
}

// the constructor behind both create entries.  f == nullptr: P2D and sigma2 are host arrays; else they are gathered on the
// device from the resident frame's undistorted keys (k_pnp_gather), sigma2 being level_sigma2 (n_levels floats, host)
static int orbp_make(orbm_handle* h, orbm_frame* f, int n_all, const int32_t* idx, int n, const float* P2D, const float* sigma2, const float* P3Dw,
                     const float* level_sigma2, int n_levels, const float K[4], orbp_t** out)
{
    if (n == 0) return fail(ORBX_E_UNSUPPORTED, "no correspondences: the reference divides by N");
    if (n > ORBP_MAX_POINTS) return fail(ORBX_E_UNSUPPORTED, "%d correspondences: above %d", n, ORBP_MAX_POINTS);
    for (int i = 0; i < n; i++)
        if (idx[i] < 0 || idx[i] >= n_all) return fail(ORBX_E_INVALID, "idx[%d] = %d outside [0, %d)", i, idx[i], n_all);
    orbp_solver* s = new orbp_solver();
    s->attach(h);
    s->nAll = n_all; s->n = n;
    s->idx.assign(idx, idx + n);
    memcpy(s->K, K, sizeof s->K);
    HIPCHK_OR(hipMalloc((void**)&s->d_pts, (size_t)n * sizeof(float4)), orbp_free(s));
    HIPCHK_OR(hipMalloc((void**)&s->d_uv, (size_t)n * sizeof(float2)), orbp_free(s));
    HIPCHK_OR(hipMalloc((void**)&s->d_mask, (size_t)n), orbp_free(s));
    for (hipEvent_t& e : s->ev) HIPCHK_OR(hipEventCreate(&e), orbp_free(s));
    std::vector<float4> pts((size_t)n);
    for (int i = 0; i < n; i++) pts[i] = make_float4(P3Dw[i * 3], P3Dw[i * 3 + 1], P3Dw[i * 3 + 2], f ? 0.f : sigma2[i]);
    HIPCHK_OR(hipMemcpyAsync(s->d_pts, pts.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream), orbp_free(s));
    if (!f)
        HIPCHK_OR(hipMemcpyAsync(s->d_uv, P2D, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream), orbp_free(s));
    else {
        // the indices and the level table ride in the work block: idx (n) | level_sigma2 (n_levels)
        Packer pk;
        const size_t oIdx = pk.take((size_t)n * 4), oLev = pk.take((size_t)n_levels * 4);
        int rc = s->reserve(pk.off, pk.off);
        if (rc) { orbp_free(s); return rc; }
        memcpy(s->h_stage + oIdx, idx, (size_t)n * 4);
        memcpy(s->h_stage + oLev, level_sigma2, (size_t)n_levels * 4);
        uint8_t* d = (uint8_t*)s->d_work;
        HIPCHK_OR(hipMemcpyAsync(d, s->h_stage, pk.off, hipMemcpyHostToDevice, h->stream), orbp_free(s));
        hipLaunchKernelGGL(orbp::k_pnp_gather, dim3((n + orbp::kPointThreads - 1) / orbp::kPointThreads), dim3(orbp::kPointThreads), 0, h->stream,
                           (const orbm::KeyDev*)f->d_keysUn, (const int32_t*)(d + oIdx), n, (const float*)(d + oLev), n_levels, s->d_pts, s->d_uv);
        HIPCHK_OR(hipGetLastError(), orbp_free(s));
    }
    HIPCHK_OR(hipStreamSynchronize(h->stream), orbp_free(s));   // (`pts` is pageable and local)
    // the constructor ends in SetRansacParameters()
    orbp_ransac_parameters(n, s->prob, s->minInliers, s->maxIts, 4, s->eps);
    *out = s;
    return ORBX_OK;
}

extern "C" int orbp_create(orbm_t* h, int n_all, const int32_t* idx, int n, const float* P2D, const float* sigma2, const float* P3Dw, const float K[4],
                           orbp_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!K || n < 0 || n_all < 0 || (n && (!idx || !P2D || !sigma2 || !P3Dw))) return fail(ORBX_E_INVALID, "bad argument");
    return orbp_make(h, nullptr, n_all, idx, n, P2D, sigma2, P3Dw, nullptr, 0, K, out);
}

extern "C" int orbp_create_frame(orbm_t* h, orbm_frame_t* f, const int32_t* idx, int n, const float* P3Dw, const float* level_sigma2, int n_levels,
                                 const float K[4], orbp_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    int rc = orbm_check(h);
    if (rc || (rc = frame_usable(h, f))) return rc;
    if (!K || n < 0 || !level_sigma2 || n_levels < 1 || n_levels > ORBX_MAX_LEVELS || (n && (!idx || !P3Dw))) return fail(ORBX_E_INVALID, "bad argument");
    return orbp_make(h, f, f->n, idx, n, nullptr, nullptr, P3Dw, level_sigma2, n_levels, K, out);
}

extern "C" int orbp_size(orbp_t* s, int* n, int* n_all)
{
    if (!s || !n || !n_all) return fail(ORBX_E_INVALID, "null argument");
    *n = s->n; *n_all = s->nAll;
    return ORBX_OK;
}

extern "C" int orbp_max_iterations(orbp_t* s, int* iterations)
{
    if (!s || !iterations) return fail(ORBX_E_INVALID, "null argument");
    *iterations = s->maxIts;
    return ORBX_OK;
}

extern "C" int orbp_min_inliers(orbp_t* s, int* min_inliers)
{
    if (!s || !min_inliers) return fail(ORBX_E_INVALID, "null argument");
    *min_inliers = s->minInliers;
    return ORBX_OK;
}

extern "C" int orbp_run(orbp_t* const* solvers, int count, const int32_t* const* sets, const int32_t* n_sets)
{
    if (!solvers || !sets || !n_sets || count < 1) return fail(ORBX_E_INVALID, "bad argument");
    orbm_handle* h = nullptr;
    int rc = ransac_batch(solvers, count, &h);
    if (rc) return rc;
    // a solver with N < mRansacMinInliers never draws (iterate returns bNoMore at once): nothing to compute for it
    std::vector<int> act;
    int total = 0, maxSets = 0;
    for (int c = 0; c < count; c++) {
        orbp_solver* s = solvers[c];
        // a solver that has iterated CONTINUES its table (the sets given are those of the hypotheses behind it); without a
        // table (SetRansacParameters dropped it, and rewinds nothing) there is nothing to continue
        if ((s->nIterations || s->bestInliers) && !s->tableValid)
            return fail(ORBX_E_UNSUPPORTED, "solvers[%d] has iterated and SetRansacParameters dropped its table: nothing to continue", c);
        if ((s->nIterations || s->bestInliers) && (int)s->table.size() + n_sets[c] > orbp::kMaxSets)
            return fail(ORBX_E_UNSUPPORTED, "solvers[%d]: %d hypotheses behind %d: above %d", c, n_sets[c], (int)s->table.size(), orbp::kMaxSets);
        if (s->n < s->minInliers) continue;
        if (!sets[c]) return fail(ORBX_E_INVALID, "sets[%d] is null", c);
        if (n_sets[c] < 1 || n_sets[c] > orbp::kMaxSets) return fail(ORBX_E_INVALID, "n_sets[%d] = %d outside [1, %d]", c, n_sets[c], orbp::kMaxSets);
        for (int k = 0; k < n_sets[c] * 4; k++)
            if (sets[c][k] < 0 || sets[c][k] >= s->n) return fail(ORBX_E_INVALID, "sets[%d][%d] = %d outside [0, %d)", c, k, sets[c][k], s->n);
        act.push_back(c);
        total += n_sets[c];
        maxSets = std::max(maxSets, n_sets[c]);
    }
    const int na = (int)act.size();
    if (na) {
        constexpr int kLds = orbp::kLaneDoubles * orbp::kFitThreads * (int)sizeof(double);
        static std::atomic<uint64_t> ldsRaised{0};   // (a bit per device: the attribute is the device's, set once)
        if (!(ldsRaised.load() >> (h->device & 63) & 1)) {
            HIPCHK(hipFuncSetAttribute((const void*)orbp::k_pnp_fit, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
            HIPCHK(hipFuncSetAttribute((const void*)orbp::k_pnp_refine, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
            ldsRaised.fetch_or(1ull << (h->device & 63));
        }
        Packer pk;
        const size_t oDesc = pk.take((size_t)na * sizeof(orbp::Desc)), oSets = pk.take((size_t)total * 16), upBytes = pk.off;
        const size_t oHyp = pk.take((size_t)total * sizeof(OrbpHypothesis)), work = pk.off;
        orbp_solver* own = solvers[act[0]];
        if ((rc = own->reserve(work, work))) return rc;
        uint8_t* hs = own->h_stage;
        uint8_t* d = (uint8_t*)own->d_work;
        orbp::Desc* hd = (orbp::Desc*)(hs + oDesc);
        int base = 0;
        for (int a = 0; a < na; a++) {
            orbp_solver* s = solvers[act[a]];
            orbp::Desc& D = hd[a];
            D.pts = s->d_pts; D.uv = s->d_uv; D.n = s->n; D.iters = n_sets[act[a]]; D.hypBase = base; D.minInliers = s->minInliers;
            D.best0 = 0;
            if (s->nIterations || s->bestInliers)
                for (const OrbpHypothesis& hy : s->table) if (hy.is_record) D.best0 = std::max(D.best0, hy.n_inliers);
            D.th2 = s->th2;
            D.fu = s->K[0]; D.fv = s->K[1]; D.uc = s->K[2]; D.vc = s->K[3];   // double members holding the frame's floats
            memcpy(hs + oSets + (size_t)base * 16, sets[act[a]], (size_t)D.iters * 16);
            base += D.iters;
        }
        hipStream_t st = h->stream;
        const auto c0 = std::chrono::steady_clock::now();
        const orbp::Desc* dd = (const orbp::Desc*)(d + oDesc);
        orbp::Hyp* dh = (orbp::Hyp*)(d + oHyp);
        const int fitBlocks = (total + orbp::kFitThreads - 1) / orbp::kFitThreads;
        HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(dh, 0, (size_t)total * sizeof(OrbpHypothesis), st));
        HIPCHK(hipEventRecord(own->ev[0], st));
        hipLaunchKernelGGL(orbp::k_pnp_fit, dim3(fitBlocks), dim3(orbp::kFitThreads), kLds, st, dd, na, total, (const int32_t*)(d + oSets), dh);
        HIPCHK(hipEventRecord(own->ev[1], st));
        hipLaunchKernelGGL(orbp::k_pnp_score, dim3((maxSets + orbp::kHypPerBlock - 1) / orbp::kHypPerBlock, na), dim3(orbp::kScoreThreads), 0, st, dd, dh);
        hipLaunchKernelGGL(orbp::k_pnp_records, dim3((na + 63) / 64), dim3(64), 0, st, dd, na, dh);
        HIPCHK(hipEventRecord(own->ev[2], st));
        hipLaunchKernelGGL(orbp::k_pnp_refine, dim3(fitBlocks), dim3(orbp::kFitThreads), kLds, st, dd, na, total, dh);
        HIPCHK(hipEventRecord(own->ev[3], st));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs + oHyp, d + oHyp, (size_t)total * sizeof(OrbpHypothesis), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const auto c1 = std::chrono::steady_clock::now();
        double ms[4] = {std::chrono::duration<double, std::milli>(c1 - c0).count(), 0, 0, 0};
        for (int k = 0; k < 3; k++) {
            float e = 0.f;
            HIPCHK(hipEventElapsedTime(&e, own->ev[k], own->ev[k + 1]));
            ms[k + 1] = e;
        }
        for (int c = 0; c < count; c++) memcpy(solvers[c]->runMs, ms, sizeof ms);
        const OrbpHypothesis* ht = (const OrbpHypothesis*)(hs + oHyp);
        base = 0;
        for (int a = 0; a < na; a++) {
            orbp_solver* s = solvers[act[a]];
            if (s->nIterations || s->bestInliers) s->table.insert(s->table.end(), ht + base, ht + base + n_sets[act[a]]);
            else s->table.assign(ht + base, ht + base + n_sets[act[a]]);
            base += n_sets[act[a]];
        }
    }
    for (int c = 0; c < count; c++) {
        if (solvers[c]->n < solvers[c]->minInliers) solvers[c]->table.clear();
        solvers[c]->tableValid = true;
    }
    return ORBX_OK;
}

extern "C" int orbp_hypotheses(orbp_t* s, OrbpHypothesis* out, int cap, int* n_out)
{
    return s ? s->hypotheses("orbp", out, cap, n_out) : fail(ORBX_E_INVALID, "bad argument");
}

extern "C" int orbp_last_run_ms(orbp_t* s, double ms[4])
{
    if (!s || !ms) return fail(ORBX_E_INVALID, "null argument");
    for (int k = 0; k < 4; k++) ms[k] = s->runMs[k];
    return ORBX_OK;
}

// Rcw / tcw .convertTo(CV_32F) into eye(4, 4)
static void orbp_tcw(const double R[9], const double t[3], float T[16])
{
    for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r * 3 + c];
        T[r * 4 + 3] = (float)t[r];
    }
}

// the flags of one pose, recomputed on the device and scattered through mvKeyPointIndices
static int orbp_mask(orbp_solver* s, const double R[9], const double t[3], uint8_t* inliers)
{
    orbm_handle* h = s->h;
    int rc = orbm_check(h);
    if (rc) return rc;
    orbp::Pose pose;
    memcpy(pose.v, R, 72); memcpy(pose.v + 9, t, 24);
    hipLaunchKernelGGL(orbp::k_pnp_mask, dim3((s->n + orbp::kPointThreads - 1) / orbp::kPointThreads), dim3(orbp::kPointThreads), 0, h->stream,
                       (const float4*)s->d_pts, (const float2*)s->d_uv, s->n, pose, (double)s->K[0], (double)s->K[1], (double)s->K[2], (double)s->K[3],
                       s->th2, s->d_mask);
    return s->scatter_mask(s->idx, inliers);
}

// iterate (PnPsolver.cc:165-258) over the table.  The state is advanced on copies and committed when the call is known to
// stay inside the table (ORBX_E_CAPACITY leaves the solver as it was).
extern "C" int orbp_iterate(orbp_t* s, int n_iterations, OrbpResult* res, uint8_t* inliers)
{
    if (!s || !res || (s->nAll && !inliers)) return fail(ORBX_E_INVALID, "null argument");
    memset(res, 0, sizeof *res);
    res->hypothesis = -1;
    res->best_hypothesis = s->bestHyp;
    if (s->nAll) memset(inliers, 0, (size_t)s->nAll);
    auto fill = [&](int its, int best, int bestHyp) {
        res->iterations = its; res->best_inliers = best; res->best_hypothesis = bestHyp;
        if (bestHyp >= 0) orbp_tcw(s->table[bestHyp].R, s->table[bestHyp].t, res->best_Tcw);
    };
    if (s->n < s->minInliers) {
        res->no_more = 1;
        res->iterations = s->nIterations; res->best_inliers = s->bestInliers;
        return ORBX_OK;
    }
    if (!s->tableValid) return fail(ORBX_E_INVALID, "no table: orbp_run comes first");
    int its = s->nIterations, best = s->bestInliers, bestHyp = s->bestHyp, cur = 0;
    while (its < s->maxIts || cur < n_iterations) {
        if (its >= (int)s->table.size())
            return fail(ORBX_E_CAPACITY, "iterate(%d) from iteration %d passes the table's %d hypotheses", n_iterations, s->nIterations, (int)s->table.size());
        cur++;
        its++;
        const OrbpHypothesis& hy = s->table[its - 1];
        if (hy.n_inliers >= s->minInliers) {
            if (hy.n_inliers > best) { best = hy.n_inliers; bestHyp = its - 1; }
            // Refine() works on the best mask, whatever the current hypothesis: the record's result
            const OrbpHypothesis& rec = s->table[bestHyp];
            if (rec.refine_ok) {
                const int rc = orbp_mask(s, rec.refine_R, rec.refine_t, inliers);
                if (rc) return rc;
                s->nIterations = its; s->bestInliers = best; s->bestHyp = bestHyp;
                res->returned = 1; res->refined = 1; res->n_inliers = rec.refine_inliers; res->hypothesis = its - 1;
                orbp_tcw(rec.refine_R, rec.refine_t, res->Tcw);
                fill(its, best, bestHyp);
                return ORBX_OK;
            }
        }
    }
    if (its >= s->maxIts) {
        res->no_more = 1;
        if (best >= s->minInliers) {
            const OrbpHypothesis& b = s->table[bestHyp];
            const int rc = orbp_mask(s, b.R, b.t, inliers);
            if (rc) return rc;
            res->returned = 1; res->n_inliers = best; res->hypothesis = bestHyp;
            orbp_tcw(b.R, b.t, res->Tcw);
        }
    }
    s->nIterations = its; s->bestInliers = best; s->bestHyp = bestHyp;
    fill(its, best, bestHyp);
    return ORBX_OK;
}
