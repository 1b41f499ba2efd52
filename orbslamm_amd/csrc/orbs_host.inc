// orbs_host.inc -- host side of the device Sim3Solver (part of orbslamm_hip.hip; kernels: orbs_kernels.hip, DESIGN.md §8i).
// orbs_run is one chain for a whole batch of solvers with the host in the middle once: the fit kernel leaves one
// quaternion per hypothesis, the host turns it into mR12i with libm's binary64 atan2 / cos / sin (what the reference
// calls; the device's are other implementations), the pose and score kernels finish.  orbs_iterate replays the
// reference's iterate over the per-hypothesis table with the solver's state, on integers.

struct orbs_solver : orbm_ransac_base<OrbsHypothesis> {  // (a batch's transit buffers, d_work and h_stage, live in its first solver)
    orbs_solver() { minInliers = 6; }
    int n1 = 0, fixScale = 0;
    float cam[32] = {0};                 // Rcw1, tcw1, Rcw2, tcw2, K1, K2
    std::vector<int32_t> idx1;           // mvnIndices1
    float4* d_pts = nullptr;             // three planes of n (orbs::Desc::pts)
    float* d_cam = nullptr;
    float* d_pose = nullptr; int poseCap = 0;   // iterations x kPoseWords
    // iterate's state beyond the base's (runMs: up + fit + down, host libm, up + pose + score + down)
    bool hasBest = false;
    float bestT12[16] = {0}, bestR[9] = {0}, bestT[3] = {0}, bestS = 0.f;
};

static_assert(sizeof(OrbsHypothesis) == orbs::kHypWords * 4, "OrbsHypothesis layout");

static void orbs_free(orbs_solver* s)
{
    if (!s) return;
    s->release({s->d_pts, s->d_cam, s->d_pose, s->d_mask});
    delete s;
}

extern "C" void orbs_destroy(orbs_t* s) { orbs_free(s); }

// SetRansacParameters' mRansacMaxIts (Sim3Solver.cc:122-147): epsilon is derived from the counts
static int orbs_ransac_iterations(int n, double probability, int minInliers, int maxIterations)
{
    return ransac_iterations(n, probability, minInliers, maxIterations, (float)minInliers / n);
}

extern "C" int orbs_set_ransac(orbs_t* s, double probability, int min_inliers, int max_iterations)
{
    if (!s) return fail(ORBX_E_INVALID, "null argument");
    const int its = orbs_ransac_iterations(s->n, probability, min_inliers, max_iterations);
    if (its > ORBS_MAX_ITERATIONS) return fail(ORBX_E_UNSUPPORTED, "%d iterations: above %d", its, ORBS_MAX_ITERATIONS);
    if (s->n < 3 && s->n >= min_inliers)
        return fail(ORBX_E_UNSUPPORTED, "%d correspondences with min_inliers %d: the reference would draw from an emptied vector", s->n, min_inliers);
    s->prob = probability;
    s->minInliers = min_inliers;
    s->maxIts = its;
    s->nIterations = 0;
    s->tableValid = false;
    return ORBX_OK;
}

extern "C" int orbs_create(orbm_t* h, int n1, const int32_t* idx1, int n, const float* X1w, const float* X2w, const float Rcw1[9],
                           const float tcw1[3], const float Rcw2[9], const float tcw2[3], const float K1[4], const float K2[4],
                           const float* sigma2_1, const float* sigma2_2, int fix_scale, orbs_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!Rcw1 || !tcw1 || !Rcw2 || !tcw2 || !K1 || !K2 || n < 0 || n1 < 0 || (n && (!idx1 || !X1w || !X2w || !sigma2_1 || !sigma2_2)))
        return fail(ORBX_E_INVALID, "bad argument");
    if (n > ORBS_MAX_POINTS) return fail(ORBX_E_UNSUPPORTED, "%d correspondences: above %d", n, ORBS_MAX_POINTS);
    for (int i = 0; i < n; i++)
        if (idx1[i] < 0 || idx1[i] >= n1) return fail(ORBX_E_INVALID, "idx1[%d] = %d outside [0, %d)", i, idx1[i], n1);
    orbs_solver* s = new orbs_solver();
    s->attach(h);
    s->n1 = n1; s->n = n; s->fixScale = fix_scale ? 1 : 0;
    s->idx1.assign(idx1, idx1 + n);
    memcpy(s->cam, Rcw1, 36); memcpy(s->cam + 9, tcw1, 12); memcpy(s->cam + 12, Rcw2, 36); memcpy(s->cam + 21, tcw2, 12);
    memcpy(s->cam + 24, K1, 16); memcpy(s->cam + 28, K2, 16);
    const int np = std::max(n, 1);
    HIPCHK_OR(hipMalloc((void**)&s->d_pts, (size_t)np * 5 * sizeof(float4)), orbs_free(s));   // three planes, then the two input planes
    HIPCHK_OR(hipMalloc((void**)&s->d_cam, sizeof s->cam), orbs_free(s));
    HIPCHK_OR(hipMalloc((void**)&s->d_mask, (size_t)np), orbs_free(s));
    HIPCHK_OR(hipMemcpyAsync(s->d_cam, s->cam, sizeof s->cam, hipMemcpyHostToDevice, h->stream), orbs_free(s));
    if (n) {
        std::vector<float4> in((size_t)2 * n);
        for (int i = 0; i < n; i++) {
            in[i] = make_float4(X1w[i * 3], X1w[i * 3 + 1], X1w[i * 3 + 2], sigma2_1[i]);
            in[(size_t)n + i] = make_float4(X2w[i * 3], X2w[i * 3 + 1], X2w[i * 3 + 2], sigma2_2[i]);
        }
        float4* d_in = s->d_pts + (size_t)3 * n;
        HIPCHK_OR(hipMemcpyAsync(d_in, in.data(), in.size() * sizeof(float4), hipMemcpyHostToDevice, h->stream), orbs_free(s));
        hipLaunchKernelGGL(orbs::k_sim3_points, dim3((n + orbs::kPointThreads - 1) / orbs::kPointThreads), dim3(orbs::kPointThreads), 0, h->stream,
                           (const float4*)d_in, n, (const float*)s->d_cam, s->d_pts);
        HIPCHK_OR(hipGetLastError(), orbs_free(s));
        HIPCHK_OR(hipStreamSynchronize(h->stream), orbs_free(s));   // (`in` is pageable and local)
    } else
        HIPCHK_OR(hipStreamSynchronize(h->stream), orbs_free(s));
    // the constructor ends in SetRansacParameters()
    s->maxIts = orbs_ransac_iterations(n, s->prob, s->minInliers, 300);
    *out = s;
    return ORBX_OK;
}

extern "C" int orbs_size(orbs_t* s, int* n, int* n1)
{
    if (!s || !n || !n1) return fail(ORBX_E_INVALID, "null argument");
    *n = s->n; *n1 = s->n1;
    return ORBX_OK;
}

extern "C" int orbs_max_iterations(orbs_t* s, int* iterations)
{
    if (!s || !iterations) return fail(ORBX_E_INVALID, "null argument");
    *iterations = s->maxIts;
    return ORBX_OK;
}

extern "C" int orbs_points(orbs_t* s, float* out)
{
    if (!s || (s->n && !out)) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbm_check(s->h);
    if (rc) return rc;
    if (!s->n) return ORBX_OK;
    HIPCHK(hipMemcpyAsync(out, s->d_pts, (size_t)s->n * 3 * sizeof(float4), hipMemcpyDeviceToHost, s->h->stream));
    HIPCHK(hipStreamSynchronize(s->h->stream));
    return ORBX_OK;
}

// the quaternion evec.row(0) to mR12i (Sim3Solver.cc:277-288 and cvRodrigues2's vector branch), in binary64 through libm
static void orbs_rotation(const float q[4], float R[9])
{
    float vec[3] = {q[1], q[2], q[3]};
    // cv::norm: double sum of squares in order
    double ss = 0;
    for (int k = 0; k < 3; k++) ss += (double)vec[k] * (double)vec[k];
    const double nrm = std::sqrt(ss);
    const double ang = std::atan2(nrm, (double)q[0]);
    // vec = 2*ang*vec/norm(vec): one MatExpr, alpha = (2*ang) * (1./norm); 0 * inf = NaN when the imaginary part is zero
    const double alpha = (2 * ang) * (1. / nrm);
    for (int k = 0; k < 3; k++) vec[k] = cvm::expr_scale(vec[k], alpha);
    double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.f : 0.f;
        return;
    }
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double c = std::cos(theta), sn = std::sin(theta), c1 = 1. - c;
    const double itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) R[k] = (float)(c * I[k] + c1 * rrt[k] + sn * r_x[k]);
}

extern "C" int orbs_run(orbs_t* const* solvers, int count, const int32_t* const* sets)
{
    if (!solvers || !sets || count < 1) return fail(ORBX_E_INVALID, "bad argument");
    orbm_handle* h = nullptr;
    int rc = ransac_batch(solvers, count, &h);
    if (rc) return rc;
    // a solver with N < mRansacMinInliers never draws (iterate returns bNoMore at once): nothing to compute for it
    std::vector<int> act;
    int total = 0, maxIts = 0;
    for (int c = 0; c < count; c++) {
        orbs_solver* s = solvers[c];
        if (s->n < s->minInliers) continue;
        if (s->n < 3) return fail(ORBX_E_UNSUPPORTED, "solvers[%d]: %d correspondences with min_inliers %d: the reference would draw from an emptied vector", c, s->n, s->minInliers);
        if (!sets[c]) return fail(ORBX_E_INVALID, "sets[%d] is null", c);
        for (int k = 0; k < s->maxIts * 3; k++)
            if (sets[c][k] < 0 || sets[c][k] >= s->n) return fail(ORBX_E_INVALID, "sets[%d][%d] = %d outside [0, %d)", c, k, sets[c][k], s->n);
        act.push_back(c);
        total += s->maxIts;
        maxIts = std::max(maxIts, s->maxIts);
    }
    const int na = (int)act.size();
    if (na) {
        for (int c : act) {
            orbs_solver* s = solvers[c];
            if (s->maxIts > s->poseCap) {
                HIPCHK(hipStreamSynchronize(h->stream));
                if (s->d_pose) HIPCHK(hipFree(s->d_pose));
                s->d_pose = nullptr; s->poseCap = 0;
                HIPCHK(hipMalloc((void**)&s->d_pose, (size_t)s->maxIts * orbs::kPoseWords * 4));
                s->poseCap = s->maxIts;
            }
        }
        Packer pk;
        const size_t oDesc = pk.take((size_t)na * sizeof(orbs::Desc)), oSets = pk.take((size_t)total * 12), upBytes = pk.off;
        const size_t oQuat = pk.take((size_t)total * 16), oRot = pk.take((size_t)total * 36), oHyp = pk.take((size_t)total * sizeof(OrbsHypothesis)),
                     work = pk.off;
        orbs_solver* own = solvers[act[0]];
        if ((rc = own->reserve(work, work))) return rc;
        uint8_t* hs = own->h_stage;
        uint8_t* d = (uint8_t*)own->d_work;
        orbs::Desc* hd = (orbs::Desc*)(hs + oDesc);
        int base = 0;
        for (int a = 0; a < na; a++) {
            orbs_solver* s = solvers[act[a]];
            orbs::Desc& D = hd[a];
            D.pts = s->d_pts; D.pose = s->d_pose; D.n = s->n; D.iters = s->maxIts; D.hypBase = base; D.fixScale = s->fixScale;
            memcpy(D.K1, s->cam + 24, 16); memcpy(D.K2, s->cam + 28, 16);
            memcpy(hs + oSets + (size_t)base * 12, sets[act[a]], (size_t)s->maxIts * 12);
            base += s->maxIts;
        }
        hipStream_t st = h->stream;
        const auto c0 = std::chrono::steady_clock::now();
        const orbs::Desc* dd = (const orbs::Desc*)(d + oDesc);
        const int32_t* ds = (const int32_t*)(d + oSets);
        HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(orbs::k_sim3_fit, dim3((total + orbs::kFitThreads - 1) / orbs::kFitThreads), dim3(orbs::kFitThreads), 0, st, dd, na, total, ds,
                           (float*)(d + oQuat));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs + oQuat, d + oQuat, (size_t)total * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const auto c1 = std::chrono::steady_clock::now();
        const float* q = (const float*)(hs + oQuat);
        float* R = (float*)(hs + oRot);
        for (int g = 0; g < total; g++) orbs_rotation(q + (size_t)g * 4, R + (size_t)g * 9);
        const auto c2 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpyAsync(d + oRot, hs + oRot, (size_t)total * 36, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(orbs::k_sim3_pose, dim3((total + orbs::kPoseThreads - 1) / orbs::kPoseThreads), dim3(orbs::kPoseThreads), 0, st, dd, na, total, ds,
                           (const float*)(d + oRot), (float*)(d + oHyp));
        hipLaunchKernelGGL(orbs::k_sim3_score, dim3((maxIts + orbs::kHypPerBlock - 1) / orbs::kHypPerBlock, na), dim3(orbs::kScoreThreads), 0, st, dd,
                           (int32_t*)(d + oHyp));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs + oHyp, d + oHyp, (size_t)total * sizeof(OrbsHypothesis), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const auto c3 = std::chrono::steady_clock::now();
        for (int c = 0; c < count; c++) {
            solvers[c]->runMs[0] = std::chrono::duration<double, std::milli>(c1 - c0).count();
            solvers[c]->runMs[1] = std::chrono::duration<double, std::milli>(c2 - c1).count();
            solvers[c]->runMs[2] = std::chrono::duration<double, std::milli>(c3 - c2).count();
        }
        const OrbsHypothesis* ht = (const OrbsHypothesis*)(hs + oHyp);
        base = 0;
        for (int a = 0; a < na; a++) {
            orbs_solver* s = solvers[act[a]];
            s->table.assign(ht + base, ht + base + s->maxIts);
            base += s->maxIts;
        }
    }
    for (int c = 0; c < count; c++) {
        if (solvers[c]->n < solvers[c]->minInliers) solvers[c]->table.clear();
        solvers[c]->tableValid = true;
    }
    return ORBX_OK;
}

extern "C" int orbs_hypotheses(orbs_t* s, OrbsHypothesis* out, int cap, int* n_out)
{
    return s ? s->hypotheses("orbs", out, cap, n_out) : fail(ORBX_E_INVALID, "bad argument");
}

extern "C" int orbs_last_run_ms(orbs_t* s, double ms[3])
{
    if (!s || !ms) return fail(ORBX_E_INVALID, "null argument");
    for (int k = 0; k < 3; k++) ms[k] = s->runMs[k];
    return ORBX_OK;
}

static void orbs_fill_result(const orbs_solver* s, OrbsResult* r)
{
    r->iterations = s->nIterations;
    r->best_inliers = s->bestInliers;
    r->has_best = s->hasBest ? 1 : 0;
    memcpy(r->best_R, s->bestR, sizeof s->bestR);
    memcpy(r->best_t, s->bestT, sizeof s->bestT);
    r->best_s = s->bestS;
}

// iterate (Sim3Solver.cc:149-224) over the table
extern "C" int orbs_iterate(orbs_t* s, int n_iterations, OrbsResult* res, uint8_t* inliers)
{
    if (!s || !res || (s->n1 && !inliers)) return fail(ORBX_E_INVALID, "null argument");
    memset(res, 0, sizeof *res);
    res->hypothesis = -1;
    if (s->n < s->minInliers) {
        if (s->n1) memset(inliers, 0, (size_t)s->n1);
        res->no_more = 1;
        orbs_fill_result(s, res);
        return ORBX_OK;
    }
    if (!s->tableValid) return fail(ORBX_E_INVALID, "no table: orbs_run comes first");
    if (s->n1) memset(inliers, 0, (size_t)s->n1);
    int nCurrentIterations = 0;
    while (s->nIterations < s->maxIts && nCurrentIterations < n_iterations) {
        nCurrentIterations++;
        s->nIterations++;
        const OrbsHypothesis& hy = s->table[s->nIterations - 1];
        if (hy.n_inliers >= s->bestInliers) {
            s->bestInliers = hy.n_inliers;
            memcpy(s->bestT12, hy.T12, sizeof hy.T12);
            memcpy(s->bestR, hy.R12, sizeof hy.R12);
            memcpy(s->bestT, hy.t12, sizeof hy.t12);
            s->bestS = hy.s12;
            s->hasBest = true;
            if (hy.n_inliers > s->minInliers) {
                // the flags of this hypothesis, recomputed on the device from its stored T12 / T21
                orbm_handle* h = s->h;
                int rc = orbm_check(h);
                if (rc) { s->nIterations--; return rc; }
                hipLaunchKernelGGL(orbs::k_sim3_mask, dim3((s->n + orbs::kPointThreads - 1) / orbs::kPointThreads), dim3(orbs::kPointThreads), 0, h->stream,
                                   (const float4*)s->d_pts, s->n, (const float*)(s->d_pose + (size_t)(s->nIterations - 1) * orbs::kPoseWords),
                                   (const float*)s->d_cam, s->d_mask);
                if ((rc = s->scatter_mask(s->idx1, inliers))) return rc;
                res->n_inliers = hy.n_inliers;
                res->returned = 1;
                res->hypothesis = s->nIterations - 1;
                memcpy(res->T12, s->bestT12, sizeof s->bestT12);
                orbs_fill_result(s, res);
                return ORBX_OK;
            }
        }
    }
    if (s->nIterations >= s->maxIts) res->no_more = 1;
    orbs_fill_result(s, res);
    return ORBX_OK;
}
