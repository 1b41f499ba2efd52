// orbl_host.inc -- host side of the device CreateNewMapPoints (part of orbslamm_hip.hip; kernels: orbl_kernels.hip,
// DESIGN.md §8k).  One call = the baseline gate, ComputeF12, the epipole and the lock-step walk over node ids for every
// neighbour on the host, one packed upload, five launches, one copy down, one synchronise.  Below it: the batched Fuse of
// SearchInNeighbors (orbl_level_breaks, orbl_fuse_batch*, DESIGN.md §8l) on the shared staging of orbf_host.inc.

static_assert(sizeof(OrblNewPoint) == sizeof(orbl::Rec) && sizeof(OrblNewPoint) == 44, "OrblNewPoint layout");
static_assert(sizeof(OrblKeyFrame) == 80, "OrblKeyFrame layout");
static_assert(orbl::kMaxNeighbours == ORBL_MAX_NEIGHBOURS, "orbl limits");
static_assert(orbl::ST_ACCEPTED == ORBL_ST_ACCEPTED && orbl::ST_SCALE == ORBL_ST_SCALE && orbl::ST_NO_MATCH == ORBL_ST_NO_MATCH, "orbl status codes");

// ComputeF12 (LocalMapping.cc:536-553) and SearchForTriangulation's epipole (ORBmatcher.cc:666-672)
extern "C" int orbl_compute_f12(const OrblKeyFrame* kf1, const OrblKeyFrame* kf2, float F12[9], float epipole[2])
{
    if (!kf1 || !kf2 || !F12 || !epipole) return fail(ORBX_E_INVALID, "null argument");
    // R12 = R1w*R2w.t() (GEMM_2_T); t12 = -R1w*R2w.t()*t2w + t1w: the scaled product first, then gemm with C
    float R12[9], M[9], t12[3];
    cvm::mm3_t2(kf1->Rcw, kf2->Rcw, R12);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)kf1->Rcw[3 * i + k] * (double)kf2->Rcw[3 * j + k];
            M[3 * i + j] = (float)(s * -1.0);
        }
    for (int i = 0; i < 3; i++)
        t12[i] = cvm::gemm3_elem(M[3 * i], M[3 * i + 1], M[3 * i + 2], kf2->tcw[0], kf2->tcw[1], kf2->tcw[2], 1.0, kf1->tcw[i], 1.0);
    const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    // K1.t().inv()*t12x*R12*K2.inv(): both inverses evaluated (cv::invert's 3x3 branch), three plain products left to right
    const float K1t[9] = {kf1->K[0], 0.f, 0.f, 0.f, kf1->K[1], 0.f, kf1->K[2], kf1->K[3], 1.f};
    const float K2[9] = {kf2->K[0], 0.f, kf2->K[2], 0.f, kf2->K[1], kf2->K[3], 0.f, 0.f, 1.f};
    float K1ti[9], K2i[9], P[9], Q[9];
    cvm::inv3(K1t, K1ti);
    cvm::inv3(K2, K2i);
    cvm::mm3(K1ti, t12x, P);
    cvm::mm3(P, R12, Q);
    cvm::mm3(Q, K2i, F12);
    // C2 = R2w*Cw + t2w (gemm with C); ex = fx*C2(0)*invz + cx in float
    float C2[3];
    for (int i = 0; i < 3; i++)
        C2[i] = cvm::gemm3_elem(kf2->Rcw[3 * i], kf2->Rcw[3 * i + 1], kf2->Rcw[3 * i + 2], kf1->Ow[0], kf1->Ow[1], kf1->Ow[2], 1.0, kf2->tcw[i], 1.0);
    const float invz = 1.0f / C2[2];
    epipole[0] = kf2->K[0] * C2[0] * invz + kf2->K[2];
    epipole[1] = kf2->K[1] * C2[1] * invz + kf2->K[3];
    return ORBX_OK;
}

// one keyframe's side as the core takes it: arrays resident in HBM (a frame's), or host arrays that ride in the call's
// staging block (dev == false: the pointers are host pointers, fvStart holds n_nodes + 1 entries, fvIdx fvStart[n_nodes])
struct OrblSide {
    bool dev;
    const void* keys; const uint8_t* desc; const int32_t* fvStart; const int32_t* fvIdx;
    const uint32_t* node; int nNodes; int n;
    const uint8_t* skip;   // host, may be null
};

static void orbl_fill_kf(orbl::KfDev& D, const OrblKeyFrame& kf)
{
    memcpy(D.Rcw, kf.Rcw, sizeof D.Rcw); memcpy(D.tcw, kf.tcw, sizeof D.tcw); memcpy(D.Ow, kf.Ow, sizeof D.Ow);
    D.fx = kf.K[0]; D.fy = kf.K[1]; D.cx = kf.K[2]; D.cy = kf.K[3];
    D.invfx = 1.0f / kf.K[0]; D.invfy = 1.0f / kf.K[1];   // Frame.cc:93-94
}

static int orbl_core(orbm_handle* h, const OrblSide& A, const OrblKeyFrame* kf1, const std::vector<OrblSide>& B, const OrblKeyFrame* kf2,
                     const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                     OrblNewPoint* out, int capacity, int* n_new, uint8_t* status, float* f12_used)
{
    int rc;
    const int K = (int)B.size(), n1 = A.n;
    *n_new = 0;
    if (f12_used) memset(f12_used, 0, (size_t)K * 11 * sizeof(float));
    // the baseline gate (:244-260), F12 and the epipole per neighbour, the lock-step walk over node ids (ORBmatcher.cc:693-823)
    std::vector<orbl::KfDev> kd((size_t)K + 1);
    std::vector<orbl::Work> work;
    memset(kd.data(), 0, kd.size() * sizeof(orbl::KfDev));
    orbl_fill_kf(kd[0], *kf1);
    bool any = false;
    for (int k = 0; k < K; k++) {
        orbl::KfDev& D = kd[1 + k];
        orbl_fill_kf(D, kf2[k]);
        float vb[3];
        for (int c = 0; c < 3; c++) vb[c] = kf2[k].Ow[c] - kf1->Ow[c];
        const float baseline = (float)cvm::norm3(vb);
        const float ratioBaselineDepth = baseline / kf2[k].median_depth;
        D.gated = (double)ratioBaselineDepth < 0.01;
        if (D.gated) continue;
        any = true;
        float ep[2];
        (void)orbl_compute_f12(kf1, &kf2[k], D.F, ep);
        D.ex = ep[0]; D.ey = ep[1];
        if (f12_used) { memcpy(f12_used + (size_t)k * 11, D.F, 36); f12_used[(size_t)k * 11 + 9] = ep[0]; f12_used[(size_t)k * 11 + 10] = ep[1]; }
        if (n1 == 0 || B[k].n == 0) continue;
        int a = 0, b = 0;
        while (a < A.nNodes && b < B[k].nNodes) {
            if (A.node[a] == B[k].node[b]) { work.push_back({k, a, b, 0}); a++; b++; }
            else if (A.node[a] < B[k].node[b]) a++;
            else b++;
        }
    }
    if (K == 0 || n1 == 0) return ORBX_OK;
    const size_t cells = (size_t)K * n1;
    if (!any || work.empty()) {
        // nothing to search: the table is known on the host
        if (status)
            for (int k = 0; k < K; k++)
                for (int q = 0; q < n1; q++)
                    status[(size_t)k * n1 + q] = kd[1 + k].gated ? ORBL_ST_NEIGHBOUR_SKIPPED : (A.skip && A.skip[q]) ? ORBL_ST_FEATURE_SKIPPED : ORBL_ST_NO_MATCH;
        return ORBX_OK;
    }
    // the staging block: descriptors of the sides | work list | skip flags | (host arrays of the sides)
    Packer pk;
    const size_t oKf = pk.take(kd.size() * sizeof(orbl::KfDev)), oWork = pk.take(work.size() * sizeof(orbl::Work));
    std::vector<size_t> oSkip((size_t)K + 1, 0), oKeys((size_t)K + 1, 0), oDesc((size_t)K + 1, 0), oFs((size_t)K + 1, 0), oFi((size_t)K + 1, 0);
    auto side = [&](int s) -> const OrblSide& { return s == 0 ? A : B[(size_t)s - 1]; };
    for (int s = 0; s <= K; s++) {
        const OrblSide& S = side(s);
        if (s && kd[s].gated) continue;
        if (S.skip && S.n) oSkip[s] = pk.take((size_t)S.n);
        if (!S.dev && S.n && S.nNodes) {   // (a side without nodes takes part in no work item)
            oKeys[s] = pk.take((size_t)S.n * sizeof(OrbxKeyPoint));
            oDesc[s] = pk.take((size_t)S.n * 32);
            oFs[s] = pk.take((size_t)(S.nNodes + 1) * 4);
            oFi[s] = pk.take((size_t)std::max(S.fvStart[S.nNodes], 1) * 4);
        }
    }
    const size_t upBytes = pk.off;
    // the device block behind it: m12 | records | cnt | (total | out | status): the copy down
    const size_t oM12 = pk.take(cells * 4), oRec = pk.take(cells * sizeof(orbl::Rec)), oCnt = pk.take((size_t)K * 4);
    const size_t oDown = pk.take(16), oOut = pk.take((size_t)n1 * sizeof(orbl::Rec)), oStatus = pk.take(cells);
    const size_t downBytes = (status ? oStatus + ((cells + 15) & ~(size_t)15) : oStatus) - oDown;
    if ((rc = orbm_reserve(h, S_BLOCK, pk.off)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    for (int s = 0; s <= K; s++) {
        const OrblSide& S = side(s);
        orbl::KfDev& D = kd[s];
        D.n = S.n;
        if (s && D.gated) continue;
        if (S.skip && S.n) { memcpy(hs + oSkip[s], S.skip, (size_t)S.n); D.skip = d + oSkip[s]; }
        if (S.dev) { D.keys = (const orbm::KeyDev*)S.keys; D.desc = S.desc; D.fvStart = S.fvStart; D.fvIdx = S.fvIdx; }
        else if (S.n && S.nNodes) {
            memcpy(hs + oKeys[s], S.keys, (size_t)S.n * sizeof(OrbxKeyPoint));
            memcpy(hs + oDesc[s], S.desc, (size_t)S.n * 32);
            memcpy(hs + oFs[s], S.fvStart, (size_t)(S.nNodes + 1) * 4);
            if (S.fvStart[S.nNodes]) memcpy(hs + oFi[s], S.fvIdx, (size_t)S.fvStart[S.nNodes] * 4);
            D.keys = (const orbm::KeyDev*)(d + oKeys[s]); D.desc = d + oDesc[s];
            D.fvStart = (const int32_t*)(d + oFs[s]); D.fvIdx = (const int32_t*)(d + oFi[s]);
        }
    }
    memcpy(hs + oKf, kd.data(), kd.size() * sizeof(orbl::KfDev));
    memcpy(hs + oWork, work.data(), work.size() * sizeof(orbl::Work));
    orbl::Args a{};
    a.kf = (const orbl::KfDev*)(d + oKf); a.work = (const orbl::Work*)(d + oWork);
    a.nNeigh = K; a.n1 = n1; a.nWork = (int)work.size(); a.nlevels = nlevels;
    for (int i = 0; i < 16; i++) { a.sf[i] = i < nlevels ? scale_factors[i] : 0.f; a.sigma2[i] = i < nlevels ? level_sigma2[i] : 0.f; }
    a.ratioFactor = 1.5f * scale_factor;
    a.m12 = (int32_t*)(d + oM12); a.status = d + oStatus; a.rec = (orbl::Rec*)(d + oRec); a.cnt = (int32_t*)(d + oCnt);
    a.total = (int32_t*)(d + oDown); a.out = (orbl::Rec*)(d + oOut);
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(a.m12, 0xFF, cells * 4, s));
    // the queries of a node over `shares` workgroups: few work items (a coarse vocabulary level: large nodes) get many
    const int wantShares = (orbl::kSearchWavesWanted / orbl::kSearchWaves + a.nWork - 1) / a.nWork;
    const int shares = std::max(1, std::min({wantShares, orbl::kSearchMaxShares, (n1 + orbl::kSearchWaves - 1) / orbl::kSearchWaves}));
    hipLaunchKernelGGL(orbl::k_newpoints_search, dim3(a.nWork, shares), dim3(orbl::kSearchThreads), 0, s, a);
    hipLaunchKernelGGL(orbl::k_newpoints_triangulate, dim3((unsigned)((cells + orbl::kTriThreads - 1) / orbl::kTriThreads)), dim3(orbl::kTriThreads), 0, s, a);
    hipLaunchKernelGGL(orbl::k_newpoints_resolve, dim3((n1 + orbl::kRowThreads - 1) / orbl::kRowThreads), dim3(orbl::kRowThreads), 0, s, a);
    hipLaunchKernelGGL(orbl::k_newpoints_count, dim3(K), dim3(orbl::kRowThreads), 0, s, a);
    hipLaunchKernelGGL(orbl::k_newpoints_compact, dim3(K), dim3(orbl::kRowThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oDown, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int total = *(const int32_t*)hs;
    *n_new = total;
    if (total > capacity) return fail(ORBX_E_CAPACITY, "%d new points, room for %d", total, capacity);
    if (total) memcpy(out, hs + (oOut - oDown), (size_t)total * sizeof(OrblNewPoint));
    if (status) memcpy(status, hs + (oStatus - oDown), cells);
    return ORBX_OK;
}

static int orbl_check_common(const OrblKeyFrame* kf1, const OrblKeyFrame* kf2, int n_neighbours, const float* scale_factors, const float* level_sigma2,
                             int nlevels, int check_ori, OrblNewPoint* out, int capacity, int* n_new)
{
    if (!n_new) return fail(ORBX_E_INVALID, "null argument");
    *n_new = 0;
    // the orientation histogram would couple the queries of a neighbour (a pruned bin depends on every match), and with them
    // the neighbours through skip1: the batch is exact only without it, as the reference runs it (ORBmatcher(0.6, false))
    if (check_ori) return fail(ORBX_E_UNSUPPORTED, "check_ori: CreateNewMapPoints builds ORBmatcher(0.6, false); the histogram would couple the queries");
    if (n_neighbours < 0) return fail(ORBX_E_INVALID, "bad argument");
    if (n_neighbours > ORBL_MAX_NEIGHBOURS) return fail(ORBX_E_UNSUPPORTED, "%d neighbours: above %d", n_neighbours, ORBL_MAX_NEIGHBOURS);
    if (!kf1 || (n_neighbours && !kf2) || !scale_factors || !level_sigma2 || nlevels < 1 || nlevels > 16 || capacity < 0 || (capacity && !out))
        return fail(ORBX_E_INVALID, "bad argument");
    return ORBX_OK;
}

static int orbl_check_featvec(const OrbmFeatVec* fv, int n, const char* who, int k)
{
    if (!fv || fv->n_nodes < 0 || (fv->n_nodes && (!fv->node_id || !fv->start)) ) return fail(ORBX_E_INVALID, "%s %d: bad feature vector", who, k);
    if (fv->n_nodes == 0) return ORBX_OK;
    if (fv->start[0] != 0) return fail(ORBX_E_INVALID, "%s %d: feature vector does not start at 0", who, k);
    for (int i = 0; i < fv->n_nodes; i++) {
        if (fv->start[i + 1] < fv->start[i]) return fail(ORBX_E_INVALID, "%s %d: feature vector starts descend", who, k);
        if (i && fv->node_id[i] <= fv->node_id[i - 1]) return fail(ORBX_E_INVALID, "%s %d: node ids do not ascend", who, k);
    }
    const int ni = fv->start[fv->n_nodes];
    if (ni && !fv->idx) return fail(ORBX_E_INVALID, "%s %d: bad feature vector", who, k);
    for (int i = 0; i < ni; i++) if (fv->idx[i] < 0 || fv->idx[i] >= n) return fail(ORBX_E_INVALID, "%s %d: feature index out of range", who, k);
    return ORBX_OK;
}

extern "C" int orbl_create_new_map_points(orbm_t* h, const OrbxKeyPoint* keys1, const uint8_t* desc1, int n1, const OrbmFeatVec* fv1,
                                          const uint8_t* skip1, const OrblKeyFrame* kf1, const OrbxKeyPoint* const* keys2,
                                          const uint8_t* const* desc2, const int32_t* n2, const OrbmFeatVec* fv2, const uint8_t* const* skip2,
                                          const OrblKeyFrame* kf2, int n_neighbours, const float* scale_factors, const float* level_sigma2,
                                          int nlevels, float scale_factor, int check_ori, OrblNewPoint* out, int capacity, int* n_new,
                                          uint8_t* status, float* f12_used)
{
    int rc = orbl_check_common(kf1, kf2, n_neighbours, scale_factors, level_sigma2, nlevels, check_ori, out, capacity, n_new);
    if (rc || (rc = orbm_check(h))) return rc;
    if (n1 < 0 || n1 > 65535 || (n1 && (!keys1 || !desc1)) || (n_neighbours && (!keys2 || !desc2 || !n2 || !fv2))) return fail(ORBX_E_INVALID, "bad argument");
    if ((rc = orbl_check_featvec(fv1, n1, "current keyframe", 0))) return rc;
    const OrblSide A = {false, keys1, desc1, fv1->start, fv1->idx, fv1->node_id, fv1->n_nodes, n1, skip1};
    std::vector<OrblSide> B((size_t)n_neighbours);
    for (int k = 0; k < n_neighbours; k++) {
        if (n2[k] < 0 || n2[k] > 65535 || (n2[k] && (!keys2[k] || !desc2[k]))) return fail(ORBX_E_INVALID, "neighbour %d: bad argument", k);
        if ((rc = orbl_check_featvec(&fv2[k], n2[k], "neighbour", k))) return rc;
        B[k] = {false, keys2[k], desc2[k], fv2[k].start, fv2[k].idx, fv2[k].node_id, fv2[k].n_nodes, n2[k], skip2 ? skip2[k] : nullptr};
    }
    return orbl_core(h, A, kf1, B, kf2, scale_factors, level_sigma2, nlevels, scale_factor, out, capacity, n_new, status, f12_used);
}

extern "C" int orbl_create_new_map_points_frames(orbm_t* h, orbm_frame_t* f1, const uint8_t* skip1, const OrblKeyFrame* kf1,
                                                 orbm_frame_t* const* f2, const uint8_t* const* skip2, const OrblKeyFrame* kf2, int n_neighbours,
                                                 const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                                                 int check_ori, OrblNewPoint* out, int capacity, int* n_new, uint8_t* status, float* f12_used)
{
    int rc = orbl_check_common(kf1, kf2, n_neighbours, scale_factors, level_sigma2, nlevels, check_ori, out, capacity, n_new);
    if (rc || (rc = orbm_check(h))) return rc;
    if (!f1 || (n_neighbours && !f2)) return fail(ORBX_E_INVALID, "null frame");
    if ((rc = frame_usable(h, f1))) return rc;
    if (f1->n > 65535) return fail(ORBX_E_INVALID, "%d features in the current keyframe: above 65535", f1->n);
    if (!f1->hasBow) return fail(ORBX_E_INVALID, "orbm_frame_compute_bow has not run on the current keyframe");
    const OrblSide A = {true, f1->d_keysUn, f1->d_desc, f1->d_fvStart, f1->d_fvIdx, f1->fvNode.data(), f1->fvNodes, f1->n, skip1};
    std::vector<OrblSide> B((size_t)n_neighbours);
    for (int k = 0; k < n_neighbours; k++) {
        orbm_frame* f = f2[k];
        if ((rc = frame_usable(h, f))) return rc;
        // the exactness argument needs distinct keyframes: a neighbour's AddMapPoint must touch no other search
        if (f == f1) return fail(ORBX_E_INVALID, "neighbour %d is the current keyframe", k);
        for (int e = 0; e < k; e++) if (f2[e] == f) return fail(ORBX_E_INVALID, "neighbour %d repeats neighbour %d", k, e);
        if (f->n > 65535) return fail(ORBX_E_INVALID, "%d features in neighbour %d: above 65535", f->n, k);
        if (!f->hasBow) return fail(ORBX_E_INVALID, "orbm_frame_compute_bow has not run on neighbour %d", k);
        B[k] = {true, f->d_keysUn, f->d_desc, f->d_fvStart, f->d_fvIdx, f->fvNode.data(), f->fvNodes, f->n, skip2 ? skip2[k] : nullptr};
    }
    return orbl_core(h, A, kf1, B, kf2, scale_factors, level_sigma2, nlevels, scale_factor, out, capacity, n_new, status, f12_used);
}

// ------------------------------------------------------------------ SearchInNeighbors: the batched Fuse (DESIGN.md §8l)
// One call = the checks, the job list cut into tiles, the staging of orbf_host.inc (host arrays: every distinct target's
// grid built on the host), one packed upload, one launch, one copy down, one synchronise.
static_assert(sizeof(OrblFuseResult) == 20 && sizeof(OrblFuseResult) == sizeof(orbl::FuseRes), "OrblFuseResult layout");

static int orbl_predict_float(float ratio, float log_scale_factor) { return (int)std::ceil(std::log(ratio) / log_scale_factor); }

extern "C" int orbl_level_breaks(float log_scale_factor, int nlevels, orbl_predict_fn predict, float* out)
{
    if (!out || nlevels < 1 || nlevels > 16 || !(log_scale_factor > 0.f) || !std::isfinite(log_scale_factor))
        return fail(ORBX_E_INVALID, "bad argument");
    if (!predict) predict = orbl_predict_float;
    auto asFloat = [](uint32_t b) { float f; memcpy(&f, &b, 4); return f; };
    // positive finite floats order as their bit patterns; the level is a monotone step function of the ratio (checked over
    // every float of [2^-8, 2^12] by tests/test_fuse_cpu.py): the largest pattern whose level is <= L
    const uint32_t lo0 = 0x00000001u, hi0 = 0x7F7FFFFFu;
    for (int L = -1; L < nlevels; L++) {
        if (predict(asFloat(lo0), log_scale_factor) > L || predict(asFloat(hi0), log_scale_factor) <= L)
            return fail(ORBX_E_INVALID, "level %d has no break among the positive floats", L);
        uint32_t lo = lo0, hi = hi0;   // level(lo) <= L < level(hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (predict(asFloat(mid), log_scale_factor) <= L) lo = mid; else hi = mid;
        }
        out[L + 1] = asFloat(lo);
    }
    for (int j = 0; j < nlevels; j++)
        if (!(out[j] < out[j + 1])) return fail(ORBX_E_INVALID, "the predicted level is not a monotone function of the ratio");
    return ORBX_OK;
}

static int orbl_fuse_check(orbm_handle* h, const OrblFuseTarget* targets, int n_targets, const OrblFusePoint* points, int n_points,
                           const int32_t* job_start, const int32_t* job_point, const float* scale_factors, const float* inv_level_sigma2,
                           int nlevels, const float* level_breaks, OrblFuseResult* out, int64_t* n_jobs)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    *n_jobs = 0;
    if (n_targets < 0 || n_points < 0) return fail(ORBX_E_INVALID, "bad argument");
    if (n_targets > ORBL_FUSE_MAX_TARGETS) return fail(ORBX_E_UNSUPPORTED, "%d targets: above %d", n_targets, ORBL_FUSE_MAX_TARGETS);
    if (n_targets == 0) return ORBX_OK;
    if (!targets || !job_start || !scale_factors || !inv_level_sigma2 || !level_breaks || nlevels < 1 || nlevels > 16)
        return fail(ORBX_E_INVALID, "bad argument");
    if (job_start[0] != 0) return fail(ORBX_E_INVALID, "job_start does not start at 0");
    for (int k = 0; k < n_targets; k++)
        if (job_start[k + 1] < job_start[k]) return fail(ORBX_E_INVALID, "job_start descends at target %d", k);
    const int64_t J = job_start[n_targets];
    if (J > ORBL_FUSE_MAX_JOBS) return fail(ORBX_E_UNSUPPORTED, "%lld job entries: above %d", (long long)J, ORBL_FUSE_MAX_JOBS);
    if ((rc = orbf_check_breaks(level_breaks, nlevels))) return rc;
    if (J == 0) return ORBX_OK;
    if (!job_point || !points || !out) return fail(ORBX_E_INVALID, "bad argument");
    for (int64_t i = 0; i < J; i++)
        if (job_point[i] < 0 || job_point[i] >= n_points) return fail(ORBX_E_INVALID, "job entry %lld: point %d outside the pool of %d", (long long)i, job_point[i], n_points);
    *n_jobs = J;
    return ORBX_OK;
}

static int orbl_fuse_core(orbm_handle* h, const OrblFuseTarget* targets, const std::vector<OrbfSide>& sides, const OrblFusePoint* points,
                          int n_points, const int32_t* job_start, const int32_t* job_point, int64_t J, float th, const float* scale_factors,
                          const float* inv_level_sigma2, int nlevels, const float* level_breaks, OrblFuseResult* out)
{
    int rc;
    const int T = (int)sides.size();
    std::vector<orbl::FuseWork> work;
    for (int k = 0; k < T; k++)
        for (int b = job_start[k]; b < job_start[k + 1]; b += orbl::kFuseTile)
            work.push_back({k, b, std::min(orbl::kFuseTile, job_start[k + 1] - b), 0});
    // the staging block: orbf's head (target records | points | host arrays of the targets) | job list | tiles
    Packer pk;
    OrbfStage st;
    orbf_stage_take(pk, sides, n_points, st);
    const size_t oJob = pk.take((size_t)J * 4), oWork = pk.take(work.size() * sizeof(orbl::FuseWork));
    const size_t upBytes = pk.off;
    const size_t oOut = pk.take((size_t)J * sizeof(orbl::FuseRes));
    const size_t downBytes = (size_t)J * sizeof(orbl::FuseRes);
    if ((rc = orbm_reserve(h, S_BLOCK, pk.off)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orbf_stage_fill(hs, d, st, targets, sides, points, n_points);
    memcpy(hs + oJob, job_point, (size_t)J * 4);
    memcpy(hs + oWork, work.data(), work.size() * sizeof(orbl::FuseWork));
    orbl::FuseArgs a{};
    a.tgt = (const orbf::FuseTgt*)(d + st.tgt); a.pts = (const orbf::FusePt*)(d + st.pts); a.jobPoint = (const int32_t*)(d + oJob);
    a.work = (const orbl::FuseWork*)(d + oWork); a.out = (orbl::FuseRes*)(d + oOut);
    a.th = th; a.nlevels = nlevels;
    orbf_fill_tables(scale_factors, level_breaks, nlevels, a.sf, a.breaks);
    for (int i = 0; i < 16; i++) a.invSigma2[i] = i < nlevels ? inv_level_sigma2[i] : 0.f;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(orbl::k_fuse_batch, dim3((unsigned)work.size()), dim3(orbl::kFuseThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oOut, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out, hs, downBytes);
    return ORBX_OK;
}

extern "C" int orbl_fuse_batch(orbm_t* h, const OrblFuseTarget* targets, const OrbxKeyPoint* const* keys_un, const uint8_t* const* desc,
                               const int32_t* n, int n_targets, const OrblFusePoint* points, int n_points, const int32_t* job_start,
                               const int32_t* job_point, float th, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                               const float* level_breaks, OrblFuseResult* out)
{
    int64_t J;
    int rc = orbl_fuse_check(h, targets, n_targets, points, n_points, job_start, job_point, scale_factors, inv_level_sigma2, nlevels, level_breaks, out, &J);
    if (rc || n_targets == 0) return rc;
    std::vector<OrbfSide> sides;
    if ((rc = orbf_sides_host(targets, keys_un, desc, n, n_targets, sides)) || J == 0) return rc;
    return orbl_fuse_core(h, targets, sides, points, n_points, job_start, job_point, J, th, scale_factors, inv_level_sigma2, nlevels, level_breaks, out);
}

extern "C" int orbl_fuse_batch_frames(orbm_t* h, const OrblFuseTarget* targets, orbm_frame_t* const* frames, int n_targets,
                                      const OrblFusePoint* points, int n_points, const int32_t* job_start, const int32_t* job_point, float th,
                                      const float* scale_factors, const float* inv_level_sigma2, int nlevels, const float* level_breaks,
                                      OrblFuseResult* out)
{
    int64_t J;
    int rc = orbl_fuse_check(h, targets, n_targets, points, n_points, job_start, job_point, scale_factors, inv_level_sigma2, nlevels, level_breaks, out, &J);
    if (rc || n_targets == 0) return rc;
    if (!frames) return fail(ORBX_E_INVALID, "null frame");
    std::vector<OrbfSide> sides;
    if ((rc = orbf_sides_frames(h, frames, n_targets, sides)) || J == 0) return rc;
    return orbl_fuse_core(h, targets, sides, points, n_points, job_start, job_point, J, th, scale_factors, inv_level_sigma2, nlevels, level_breaks, out);
}
