// orbi_host.inc -- host side of the device Initializer (part of orbslamm_hip.hip; kernels: orbi_kernels.hip, DESIGN.md §8h).
// Glue around one chain per call: the argument checks (which read every match and set index anyway, so vMatches12 is
// compacted here), one packed upload, the launches, one copy down, and the last comparisons of ReconstructF /
// ReconstructH, which need acosf of one value per candidate.

struct orbi_init : orbm_solver_base {    // (h_stage: the upload, then the results)
    int model = ORBI_MODEL_HF, iters = 0, n1 = 0;
    float K[4] = {0.f, 0.f, 0.f, 0.f};
    float sigma = 1.f;
    orbi::Key* d_keys1 = nullptr;        // mvKeys1 (n1) ...
    orbi::Norm* d_norm = nullptr;        // ... behind it: Normalize of frame 1 (cached) and frame 2 (per call)
    orbi::Norm norm1{};
    std::vector<orbi::Pair> pairs;
};

static void orbi_free(orbi_init* ini)
{
    if (!ini) return;
    ini->release({ini->d_keys1});
    delete ini;
}

extern "C" void orbi_destroy(orbi_t* ini) { orbi_free(ini); }

static int orbi_make(orbm_handle* h, const OrbxKeyPoint* hkeys, orbm_frame* f1, int n1, const float K[4], float sigma, int iterations,
                     int model, orbi_init** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!K || n1 < 0 || (n1 && !hkeys && !f1)) return fail(ORBX_E_INVALID, "bad argument");
    if (model != ORBI_MODEL_HF && model != ORBI_MODEL_F) return fail(ORBX_E_INVALID, "unknown model %d", model);
    if (iterations < 1) return fail(ORBX_E_INVALID, "iterations %d < 1", iterations);
    if (iterations > ORBI_MAX_ITERATIONS) return fail(ORBX_E_UNSUPPORTED, "iterations %d above %d", iterations, ORBI_MAX_ITERATIONS);
    if (n1 > ORBI_MAX_FEATURES) return fail(ORBX_E_UNSUPPORTED, "%d keys in frame 1: above %d", n1, ORBI_MAX_FEATURES);
    orbi_init* ini = new orbi_init();
    ini->attach(h);
    ini->model = model; ini->iters = iterations; ini->n1 = n1; ini->sigma = sigma;
    for (int k = 0; k < 4; k++) ini->K[k] = K[k];
    const size_t keyBytes = ((size_t)std::max(n1, 1) * sizeof(orbi::Key) + 255) & ~(size_t)255;
    HIPCHK_OR(hipMalloc((void**)&ini->d_keys1, keyBytes + 2 * sizeof(orbi::Norm)), orbi_free(ini));
    ini->d_norm = (orbi::Norm*)((uint8_t*)ini->d_keys1 + keyBytes);
    if (n1) {
        if (f1) HIPCHK_OR(hipMemcpyAsync(ini->d_keys1, f1->d_keysUn, (size_t)n1 * sizeof(orbi::Key), hipMemcpyDeviceToDevice, h->stream), orbi_free(ini));
        else HIPCHK_OR(hipMemcpyAsync(ini->d_keys1, hkeys, (size_t)n1 * sizeof(orbi::Key), hipMemcpyHostToDevice, h->stream), orbi_free(ini));
        hipLaunchKernelGGL(orbi::k_init_normalize, dim3(1), dim3(orbi::kNormThreads), 0, h->stream, ini->d_keys1, n1, ini->d_keys1, n1, ini->d_norm);
        HIPCHK_OR(hipGetLastError(), orbi_free(ini));
        HIPCHK_OR(hipMemcpyAsync(&ini->norm1, ini->d_norm, sizeof(orbi::Norm), hipMemcpyDeviceToHost, h->stream), orbi_free(ini));
    }
    HIPCHK_OR(hipStreamSynchronize(h->stream), orbi_free(ini));
    *out = ini;
    return ORBX_OK;
}

extern "C" int orbi_create(orbm_t* h, const OrbxKeyPoint* keys1_un, int n1, const float K[4], float sigma, int iterations, int model, orbi_t** out)
{
    return orbi_make(h, keys1_un, nullptr, n1, K, sigma, iterations, model, out);
}

extern "C" int orbi_create_frame(orbm_t* h, orbm_frame_t* f1, const float K[4], float sigma, int iterations, int model, orbi_t** out)
{
    if (!h || !f1 || !out) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbm_check(h);
    if (rc || (rc = frame_usable(h, f1))) return rc;
    return orbi_make(h, nullptr, f1, f1->n, K, sigma, iterations, model, out);
}

extern "C" int orbi_size(orbi_t* ini, int* n1)
{
    if (!ini || !n1) return fail(ORBX_E_INVALID, "null argument");
    *n1 = ini->n1;
    return ORBX_OK;
}

extern "C" int orbi_normalization(orbi_t* ini, float out[4])
{
    if (!ini || !out) return fail(ORBX_E_INVALID, "null argument");
    out[0] = ini->norm1.meanX; out[1] = ini->norm1.meanY; out[2] = ini->norm1.sX; out[3] = ini->norm1.sY;
    return ORBX_OK;
}

static int orbi_run(orbi_init* ini, const OrbxKeyPoint* hkeys2, const orbi::Key* dkeys2, int n2, const int32_t* matches12, const int32_t* sets,
                    OrbiResult* res, float* p3d, uint8_t* tri)
{
    orbm_handle* h = ini->h;
    int rc = orbm_check(h);
    if (rc) return rc;
    const int n1 = ini->n1, iters = ini->iters;
    const bool hf = ini->model == ORBI_MODEL_HF;
    if (!sets || !res || (n1 && (!matches12 || !p3d || !tri)) || n2 < 0 || (n2 && !hkeys2 && !dkeys2)) return fail(ORBX_E_INVALID, "bad argument");
    if (n2 > ORBI_MAX_FEATURES) return fail(ORBX_E_UNSUPPORTED, "%d keys in frame 2: above %d", n2, ORBI_MAX_FEATURES);
    // mvMatches12 (Initializer.cc:51-63)
    std::vector<orbi::Pair>& pairs = ini->pairs;
    pairs.clear();
    for (int i = 0; i < n1; i++) {
        const int32_t m = matches12[i];
        if (m < 0) continue;
        if (m >= n2) return fail(ORBX_E_INVALID, "matches12[%d] = %d: frame 2 has %d keys", i, m, n2);
        pairs.push_back(orbi::Pair{i, m});
    }
    const int N = (int)pairs.size();
    if (N < 8) return fail(ORBX_E_UNSUPPORTED, "%d matches: the 8-point sets need at least 8", N);
    for (int k = 0; k < iters * 8; k++)
        if (sets[k] < 0 || sets[k] >= N) return fail(ORBX_E_INVALID, "sets[%d] = %d outside [0, %d)", k, sets[k], N);

    Packer pk;
    const size_t oKeys2 = pk.take(hkeys2 ? (size_t)n2 * sizeof(orbi::Key) : 0), oPairs = pk.take((size_t)N * sizeof(orbi::Pair)),
                 oSets = pk.take((size_t)iters * 8 * 4), upBytes = pk.off;
    const size_t oHypF = pk.take((size_t)iters * 9 * 4), oHypH = pk.take(hf ? (size_t)iters * 18 * 4 : 0), oScF = pk.take((size_t)iters * 4),
                 oScH = pk.take(hf ? (size_t)iters * 4 : 0), oRec = pk.take((size_t)8 * N * sizeof(float4)), oFlag = pk.take((size_t)8 * N);
    const size_t oHdr = pk.take(sizeof(orbi::Hdr)), oP3D = pk.take((size_t)n1 * 12), oTri = pk.take((size_t)n1), total = pk.off;
    const size_t downBytes = total - oHdr;
    if ((rc = ini->reserve(total, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = ini->h_stage;
    uint8_t* d = (uint8_t*)ini->d_work;
    if (hkeys2 && n2) memcpy(hs + oKeys2, hkeys2, (size_t)n2 * sizeof(orbi::Key));
    memcpy(hs + oPairs, pairs.data(), (size_t)N * sizeof(orbi::Pair));
    memcpy(hs + oSets, sets, (size_t)iters * 8 * 4);
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d + oHdr, 0, sizeof(orbi::Hdr), s));
    const orbi::Key* k1 = ini->d_keys1;
    const orbi::Key* k2 = hkeys2 ? (const orbi::Key*)(d + oKeys2) : dkeys2;
    const orbi::Pair* dp = (const orbi::Pair*)(d + oPairs);
    const int32_t* ds = (const int32_t*)(d + oSets);
    float *hypF = (float*)(d + oHypF), *hypH = (float*)(d + oHypH), *scF = (float*)(d + oScF), *scH = (float*)(d + oScH);
    orbi::Hdr* hdr = (orbi::Hdr*)(d + oHdr);
    const float* K = ini->K;
    hipLaunchKernelGGL(orbi::k_init_normalize, dim3(1), dim3(orbi::kNormThreads), 0, s, k2, n2, k2, n2, ini->d_norm + 1);
    const int fitBlocks = (iters + orbi::kFitThreads - 1) / orbi::kFitThreads;
    hipLaunchKernelGGL(orbi::k_init_fit<false>, dim3(fitBlocks), dim3(orbi::kFitThreads), 0, s, k1, k2, ini->d_norm, dp, ds, iters, hypF);
    if (hf) hipLaunchKernelGGL(orbi::k_init_fit<true>, dim3(fitBlocks), dim3(orbi::kFitThreads), 0, s, k1, k2, ini->d_norm, dp, ds, iters, hypH);
    hipLaunchKernelGGL(orbi::k_init_score<false>, dim3(iters), dim3(orbi::kScoreThreads), 0, s, k1, k2, dp, N, (const float*)hypF, ini->sigma, scF);
    if (hf) hipLaunchKernelGGL(orbi::k_init_score<true>, dim3(iters), dim3(orbi::kScoreThreads), 0, s, k1, k2, dp, N, (const float*)hypH, ini->sigma, scH);
    hipLaunchKernelGGL(orbi::k_init_pick, dim3(1), dim3(64), 0, s, (const float*)hypF, (const float*)scF, (const float*)hypH, (const float*)scH,
                       iters, (int)hf, K[0], K[1], K[2], K[3], hdr);
    hipLaunchKernelGGL(orbi::k_init_checkrt, dim3((N + orbi::kRtThreads - 1) / orbi::kRtThreads, 8), dim3(orbi::kRtThreads), 0, s, k1, k2, dp, N,
                       K[0], K[1], K[2], K[3], ini->sigma, (int)hf, hdr, (float4*)(d + oRec), (uint8_t*)(d + oFlag));
    hipLaunchKernelGGL(orbi::k_init_winner, dim3(1), dim3(orbi::kWinThreads), 0, s, hdr, N, n1, dp, (const float4*)(d + oRec),
                       (const uint8_t*)(d + oFlag), (float*)(d + oP3D), (uint8_t*)(d + oTri));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oHdr, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));

    // ReconstructF's / ReconstructH's last comparisons (:514-584, :704-746)
    const orbi::Hdr& H = *(const orbi::Hdr*)hs;
    OrbiResult r;
    memset(&r, 0, sizeof r);
    r.reconstructed_h = H.reconH;
    r.SH = H.SH; r.SF = H.SF; r.RH = H.RH;
    for (int k = 0; k < 9; k++) { r.H21[k] = H.H21[k]; r.F21[k] = H.F21[k]; }
    r.it_H = H.itH; r.it_F = H.itF;
    r.inliers_H = H.nInliersH; r.inliers_F = H.nInliersF;
    r.n_matches = N;
    r.n_inliers = H.nInliers;
    r.n_candidates = H.nCand;
    r.best = H.nCand ? H.best : -1;
    for (int c = 0; c < H.nCand; c++) {
        r.n_good[c] = H.nGood[c];
        // CheckRT (:911-919): acos of the float is acosf (`using namespace std`), then *180 in float, /CV_PI in double
        r.parallax[c] = H.nGood[c] > 0 ? (float)((double)(std::acos(H.kthCos[c]) * 180) / 3.1415926535897932384626433832795) : 0.f;
    }
    bool ok = false;
    if (H.nCand == 4) {
        const int maxGood = std::max(std::max(r.n_good[0], r.n_good[1]), std::max(r.n_good[2], r.n_good[3]));
        const int nMinGood = std::max(static_cast<int>(0.9 * r.n_inliers), 50);
        int nsimilar = 0;
        for (int c = 0; c < 4; c++) if (r.n_good[c] > 0.7 * maxGood) nsimilar++;
        r.rt_state = 1;
        ok = !(maxGood < nMinGood || nsimilar > 1) && r.parallax[r.best] > 1.0f;
    } else if (H.nCand == 8) {
        int bestGood = 0, secondBestGood = 0;
        float bestParallax = -1;
        for (int c = 0; c < 8; c++) {
            if (r.n_good[c] > bestGood) { secondBestGood = bestGood; bestGood = r.n_good[c]; bestParallax = r.parallax[c]; }
            else if (r.n_good[c] > secondBestGood) secondBestGood = r.n_good[c];
        }
        ok = secondBestGood < 0.75 * bestGood && bestParallax >= 1.0f && bestGood > 50 && bestGood > 0.9 * r.n_inliers;
    }
    if (ok) {
        r.rt_state = 2;
        for (int k = 0; k < 9; k++) r.R21[k] = H.R[r.best][k];
        for (int k = 0; k < 3; k++) r.t21[k] = H.t[r.best][k];
        memcpy(p3d, hs + (oP3D - oHdr), (size_t)n1 * 12);
        memcpy(tri, hs + (oTri - oHdr), (size_t)n1);
    }
    r.ok = ok;
    *res = r;
    return ORBX_OK;
}

extern "C" int orbi_initialize(orbi_t* ini, const OrbxKeyPoint* keys2_un, int n2, const int32_t* matches12, const int32_t* sets,
                               OrbiResult* res, float* p3d, uint8_t* triangulated)
{
    if (!ini || (n2 && !keys2_un)) return fail(ORBX_E_INVALID, "null argument");
    return orbi_run(ini, keys2_un, nullptr, n2, matches12, sets, res, p3d, triangulated);
}

extern "C" int orbi_initialize_frame(orbi_t* ini, orbm_frame_t* f2, const int32_t* matches12, const int32_t* sets,
                                     OrbiResult* res, float* p3d, uint8_t* triangulated)
{
    if (!ini || !f2) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbm_check(ini->h);
    if (rc || (rc = frame_usable(ini->h, f2))) return rc;
    return orbi_run(ini, nullptr, (const orbi::Key*)f2->d_keysUn, f2->n, matches12, sets, res, p3d, triangulated);
}
