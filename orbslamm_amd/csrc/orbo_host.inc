// orbo_host.inc -- host side of the device PoseOptimization (part of orbslamm_hip.hip; kernel: orbo_kernels.hip, ABI:
// include/orbslamm_poseopt.h, DESIGN.md §8o).  One call = the checks, one packed upload (frame records | edges | with host
// arrays the edges' observations), ONE launch for all frames, one copy of the results and the outlier bytes down, one
// synchronise.

static_assert(sizeof(OrboFrame) == 80 && sizeof(OrboEdge) == 16 && sizeof(OrboResult) == 176, "orbslamm_poseopt.h layouts");
static_assert(orbo::kMaxEdges == ORBO_MAX_EDGES && orbo::kMaxFrames == ORBO_MAX_FRAMES, "orbo limits");
static_assert(ORBO_MAX_CALL_EDGES < INT32_MAX / 64, "a call's edge total and its byte offsets per edge stay small");

// what needs neither the handle nor a GPU.  Zero frames are settled by the callers before this: ORBX_OK, nothing read
static int orbo_check_args(const OrboFrame* frames, int n_frames, const int32_t* edge_start, const OrboEdge* edges, const float* inv_level_sigma2,
                           int nlevels, const OrboResult* out, const uint8_t* outlier)
{
    if (n_frames < 0) return fail(ORBX_E_INVALID, "negative frame count");
    if (n_frames > ORBO_MAX_FRAMES) return fail(ORBX_E_UNSUPPORTED, "%d frames: above %d", n_frames, ORBO_MAX_FRAMES);
    if (!inv_level_sigma2 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d] or no sigma table", nlevels, ORBX_MAX_LEVELS);
    if (!edge_start) return fail(ORBX_E_INVALID, "null edge_start");
    if (edge_start[0] != 0) return fail(ORBX_E_INVALID, "edge_start[0] = %d: it starts at 0", edge_start[0]);
    for (int f = 0; f < n_frames; f++) {
        if (edge_start[f + 1] < edge_start[f]) return fail(ORBX_E_INVALID, "edge_start descends at frame %d", f);
        if (edge_start[f + 1] - edge_start[f] > ORBO_MAX_EDGES)
            return fail(ORBX_E_UNSUPPORTED, "%d edges in frame %d: above %d", edge_start[f + 1] - edge_start[f], f, ORBO_MAX_EDGES);
        if (edge_start[f + 1] > ORBO_MAX_CALL_EDGES)
            return fail(ORBX_E_UNSUPPORTED, "more than %d edges in one call (reached at frame %d)", ORBO_MAX_CALL_EDGES, f);
    }
    if (n_frames && (!frames || !out)) return fail(ORBX_E_INVALID, "null argument");
    if (edge_start[n_frames] && (!edges || !outlier)) return fail(ORBX_E_INVALID, "null argument");
    return ORBX_OK;
}

// resident: the frames' device keys, or null: obs holds every edge's observation
static int orbo_core(orbm_handle* h, const OrboFrame* frames, orbm_frame* const* resident, const std::vector<orbo::Obs>& obs, int n_frames,
                     const int32_t* edge_start, const OrboEdge* edges, const float* inv_level_sigma2, int nlevels, OrboResult* out, uint8_t* outlier)
{
    int rc;
    const size_t total = (size_t)edge_start[n_frames];
    Packer pk;
    const size_t oFrames = pk.take((size_t)n_frames * sizeof(orbo::FrameIn)), oEdges = pk.take(total * sizeof(OrboEdge)),
                 oObs = pk.take(obs.size() * sizeof(orbo::Obs)), upBytes = pk.off;
    const size_t oPw = pk.take(total * sizeof(float4)), oUv = pk.take(total * sizeof(float2));
    const size_t oOut = pk.take((size_t)n_frames * sizeof(OrboResult)), oFlags = pk.take(total), work = pk.off;
    const size_t downBytes = work - oOut;
    if ((rc = orbm_reserve(h, S_BLOCK, work)) || (rc = orbm_pinned(h, std::max(upBytes, downBytes)))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    orbo::FrameIn* hf = (orbo::FrameIn*)(hs + oFrames);
    for (int f = 0; f < n_frames; f++) {
        memcpy(hf[f].Tcw, frames[f].Tcw, sizeof hf[f].Tcw);
        memcpy(hf[f].K, frames[f].K, sizeof hf[f].K);
        hf[f].keys = resident ? resident[f]->d_keysUn : nullptr;
        hf[f].nKeys = resident ? resident[f]->n : 0;
        hf[f].e0 = edge_start[f]; hf[f].n = edge_start[f + 1] - edge_start[f]; hf[f].pad = 0;
    }
    if (total) memcpy(hs + oEdges, edges, total * sizeof(OrboEdge));
    if (!obs.empty()) memcpy(hs + oObs, obs.data(), obs.size() * sizeof(orbo::Obs));
    orbo::Args a{};
    a.frames = (const orbo::FrameIn*)(d + oFrames); a.edges = (const OrboEdge*)(d + oEdges); a.obs = (const orbo::Obs*)(d + oObs);
    a.pw = (float4*)(d + oPw); a.uv = (float2*)(d + oUv); a.out = (OrboResult*)(d + oOut); a.outlier = d + oFlags;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.invSigma2[l] = l < nlevels ? inv_level_sigma2[l] : 0.f;
    a.nlevels = nlevels;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d + oOut, 0, (size_t)n_frames * sizeof(OrboResult), s));   // (the records' padding word too: the same bytes every call)
    hipLaunchKernelGGL(orbo::k_pose_optimize, dim3((unsigned)n_frames), dim3(orbo::kLanes), 0, s, a, n_frames);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, d + oOut, downBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const OrboResult* hr = (const OrboResult*)hs;
    for (int f = 0; f < n_frames; f++)
        if (hr[f].rounds < 0) return fail(ORBX_E_INVALID, "frame %d: an edge's octave lies outside [0, %d)", f, nlevels);
    memcpy(out, hr, (size_t)n_frames * sizeof(OrboResult));
    if (total) memcpy(outlier, hs + (oFlags - oOut), total);
    return ORBX_OK;
}

extern "C" int orbo_pose_optimize(orbm_t* h, const OrboFrame* frames, const OrbxKeyPoint* const* keys_un, const int32_t* n_keys, int n_frames,
                                  const int32_t* edge_start, const OrboEdge* edges, const float* inv_level_sigma2, int nlevels, OrboResult* out,
                                  uint8_t* outlier)
{
    if (n_frames == 0) return ORBX_OK;   // nothing to do: no argument is read, no handle needed
    int rc = orbo_check_args(frames, n_frames, edge_start, edges, inv_level_sigma2, nlevels, out, outlier);
    if (rc) return rc;
    if (!keys_un || !n_keys) return fail(ORBX_E_INVALID, "null key arrays");
    // the pointer chasing of :302-341 for the observation: mvKeysUn[feature]
    std::vector<orbo::Obs> obs;
    try { obs.resize((size_t)edge_start[n_frames]); }
    catch (const std::bad_alloc&) { return fail(ORBX_E_CAPACITY, "no host memory for the observations of %d edges", edge_start[n_frames]); }
    for (int f = 0; f < n_frames; f++) {
        if (n_keys[f] < 0 || (n_keys[f] && !keys_un[f])) return fail(ORBX_E_INVALID, "frame %d: bad key array", f);
        for (int e = edge_start[f]; e < edge_start[f + 1]; e++) {
            const int i = edges[e].feature;
            if (i < 0 || i >= n_keys[f]) return fail(ORBX_E_INVALID, "edge %d: feature %d outside frame %d's [0, %d)", e, i, f, n_keys[f]);
            const OrbxKeyPoint& kp = keys_un[f][i];
            if (kp.octave < 0 || kp.octave >= nlevels) return fail(ORBX_E_INVALID, "edge %d: octave %d outside [0, %d)", e, kp.octave, nlevels);
            obs[(size_t)e] = orbo::Obs{kp.x, kp.y, kp.octave};
        }
    }
    if ((rc = orbm_check(h))) return rc;
    return orbo_core(h, frames, nullptr, obs, n_frames, edge_start, edges, inv_level_sigma2, nlevels, out, outlier);
}

extern "C" int orbo_pose_optimize_frames(orbm_t* h, const OrboFrame* frames, orbm_frame_t* const* resident, int n_frames, const int32_t* edge_start,
                                         const OrboEdge* edges, const float* inv_level_sigma2, int nlevels, OrboResult* out, uint8_t* outlier)
{
    if (n_frames == 0) return ORBX_OK;
    int rc = orbo_check_args(frames, n_frames, edge_start, edges, inv_level_sigma2, nlevels, out, outlier);
    if (rc) return rc;
    if (!resident) return fail(ORBX_E_INVALID, "null frame");
    for (int f = 0; f < n_frames; f++) {
        if (!resident[f] || !resident[f]->owner) return fail(ORBX_E_INVALID, "null frame");
        for (int e = edge_start[f]; e < edge_start[f + 1]; e++)
            if (edges[e].feature < 0 || edges[e].feature >= resident[f]->n)
                return fail(ORBX_E_INVALID, "edge %d: feature %d outside frame %d's [0, %d)", e, edges[e].feature, f, resident[f]->n);
    }
    if ((rc = orbm_check(h))) return rc;
    for (int f = 0; f < n_frames; f++) if ((rc = frame_usable(h, resident[f]))) return rc;
    return orbo_core(h, frames, resident, std::vector<orbo::Obs>(), n_frames, edge_start, edges, inv_level_sigma2, nlevels, out, outlier);
}
