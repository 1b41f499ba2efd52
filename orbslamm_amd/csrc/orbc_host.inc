// orbc_host.inc -- host side of the device SearchAndFuse (part of orbslamm_hip.hip; kernels: orbc_kernels.hip, ABI:
// include/orbslamm_loopfuse.h, DESIGN.md §8m).  One call = the checks, the staging of orbf_host.inc (host arrays: every distinct
// target's grid built on the host), one packed upload, three launches, the copy of hit_start down, one
// synchronise, then the copy of exactly the hits and a second synchronise.  Nothing of size T x P crosses the link unless
// the caller asks for the status table.

static_assert(sizeof(OrbcHit) == 16 && sizeof(OrbcHit) == sizeof(orbc::Hit), "OrbcHit layout");
static_assert(ORBC_MAX_TARGETS >= 4096 && ORBC_MAX_PAIRS >= (1 << 26), "the ceilings of orbslamm_loopfuse.h");
static_assert((int64_t)ORBC_MAX_PAIRS / 128 + ORBC_MAX_TARGETS < (1 << 30), "tile counts stay inside int32");

// what needs neither the handle nor a GPU; *empty: nothing to search
static int orbc_check_args(const OrblFuseTarget* targets, int n_targets, const OrblFusePoint* points, int n_points, int max_dist,
                           const float* scale_factors, int nlevels, const float* level_breaks, const OrbcHit* hits, int capacity,
                           int* n_hits, int32_t* hit_start, bool* empty)
{
    *empty = true;
    if (!n_hits) return fail(ORBX_E_INVALID, "bad argument");
    *n_hits = 0;
    if (n_targets < 0 || n_points < 0 || capacity < 0 || (capacity > 0 && !hits)) return fail(ORBX_E_INVALID, "bad argument");
    if (n_targets > ORBC_MAX_TARGETS) return fail(ORBX_E_UNSUPPORTED, "%d targets: above %d", n_targets, ORBC_MAX_TARGETS);
    if ((int64_t)n_targets * n_points > ORBC_MAX_PAIRS)
        return fail(ORBX_E_UNSUPPORTED, "%lld pairs: above %d", (long long)n_targets * n_points, ORBC_MAX_PAIRS);
    if (max_dist < 0 || max_dist > 256) return fail(ORBX_E_INVALID, "max_dist %d outside [0, 256]", max_dist);
    if (!scale_factors || !level_breaks || nlevels < 1 || nlevels > 16) return fail(ORBX_E_INVALID, "bad argument");
    if (int rc = orbf_check_breaks(level_breaks, nlevels)) return rc;
    if ((n_targets && !targets) || (n_points && !points)) return fail(ORBX_E_INVALID, "bad argument");
    if (n_targets == 0 || n_points == 0) {
        if (hit_start) memset(hit_start, 0, ((size_t)n_targets + 1) * 4);
        return ORBX_OK;
    }
    *empty = false;
    return ORBX_OK;
}

static int orbc_core(orbm_handle* h, const OrblFuseTarget* targets, const std::vector<OrbfSide>& sides, const OrblFusePoint* points, int P,
                     float th, int max_dist, const float* scale_factors, int nlevels, const float* level_breaks, OrbcHit* hits, int capacity,
                     int* n_hits, int32_t* hit_start, uint8_t* status)
{
    int rc;
    const int T = (int)sides.size();
    const int tilesPerTarget = (P + orbc::kTile - 1) / orbc::kTile;
    const int nTiles = T * tilesPerTarget;
    const int64_t pairs = (int64_t)T * P;
    // the staging block: orbf's head (target records | points | host arrays of the distinct targets)
    Packer pk;
    OrbfStage st;
    orbf_stage_take(pk, sides, P, st);
    const size_t upBytes = pk.off;
    const size_t startBytes = ((size_t)T + 1) * 4;
    Packer tl;
    const size_t oCnt = tl.take((size_t)nTiles * 4), oOff = tl.take(((size_t)nTiles + 1) * 4), oStart = tl.take(startBytes);
    const int cap = (int)std::min<int64_t>(capacity, pairs);   // (there are never more hits than pairs)
    if ((rc = orbm_reserve(h, {{S_BLOCK, upBytes}, {S_LF_PAIR, (size_t)pairs * 4}, {S_LF_TILES, tl.off}, {S_LF_HITS, (size_t)std::max(cap, 1) * sizeof(orbc::Hit)}})) ||
        (status && (rc = orbm_reserve(h, S_LF_STATUS, (size_t)pairs))) || (rc = orbm_pinned(h, std::max(upBytes, startBytes))))
        return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = slot_ptr<uint8_t>(h, S_BLOCK);
    uint8_t* dt = slot_ptr<uint8_t>(h, S_LF_TILES);
    orbf_stage_fill(hs, d, st, targets, sides, points, P);
    orbc::Args a{};
    a.tgt = (const orbf::FuseTgt*)(d + st.tgt); a.pts = (const orbf::FusePt*)(d + st.pts);
    a.pair = slot_ptr<uint32_t>(h, S_LF_PAIR);
    a.tileCnt = (int32_t*)(dt + oCnt); a.tileOff = (const int32_t*)(dt + oOff); a.hitStart = (int32_t*)(dt + oStart);
    a.hits = slot_ptr<orbc::Hit>(h, S_LF_HITS);
    a.status = status ? slot_ptr<uint8_t>(h, S_LF_STATUS) : nullptr;
    a.nTargets = T; a.nPoints = P; a.tilesPerTarget = tilesPerTarget; a.nTiles = nTiles; a.capacity = cap; a.maxDist = max_dist; a.nlevels = nlevels;
    a.th = th;
    orbf_fill_tables(scale_factors, level_breaks, nlevels, a.sf, a.breaks);
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, hs, upBytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(orbc::k_loopfuse_search, dim3((unsigned)nTiles), dim3(orbc::kTile), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(orbm::k_scan_small, dim3(1), dim3(1024), 0, s, (const int32_t*)a.tileCnt, nTiles, (int32_t*)(dt + oOff));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(orbc::k_loopfuse_compact, dim3((unsigned)nTiles), dim3(orbc::kTile), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs, dt + oStart, startBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int32_t* hst = (const int32_t*)hs;
    const int total = hst[T];
    *n_hits = total;
    if (total > capacity) return fail(ORBX_E_CAPACITY, "%d hits: above the capacity of %d", total, capacity);
    if (hit_start) memcpy(hit_start, hst, startBytes);
    if (total) {
        const size_t hitBytes = (size_t)total * sizeof(orbc::Hit);
        if ((rc = orbm_pinned(h, hitBytes))) return rc;   // (hit_start has been read: the block may be replaced)
        HIPCHK(hipMemcpyAsync(h->h_stage, a.hits, hitBytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        memcpy(hits, h->h_stage, hitBytes);
    }
    if (status) HIPCHK(hipMemcpy(status, a.status, (size_t)pairs, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbc_search_and_fuse(orbm_t* h, const OrblFuseTarget* targets, const OrbxKeyPoint* const* keys_un, const uint8_t* const* desc,
                                    const int32_t* n, int n_targets, const OrblFusePoint* points, int n_points, float th, int max_dist,
                                    const float* scale_factors, int nlevels, const float* level_breaks, OrbcHit* hits, int capacity, int* n_hits,
                                    int32_t* hit_start, uint8_t* status)
{
    bool empty;
    int rc = orbc_check_args(targets, n_targets, points, n_points, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, &empty);
    if (rc) return rc;
    std::vector<OrbfSide> sides;
    if ((rc = orbf_sides_host(targets, keys_un, desc, n, n_targets, sides)) || (rc = orbm_check(h)) || empty) return rc;
    return orbc_core(h, targets, sides, points, n_points, th, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, status);
}

extern "C" int orbc_search_and_fuse_frames(orbm_t* h, const OrblFuseTarget* targets, orbm_frame_t* const* frames, int n_targets,
                                           const OrblFusePoint* points, int n_points, float th, int max_dist, const float* scale_factors,
                                           int nlevels, const float* level_breaks, OrbcHit* hits, int capacity, int* n_hits,
                                           int32_t* hit_start, uint8_t* status)
{
    bool empty;
    int rc = orbc_check_args(targets, n_targets, points, n_points, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, &empty);
    if (rc) return rc;
    if (n_targets && !frames) return fail(ORBX_E_INVALID, "null frame");
    std::vector<OrbfSide> sides;
    if ((rc = orbm_check(h)) || (rc = orbf_sides_frames(h, frames, n_targets, sides)) || empty) return rc;
    return orbc_core(h, targets, sides, points, n_points, th, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, status);
}
