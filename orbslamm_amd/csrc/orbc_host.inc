// orbc_host.inc -- host side of the device SearchAndFuse (part of orbslamm_hip.hip; kernels: orbc_kernels.hip, ABI:
// include/orbslamm_loopfuse.h, DESIGN.md §8m).  One call = the checks, (host arrays: every distinct target's grid built on
// the host in AssignFeaturesToGrid's order), one packed upload, three launches, the copy of hit_start down, one
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
    for (int j = 0; j < nlevels; j++)
        if (!(level_breaks[j] < level_breaks[j + 1])) return fail(ORBX_E_INVALID, "the level-break table does not ascend at %d", j);
    if ((n_targets && !targets) || (n_points && !points)) return fail(ORBX_E_INVALID, "bad argument");
    if (n_targets == 0 || n_points == 0) {
        if (hit_start) memset(hit_start, 0, ((size_t)n_targets + 1) * 4);
        return ORBX_OK;
    }
    *empty = false;
    return ORBX_OK;
}

// sides[k].keys of a host side names the arrays; `first[k]` is the earliest target with the same arrays and grid (k itself
// when there is none): those arrays ride in the staging block once
static int orbc_core(orbm_handle* h, const OrblFuseTarget* targets, const std::vector<OrblFuseSide>& sides, const std::vector<int>& first,
                     const OrblFusePoint* points, int P, float th, int max_dist, const float* scale_factors, int nlevels,
                     const float* level_breaks, OrbcHit* hits, int capacity, int* n_hits, int32_t* hit_start, uint8_t* status)
{
    int rc;
    const int T = (int)sides.size();
    const int tilesPerTarget = (P + orbc::kTile - 1) / orbc::kTile;
    const int nTiles = T * tilesPerTarget;
    const int64_t pairs = (int64_t)T * P;
    // the staging block: target records | points | (host arrays of the distinct targets: keys, descriptors, grid)
    Packer pk;
    const size_t oTgt = pk.take((size_t)T * sizeof(orbl::FuseTgt)), oPts = pk.take((size_t)P * sizeof(orbl::FusePt));
    std::vector<size_t> oKeys((size_t)T, 0), oDesc((size_t)T, 0), oCs((size_t)T, 0), oCi((size_t)T, 0);
    for (int k = 0; k < T; k++) {
        const OrblFuseSide& S = sides[k];
        if (S.dev || first[k] != k) continue;
        const size_t ncell = (size_t)S.gd.cols * S.gd.rows;
        oKeys[k] = pk.take((size_t)std::max(S.n, 1) * sizeof(OrbxKeyPoint));
        oDesc[k] = pk.take((size_t)std::max(S.n, 1) * 32);
        oCs[k] = pk.take((ncell + 1) * 4);
        oCi[k] = pk.take((size_t)std::max(S.n, 1) * 4);
    }
    const size_t upBytes = pk.off;
    const size_t startBytes = ((size_t)T + 1) * 4;
    enum { S_BLOCK = 12, S_PAIR = 13, S_TILES = 14, S_HITS = 15, S_STATUS = 16 };
    Packer tl;
    const size_t oCnt = tl.take((size_t)nTiles * 4), oOff = tl.take(((size_t)nTiles + 1) * 4), oStart = tl.take(startBytes);
    const int cap = (int)std::min<int64_t>(capacity, pairs);   // (there are never more hits than pairs)
    if ((rc = orbm_reserve(h, S_BLOCK, upBytes)) || (rc = orbm_reserve(h, S_PAIR, (size_t)pairs * 4)) || (rc = orbm_reserve(h, S_TILES, tl.off)) ||
        (rc = orbm_reserve(h, S_HITS, (size_t)std::max(cap, 1) * sizeof(orbc::Hit))) || (status && (rc = orbm_reserve(h, S_STATUS, (size_t)pairs))) ||
        (rc = orbm_pinned(h, std::max(upBytes, startBytes))))
        return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* d = (uint8_t*)h->d_buf[S_BLOCK];
    uint8_t* dt = (uint8_t*)h->d_buf[S_TILES];
    orbl::FuseTgt* td = (orbl::FuseTgt*)(hs + oTgt);
    for (int k = 0; k < T; k++) {
        const OrblFuseSide& S = sides[k];
        const OrblFuseTarget& R = targets[k];
        orbl::FuseTgt& D = td[k];
        memset(&D, 0, sizeof D);
        memcpy(D.Rcw, R.Rcw, sizeof D.Rcw); memcpy(D.tcw, R.tcw, sizeof D.tcw); memcpy(D.Ow, R.Ow, sizeof D.Ow);
        D.fx = R.K[0]; D.fy = R.K[1]; D.cx = R.K[2]; D.cy = R.K[3];
        D.minX = R.min_x; D.maxX = R.max_x; D.minY = R.min_y; D.maxY = R.max_y;
        D.grid = S.gd; D.n = S.n;
        if (S.dev) { D.keys = (const orbm::KeyDev*)S.keys; D.desc = S.desc; D.cellStart = S.cellStart; D.cellIdx = S.cellIdx; continue; }
        const int f = first[k];
        D.keys = (const orbm::KeyDev*)(d + oKeys[f]); D.desc = d + oDesc[f];
        D.cellStart = (const int32_t*)(d + oCs[f]); D.cellIdx = (const int32_t*)(d + oCi[f]);
        if (f != k) continue;
        // Frame::AssignFeaturesToGrid (Frame.cc:230-245, PosInGrid :382-392): a counting sort that keeps the insertion order
        const OrbxKeyPoint* kp = (const OrbxKeyPoint*)S.keys;
        const int ncell = S.gd.cols * S.gd.rows;
        int32_t* cs = (int32_t*)(hs + oCs[k]);
        int32_t* ci = (int32_t*)(hs + oCi[k]);
        std::vector<int32_t> cell((size_t)S.n, -1);
        memset(cs, 0, ((size_t)ncell + 1) * 4);
        for (int i = 0; i < S.n; i++) {
            const float px = roundf((kp[i].x - S.gd.minX) * S.gd.invW), py = roundf((kp[i].y - S.gd.minY) * S.gd.invH);
            if (!(px >= 0.f && px < (float)S.gd.cols && py >= 0.f && py < (float)S.gd.rows)) continue;
            cell[i] = (int)px * S.gd.rows + (int)py;
            cs[cell[i] + 1]++;
        }
        for (int c = 0; c < ncell; c++) cs[c + 1] += cs[c];
        std::vector<int32_t> fill(cs, cs + ncell);
        for (int i = 0; i < S.n; i++) if (cell[i] >= 0) ci[fill[cell[i]]++] = i;
        if (S.n) { memcpy(hs + oKeys[k], S.keys, (size_t)S.n * sizeof(OrbxKeyPoint)); memcpy(hs + oDesc[k], S.desc, (size_t)S.n * 32); }
    }
    memcpy(hs + oPts, points, (size_t)P * sizeof(orbl::FusePt));
    orbc::Args a{};
    a.tgt = (const orbl::FuseTgt*)(d + oTgt); a.pts = (const orbl::FusePt*)(d + oPts);
    a.pair = (uint32_t*)h->d_buf[S_PAIR];
    a.tileCnt = (int32_t*)(dt + oCnt); a.tileOff = (const int32_t*)(dt + oOff); a.hitStart = (int32_t*)(dt + oStart);
    a.hits = (orbc::Hit*)h->d_buf[S_HITS];
    a.status = status ? (uint8_t*)h->d_buf[S_STATUS] : nullptr;
    a.nTargets = T; a.nPoints = P; a.tilesPerTarget = tilesPerTarget; a.nTiles = nTiles; a.capacity = cap; a.maxDist = max_dist; a.nlevels = nlevels;
    a.th = th;
    for (int i = 0; i < 16; i++) a.sf[i] = i < nlevels ? scale_factors[i] : 0.f;
    for (int i = 0; i < 17; i++) a.breaks[i] = i <= nlevels ? level_breaks[i] : 0.f;
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

static bool orbc_same_grid(const OrbmGrid& a, const OrbmGrid& b) { return memcmp(&a, &b, sizeof a) == 0; }

extern "C" int orbc_search_and_fuse(orbm_t* h, const OrblFuseTarget* targets, const OrbxKeyPoint* const* keys_un, const uint8_t* const* desc,
                                    const int32_t* n, int n_targets, const OrblFusePoint* points, int n_points, float th, int max_dist,
                                    const float* scale_factors, int nlevels, const float* level_breaks, OrbcHit* hits, int capacity, int* n_hits,
                                    int32_t* hit_start, uint8_t* status)
{
    bool empty;
    int rc = orbc_check_args(targets, n_targets, points, n_points, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, &empty);
    if (rc) return rc;
    if (n_targets && (!keys_un || !desc || !n)) return fail(ORBX_E_INVALID, "bad argument");
    std::vector<OrblFuseSide> sides((size_t)n_targets);
    std::vector<int> first((size_t)n_targets);
    std::map<const void*, int> seen;   // keys_un -> the earliest target that gave it
    for (int k = 0; k < n_targets; k++) {
        if (n[k] < 0 || (n[k] && (!keys_un[k] || !desc[k]))) return fail(ORBX_E_INVALID, "target %d: bad argument", k);
        if (n[k] > 65535) return fail(ORBX_E_INVALID, "%d features in target %d: above 65535", n[k], k);
        const OrbmGrid& g = targets[k].grid;
        if (g.cols < 1 || g.rows < 1 || g.cols * g.rows > (1 << 20)) return fail(ORBX_E_INVALID, "target %d: bad grid", k);
        orbm::GridDev gd;
        gd.minX = g.minX; gd.minY = g.minY; gd.invW = g.invW; gd.invH = g.invH; gd.cols = g.cols; gd.rows = g.rows;
        sides[k] = {false, keys_un[k], desc[k], nullptr, nullptr, gd, n[k]};
        first[k] = k;
        if (n[k]) {
            auto it = seen.find(keys_un[k]);
            if (it == seen.end()) seen[keys_un[k]] = k;
            else if (desc[it->second] == desc[k] && n[it->second] == n[k] && orbc_same_grid(targets[it->second].grid, g)) first[k] = it->second;
        }
    }
    if ((rc = orbm_check(h)) || empty) return rc;
    return orbc_core(h, targets, sides, first, points, n_points, th, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, status);
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
    if ((rc = orbm_check(h))) return rc;
    std::vector<OrblFuseSide> sides((size_t)n_targets);
    std::vector<int> first((size_t)n_targets);
    for (int k = 0; k < n_targets; k++) {
        orbm_frame* f = frames[k];
        if ((rc = frame_usable(h, f))) return rc;
        if (f->n > 65535) return fail(ORBX_E_INVALID, "%d features in target %d: above 65535", f->n, k);
        sides[k] = {true, f->d_keysUn, f->d_desc, f->d_start, f->d_idx, f->gd, f->n};
        first[k] = k;
    }
    if (empty) return ORBX_OK;
    return orbc_core(h, targets, sides, first, points, n_points, th, max_dist, scale_factors, nlevels, level_breaks, hits, capacity, n_hits, hit_start, status);
}
