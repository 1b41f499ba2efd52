// orbf_host.inc -- the host pieces that the two batched Fuse searches share (part of orbslamm_hip.hip; device side:
// orbf_kernels.hip, DESIGN.md §8n): the target sides of orbl_fuse_batch* (orbl_host.inc, §8l) and orbc_search_and_fuse*
// (orbc_host.inc, §8m) from host arrays or frames, their place in the staging block, the target records with the grid of
// host arrays built in AssignFeaturesToGrid's order, and the level tables of a kernel's arguments.  What a caller keeps is
// what differs: its own checks, its work (a job list cut into tiles; tile counts, scan and compaction) and its copy down.

static_assert(sizeof(OrblFuseTarget) == 116 && sizeof(OrblFusePoint) == 64 && sizeof(OrblFusePoint) == sizeof(orbf::FusePt), "fuse record layouts");
static_assert(orbf::FST_FOUND == ORBL_FUSE_ST_FOUND && orbf::FST_LEVEL_RANGE == ORBL_FUSE_ST_LEVEL_RANGE, "fuse status codes");

// one target's arrays: resident in HBM (a frame's), or host arrays that ride in the call's staging block.  `first`: the
// earliest target with the same host arrays and grid (the target itself when there is none): they ride once
struct OrbfSide { bool dev; const void* keys; const uint8_t* desc; const int32_t* cellStart; const int32_t* cellIdx; orbm::GridDev gd; int n; int first; };

static int orbf_sides_host(const OrblFuseTarget* targets, const OrbxKeyPoint* const* keys_un, const uint8_t* const* desc, const int32_t* n,
                           int n_targets, std::vector<OrbfSide>& sides)
{
    if (n_targets && (!keys_un || !desc || !n)) return fail(ORBX_E_INVALID, "bad argument");
    sides.resize((size_t)n_targets);
    std::map<const void*, int> seen;   // keys_un -> the earliest target that gave it
    for (int k = 0; k < n_targets; k++) {
        if (n[k] < 0 || (n[k] && (!keys_un[k] || !desc[k]))) return fail(ORBX_E_INVALID, "target %d: bad argument", k);
        if (n[k] > 65535) return fail(ORBX_E_INVALID, "%d features in target %d: above 65535", n[k], k);
        const OrbmGrid& g = targets[k].grid;
        if (g.cols < 1 || g.rows < 1 || g.cols * g.rows > (1 << 20)) return fail(ORBX_E_INVALID, "target %d: bad grid", k);
        orbm::GridDev gd;
        gd.minX = g.minX; gd.minY = g.minY; gd.invW = g.invW; gd.invH = g.invH; gd.cols = g.cols; gd.rows = g.rows;
        sides[k] = {false, keys_un[k], desc[k], nullptr, nullptr, gd, n[k], k};
        if (n[k]) {
            auto it = seen.find(keys_un[k]);
            if (it == seen.end()) seen[keys_un[k]] = k;
            else if (desc[it->second] == desc[k] && n[it->second] == n[k] && memcmp(&targets[it->second].grid, &g, sizeof g) == 0) sides[k].first = it->second;
        }
    }
    return ORBX_OK;
}

static int orbf_sides_frames(orbm_handle* h, orbm_frame_t* const* frames, int n_targets, std::vector<OrbfSide>& sides)
{
    int rc;
    sides.resize((size_t)n_targets);
    for (int k = 0; k < n_targets; k++) {
        orbm_frame* f = frames[k];
        if ((rc = frame_usable(h, f))) return rc;
        if (f->n > 65535) return fail(ORBX_E_INVALID, "%d features in target %d: above 65535", f->n, k);
        sides[k] = {true, f->d_keysUn, f->d_desc, f->d_start, f->d_idx, f->gd, f->n, k};
    }
    return ORBX_OK;
}

// the head of a call's staging block: target records | points | (host arrays of the distinct targets: keys, descriptors, grid)
struct OrbfStage { size_t tgt = 0, pts = 0; std::vector<size_t> keys, desc, cellStart, cellIdx; };

static void orbf_stage_take(Packer& pk, const std::vector<OrbfSide>& sides, int n_points, OrbfStage& o)
{
    const size_t T = sides.size();
    o.tgt = pk.take(T * sizeof(orbf::FuseTgt));
    o.pts = pk.take((size_t)n_points * sizeof(orbf::FusePt));
    o.keys.assign(T, 0); o.desc.assign(T, 0); o.cellStart.assign(T, 0); o.cellIdx.assign(T, 0);
    for (size_t k = 0; k < T; k++) {
        const OrbfSide& S = sides[k];
        if (S.dev || S.first != (int)k) continue;
        const size_t ncell = (size_t)S.gd.cols * S.gd.rows;
        o.keys[k] = pk.take((size_t)std::max(S.n, 1) * sizeof(OrbxKeyPoint));
        o.desc[k] = pk.take((size_t)std::max(S.n, 1) * 32);
        o.cellStart[k] = pk.take((ncell + 1) * 4);
        o.cellIdx[k] = pk.take((size_t)std::max(S.n, 1) * 4);
    }
}

// Frame::AssignFeaturesToGrid (Frame.cc:230-245, PosInGrid :382-392): a counting sort that keeps the insertion order.
// cs: cols * rows + 1 cell starts, ci: the features of the cells
static void orbf_assign_features_to_grid(const OrbxKeyPoint* kp, int n, const orbm::GridDev& gd, int32_t* cs, int32_t* ci)
{
    const int ncell = gd.cols * gd.rows;
    std::vector<int32_t> cell((size_t)n, -1);
    memset(cs, 0, ((size_t)ncell + 1) * 4);
    for (int i = 0; i < n; i++) {
        const float px = roundf((kp[i].x - gd.minX) * gd.invW), py = roundf((kp[i].y - gd.minY) * gd.invH);
        if (!(px >= 0.f && px < (float)gd.cols && py >= 0.f && py < (float)gd.rows)) continue;
        cell[i] = (int)px * gd.rows + (int)py;
        cs[cell[i] + 1]++;
    }
    for (int c = 0; c < ncell; c++) cs[c + 1] += cs[c];
    std::vector<int32_t> fill(cs, cs + ncell);
    for (int i = 0; i < n; i++) if (cell[i] >= 0) ci[fill[cell[i]]++] = i;
}

// fills the head in the pinned block `hs`; `d`: where the block will lie on the device
static void orbf_stage_fill(uint8_t* hs, const uint8_t* d, const OrbfStage& o, const OrblFuseTarget* targets, const std::vector<OrbfSide>& sides,
                            const OrblFusePoint* points, int n_points)
{
    orbf::FuseTgt* td = (orbf::FuseTgt*)(hs + o.tgt);
    for (size_t k = 0; k < sides.size(); k++) {
        const OrbfSide& S = sides[k];
        const OrblFuseTarget& R = targets[k];
        orbf::FuseTgt& D = td[k];
        memset(&D, 0, sizeof D);
        memcpy(D.Rcw, R.Rcw, sizeof D.Rcw); memcpy(D.tcw, R.tcw, sizeof D.tcw); memcpy(D.Ow, R.Ow, sizeof D.Ow);
        D.fx = R.K[0]; D.fy = R.K[1]; D.cx = R.K[2]; D.cy = R.K[3];
        D.minX = R.min_x; D.maxX = R.max_x; D.minY = R.min_y; D.maxY = R.max_y;
        D.grid = S.gd; D.n = S.n;
        if (S.dev) { D.keys = (const orbm::KeyDev*)S.keys; D.desc = S.desc; D.cellStart = S.cellStart; D.cellIdx = S.cellIdx; continue; }
        const size_t f = (size_t)S.first;
        D.keys = (const orbm::KeyDev*)(d + o.keys[f]); D.desc = d + o.desc[f];
        D.cellStart = (const int32_t*)(d + o.cellStart[f]); D.cellIdx = (const int32_t*)(d + o.cellIdx[f]);
        if (f != k) continue;
        orbf_assign_features_to_grid((const OrbxKeyPoint*)S.keys, S.n, S.gd, (int32_t*)(hs + o.cellStart[k]), (int32_t*)(hs + o.cellIdx[k]));
        if (S.n) { memcpy(hs + o.keys[k], S.keys, (size_t)S.n * sizeof(OrbxKeyPoint)); memcpy(hs + o.desc[k], S.desc, (size_t)S.n * 32); }
    }
    memcpy(hs + o.pts, points, (size_t)n_points * sizeof(orbf::FusePt));
}

static int orbf_check_breaks(const float* level_breaks, int nlevels)
{
    for (int j = 0; j < nlevels; j++)
        if (!(level_breaks[j] < level_breaks[j + 1])) return fail(ORBX_E_INVALID, "the level-break table does not ascend at %d", j);
    return ORBX_OK;
}

// the level tables that both kernels' arguments carry
static void orbf_fill_tables(const float* scale_factors, const float* level_breaks, int nlevels, float sf[16], float breaks[17])
{
    for (int i = 0; i < 16; i++) sf[i] = i < nlevels ? scale_factors[i] : 0.f;
    for (int i = 0; i < 17; i++) breaks[i] = i <= nlevels ? level_breaks[i] : 0.f;
}
