// orbm_host.inc -- host side of the matcher entries (part of orbslamm_hip.hip): descriptor text, the matcher handle,
// SearchByBoW, the grid, the SearchByProjection family (orbt_host.inc), device-resident frames, the remaining ORBmatcher members.

// ------------------------------------------------------------------ MapSerializer's descriptor text (SURVEY.md 8f.4)
// `os << pKF->mDescriptors` / `os << pMP->GetDescriptor()` into an XML attribute (src/MapSerializer.cc:344-347, 429-431):
// cv::Mat's stream operator with OpenCV 3.0's default formatter -- "[" rows "]", elements "%3d" separated by ", ", rows by
// ";\n " (restated from the published out.cpp: third-party formatting, unpinned; the reference never reads it back).
// Host-side string formatting of data that is on the host already: not a compute path, works without a device.
extern "C" int orbm_descriptors_to_text(const uint8_t* desc, int n, int cols, char* out, size_t cap, size_t* len)
{
    if (n < 0 || cols < 0 || (n > 0 && cols > 0 && !desc) || !len) return fail(ORBX_E_INVALID, "bad argument");
    const size_t need = 2 + (size_t)n * ((size_t)cols * 3 + (cols > 0 ? (size_t)(cols - 1) * 2 : 0)) + (n > 0 ? (size_t)(n - 1) * 3 : 0);
    *len = need;
    if (!out) return ORBX_OK;                       // size query
    if (cap < need + 1) return fail(ORBX_E_CAPACITY, "text needs %zu bytes", need + 1);
    char* p = out;
    *p++ = '[';
    for (int r = 0; r < n; r++) {
        if (r) { *p++ = ';'; *p++ = '\n'; *p++ = ' '; }
        for (int c = 0; c < cols; c++) {
            if (c) { *p++ = ','; *p++ = ' '; }
            const unsigned v = desc[(size_t)r * cols + c];
            p[0] = v >= 100 ? (char)('0' + v / 100) : ' ';
            p[1] = v >= 10 ? (char)('0' + (v / 10) % 10) : ' ';
            p[2] = (char)('0' + v % 10);
            p += 3;
        }
    }
    *p++ = ']';
    *p = 0;
    return ORBX_OK;
}

// the inverse (a loader the reference does not have: MultiMapper::InitFromFile never reads descriptors back)
extern "C" int orbm_descriptors_from_text(const char* text, uint8_t* desc, int cap_rows, int cols, int* n_rows)
{
    if (!text || cols < 1 || !n_rows) return fail(ORBX_E_INVALID, "bad argument");
    const char* p = text;
    while (*p == ' ' || *p == '\n') p++;
    if (*p != '[') return fail(ORBX_E_INVALID, "descriptor text does not start with '['");
    p++;
    int r = 0, c = 0;
    bool any = false;
    for (;;) {
        while (*p == ' ' || *p == '\n') p++;
        if (*p == ']') break;
        if (*p < '0' || *p > '9') return fail(ORBX_E_INVALID, "unexpected character '%c' in descriptor text", *p);
        unsigned v = 0;
        while (*p >= '0' && *p <= '9') v = v * 10 + (unsigned)(*p++ - '0');
        if (v > 255 || c >= cols) return fail(ORBX_E_INVALID, "descriptor text: value or column out of range");
        if (desc) { if (r >= cap_rows) return fail(ORBX_E_CAPACITY, "more than %d rows", cap_rows); desc[(size_t)r * cols + c] = (uint8_t)v; }
        any = true;
        c++;
        while (*p == ' ') p++;
        if (*p == ',') p++;
        else if (*p == ';') { if (c != cols) return fail(ORBX_E_INVALID, "descriptor text: short row"); p++; r++; c = 0; }
        else if (*p != ']') return fail(ORBX_E_INVALID, "descriptor text: missing separator");
    }
    if (any) { if (c != cols) return fail(ORBX_E_INVALID, "descriptor text: short row"); r++; }
    *n_rows = r;
    return ORBX_OK;
}

// ------------------------------------------------------------------ matcher handle
// Ownership (SURVEY.md 8b): the reference builds an ORBmatcher as a stack temporary at every call site -- Tracking.cc:639,
// 809, 914, 1242, 1415, 1454, LocalMapping.cc:215, 483, LoopClosing.cc:245, 603, MultiMapper.cc:180, 687 -- holding only
// (mfNNratio, mbCheckOrientation).  So the device state a search needs (a queue, grow-only scratch, a pinned staging
// block) cannot belong to the matcher OBJECT: it belongs to the calling THREAD (orbm_thread_handle), made at the thread's
// first search and kept until the thread ends.  Constructing and destroying a matcher then touches no HIP API at all.
// orbm_create / orbm_destroy remain for callers that want a handle of their own (the ctypes mirror, the frame sets).
//
// THE list of a handle's device scratch blocks, for every family that runs on one (orbm_*, orbt, orbl_*, orbc_*): one name per role, one entry
// family (the entries and the core they share) per name, no numbers -- a new block is a new name.  Reached through the helpers below only.
enum OrbmSlot {
    S_DM_Q, S_DM_T, S_DM_DIST,                              // orbm_distance_matrix, the one entry
    S_BF_QD, S_BF_TD, S_BF_QA, S_BF_TA, S_BF_CNT, S_BF_MATCH, S_BF_BIN, S_BF_HIST, S_BF_BEST2, S_BF_XDESC,   // orbm_match_bruteforce (CNT: {nq, nt}; HIST: 32 bins + nmatch)
    S_FA_OUT, S_FA_CNT,                                     // orbm_features_in_area, on top of the G_ blocks
    // the grid of a host-array train side: reserved and built by orbm_build_grid, read by its callers (orbm_features_in_area, orbm_window_best,
    // orbm_search_for_initialization).  G_CNT / G_FILL: frame_build_big's scratch too, which may use them from a frame set's stream (and drains it)
    G_KEYS, G_CNT, G_START, G_FILL, G_IDX,
    // a family's entries reserve and fill the blocks before the bar (device-resident frames bring their own), its core the others; the core reads all
    S_WIN_TD, S_WIN_TUR, /* orbm_window_best | window_core */ S_WIN_UVR, S_WIN_UR, S_WIN_PRED, S_WIN_QD, S_WIN_QV, S_WIN_SIG, S_WIN_BI, S_WIN_BD,
    S_INI_QD, S_INI_QA, S_INI_QV, S_INI_TD, /* orbm_search_for_initialization (its _frames form: S_INI_QV alone) | init_core */
    S_INI_UVR, S_INI_LVL, S_INI_CNT, S_INI_OFF, S_INI_KEY, S_INI_CIDX, S_INI_M12, S_INI_M21, S_INI_NM, S_INI_PUSHT, S_INI_PUSHB,
    S_TRI_K1, S_TRI_D1, S_TRI_K2, S_TRI_D2, S_TRI_ST1, S_TRI_I1, S_TRI_ST2, S_TRI_I2, /* orbm_search_for_triangulation | tri_core */
    S_TRI_S1, S_TRI_U1, S_TRI_S2, S_TRI_U2, S_TRI_PA, S_TRI_PB, S_TRI_M12, S_TRI_BIN, S_TRI_NMATCH,
    S_UND_IN, S_UND_OUT, S_RGBD_KEYS, S_RGBD_KEYSUN, S_RGBD_DEPTH, S_RGBD_OUT, S_DIS_DESC, S_DIS_START, S_DIS_BEST,   // orbm_undistort_keypoints, _compute_stereo_from_rgbd, _distinctive_descriptors
    S_BLOCK,                                                // THE ONE SHARED NAME: the packed block of orbl_core, orbl_fuse_core, orbc_core, orbo_core, orbz_optimize_sim3, orbw_project_sync, orby_compute_sim3, orbq_track_pose, orbq_track_reference, orbq_relocalize, orbq_track_motion_model and orbb_core, which never nest
    // (each packs its whole call into it -- uploads, work arrays, results, flags -- at offsets that follow from the call's sizes, and stages through h_stage: a
    // call lands on whatever a larger call of another family left there, so none may read a word of it before writing it.  tests/test_gpu_one_handle.py)
    S_LF_PAIR, S_LF_TILES, S_LF_HITS, S_LF_STATUS,          // orbc_core besides S_BLOCK
    S_RELOC_ARENA,                                          // orbq_relocalize besides S_BLOCK: the searches' candidate arena, a share a job
    S_MOTION_ARENA,                                         // orbq_track_motion_model besides S_BLOCK: the same
    T_STAGE, /* device twin of the pinned staging block: bow_core and proj_core (orbt_host.inc) | proj_core, call scratch */ T_OFF, T_CAND, T_QRES, T_TSCR,
    // PERSISTENT -- these live ACROSS calls and are the projection search's alone.  T_FS / T_PREP: the scratch frame and the upload orbm_projection_prepare
    // leaves for the next search.  T_STATS: proj_core's candidate counter, zeroed when the block is first made (slot_cap() == 0), left zero by every resolve
    T_FS, T_PREP, T_STATS,
    ORBM_SLOT_COUNT
};
// What else of a handle lives ACROSS calls, besides T_FS / T_PREP / T_STATS (every other block is a call's own from its first write on): prep and
// callSeq (a prepared train side is good for the very next entry on the handle, whatever that entry is), stageSeq and the flag word behind h_stage
// (stage_down_wait counts on through a regrown block, whose word grow_pinned zeroes), relocArena / motionArena (a job's share of S_RELOC_ARENA /
// S_MOTION_ARENA: set by orbq_debug_*_arena, grown by an overflow and kept), lastRounds / lastCands, ldsAttr, the frame blocks and the counters.
struct FrameBlock { void* p; size_t bytes; };
struct orbm_handle {
    int device = -1;
    hipStream_t stream = nullptr;
    int chainIdx = -1;                   // >= 0: `stream` is one of the device's shared chain streams (chain_stream_acquire), not owned
    void* d_buf[ORBM_SLOT_COUNT] = {nullptr};   // growable scratch, one block per OrbmSlot
    size_t d_cap[ORBM_SLOT_COUNT] = {0};
    // one packed upload / download per call (orbt_host.inc)
    void* h_stage = nullptr; size_t h_stageCap = 0;   // (+ 64 bytes behind it: the flag of stage_down_wait)
    int32_t stageSeq = 0;
    size_t ldsAttr[8] = {0};             // hipFuncAttributeMaxDynamicSharedMemorySize already raised for kernel i
    int lastRounds = 0, lastCands = 0;   // of the last projection search (orbm_last_search_stats)
    // a chain's candidate arena (orbq_scaffold.inc): entries of a job's share (0: the entry's default), grown by an overflow and set by the
    // entry's orbq_debug_*_arena, and how many times the entry's last call ran its chain
    struct CandArena { int entries = 0, runs = 0; };
    CandArena relocArena, motionArena;   // orbq_relocalize's S_RELOC_ARENA, orbq_track_motion_model's S_MOTION_ARENA
    // orbm_projection_prepare: the train side of the NEXT orbm_search_by_projection, already in HBM with its grid built
    // (identified by the caller's pointers, count and grid: the search falls back to its own upload when they differ)
    struct Prepared { bool valid = false, inFlight = false; const void* keys = nullptr; const void* desc = nullptr; int nt = 0; OrbmGrid grid{}; uint64_t seq = 0; } prep;
    uint64_t callSeq = 0;                // entries made on this handle (orbm_check)
    void* h_prep = nullptr; size_t h_prepCap = 0;   // pinned block of its own: the search's staging block is refilled while this upload may still run
    // Device-resident frames (orbm_frame_*) hold a reference: a handle whose owner let go of it (orbm_destroy, the end of
    // its thread) lives on until the last of its frames is destroyed -- KeyFrames outlive the Tracking call that made them.
    std::atomic<int> refs{1};
    // one arena block per frame, recycled: a Frame per image allocates nothing in steady state (SURVEY.md 8b "no
    // allocation on the per-frame path").  Frames may be destroyed from any thread, hence the lock.
    std::mutex poolMu;
    std::vector<FrameBlock> freeBlocks;
    // allocation counters (orbm_alloc_stats): what the steady-state tests read
    std::atomic<int64_t> nDevAlloc{0}, nHostAlloc{0};
};
static std::atomic<int64_t> g_orbmHandlesMade{0};

// the only code that indexes d_buf / d_cap: grow a block (or several, in order), its pointer, its capacity, a copy into it on the handle's stream
static int orbm_reserve(orbm_handle* h, OrbmSlot s, size_t bytes) { return grow_device(h->d_buf[s], h->d_cap[s], bytes, 4096, nullptr, &h->nDevAlloc); }
struct SlotBytes { OrbmSlot slot; size_t bytes; };
static int orbm_reserve(orbm_handle* h, std::initializer_list<SlotBytes> blocks) { for (const SlotBytes& b : blocks) if (int rc = orbm_reserve(h, b.slot, b.bytes)) return rc; return ORBX_OK; }
template <class T = void> static T* slot_ptr(const orbm_handle* h, OrbmSlot s) { return (T*)h->d_buf[s]; }
static size_t slot_cap(const orbm_handle* h, OrbmSlot s) { return h->d_cap[s]; }
static int slot_upload(orbm_handle* h, OrbmSlot s, const void* src, size_t bytes) { HIPCHK(hipMemcpyAsync(h->d_buf[s], src, bytes, hipMemcpyHostToDevice, h->stream)); return ORBX_OK; }

// own_stream: a queue of the handle's own (orbm_create); otherwise one of the device's four chain streams, shared with the
// latency extractors (DESIGN.md section 4: every queue a process owns takes part in the GPU's rotation, busy or not -- a
// robot is three or four threads that all build matchers, eight robots would be thirty queues)
static int orbm_make_handle(int device, bool own_stream, orbm_handle** out)
{
    *out = nullptr;
    int ndev = orbx_device_count();
    if (ndev == 0) return fail(ORBX_E_NO_DEVICE, "no HIP device visible: the ORB matcher has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(ORBX_E_INVALID, "device %d out of range", device);
    orbm_handle* h = new orbm_handle();
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete h; return fail(ORBX_E_HIP, "cannot select device %d", device); }
    if (own_stream) {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            delete h;
            return fail(ORBX_E_HIP, "cannot create stream on device %d", device);
        }
    } else {
        int prLo = 0, prHi = 0;
        if (hipDeviceGetStreamPriorityRange(&prLo, &prHi) != hipSuccess) { delete h; return fail(ORBX_E_HIP, "cannot query stream priorities on device %d", device); }
        // (the pool is shared with the latency extractors: same priority rule, whoever comes first -- and its consequence:
        // a thread handle's synchronous entries wait on a stream other robots' chains are queued on as well; correct, but a
        // robot's matcher call can wait for another robot's frame.  include/orbslamm_hip.h says so next to orbm_thread_handle.)
        const int rc = chain_stream_acquire(device, chain_prio_normal() ? 0 : prHi, &h->stream, &h->chainIdx);
        if (rc) { delete h; return rc; }
    }
    // k_match_mfma's ring of train tiles is dynamic LDS above the default limit
    if (hipFuncSetAttribute((const void*)orbm::k_match_mfma, hipFuncAttributeMaxDynamicSharedMemorySize, orbm::kMfmaLdsBytes) != hipSuccess) {
        if (h->chainIdx >= 0) chain_stream_release(device, h->chainIdx); else (void)hipStreamDestroy(h->stream);
        delete h;
        return fail(ORBX_E_HIP, "cannot reserve %d bytes of LDS for the brute-force scan on device %d", orbm::kMfmaLdsBytes, device);
    }
    g_orbmHandlesMade++;
    live_add(h);
    *out = h;
    return ORBX_OK;
}

extern "C" int orbm_create(int device, orbm_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    return orbm_make_handle(device, true, out);
}

// drops one reference; the last one tears the device state down
static void orbm_release(orbm_handle* h)
{
    if (h->refs.fetch_sub(1) != 1) return;
    (void)hipSetDevice(h->device);
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        if (h->chainIdx >= 0) chain_stream_release(h->device, h->chainIdx);
        else (void)hipStreamDestroy(h->stream);
    }
    for (auto p : h->d_buf) if (p) (void)hipFree(p);
    for (const FrameBlock& b : h->freeBlocks) (void)hipFree(b.p);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_prep) (void)hipHostFree(h->h_prep);
    delete h;
}

extern "C" void orbm_destroy(orbm_t* h)
{
    if (!h) return;
    live_remove(h);   // no new calls; frames that still point here keep the memory alive (orbm_release)
    orbm_release(h);
}

static int orbm_check(orbm_handle* h)
{
    if (!h) return fail(ORBX_E_INVALID, "null handle");
    h->callSeq++;   // every entry on the handle counts: a prepared train side is good for the VERY NEXT call only (orbm_projection_prepare)
    HIPCHK(hipSetDevice(h->device));
    return ORBX_OK;
}

// What a solver made on a matcher handle holds of it (the Initializer, the Sim3Solver, the PnPsolver): a reference to the
// handle, whose device and stream it works on, a grow-only device work block and the pinned block of its uploads and downloads.
namespace {   // (its inline members are no exports of the library)
struct orbm_solver_base {
    orbm_handle* h = nullptr;            // device and stream; a reference is held
    void* d_work = nullptr; size_t workCap = 0;
    uint8_t* h_stage = nullptr; size_t stageCap = 0;
    void attach(orbm_handle* handle) { h = handle; h->refs++; }
    int reserve(size_t work, size_t stage)
    {
        const int rc = grow_device(d_work, workCap, work, 1 << 16, &h->stream);
        return rc ? rc : grow_pinned(h_stage, stageCap, stage, false);
    }
    // drains the stream, frees the solver's own device blocks and the two above, lets go of the handle
    void release(std::initializer_list<void*> own)
    {
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        for (void* p : own) if (p) (void)hipFree(p);
        if (d_work) (void)hipFree(d_work);
        if (h_stage) (void)hipHostFree(h_stage);
        orbm_release(h);
    }
};

// What the two RANSAC solvers (the Sim3Solver, the PnPsolver) hold and do alike: SetRansacParameters' values, iterate's
// counters, the per-hypothesis table of the family's last run (Hyp: its row) and the flags of the hypothesis it returns.
// iterate itself and the run chains are the families' own: the two references differ there in substance.
template <class Hyp>
struct orbm_ransac_base : orbm_solver_base {
    int n = 0;                           // N correspondences
    uint8_t* d_mask = nullptr;           // n flags of the returned hypothesis
    double prob = 0.99;
    int minInliers = 0, maxIts = 300;    // (minInliers: the family's default, set by its struct)
    int nIterations = 0, bestInliers = 0;
    bool tableValid = false;
    std::vector<Hyp> table;
    double runMs[4] = {0, 0, 0, 0};      // the last batch's legs (the Sim3Solver has three)

    // the table, behind orbs_hypotheses / orbp_hypotheses (family: "orbs", "orbp")
    int hypotheses(const char* family, Hyp* out, int cap, int* n_out) const
    {
        if (!n_out || (cap > 0 && !out) || cap < 0) return fail(ORBX_E_INVALID, "bad argument");
        if (!tableValid) return fail(ORBX_E_INVALID, "no table: %s_run comes first", family);
        *n_out = (int)table.size();
        if (cap < *n_out) return fail(ORBX_E_CAPACITY, "%d hypotheses, room for %d", *n_out, cap);
        if (*n_out) memcpy(out, table.data(), table.size() * sizeof(Hyp));
        return ORBX_OK;
    }
    // behind the family's mask kernel on the handle's stream: the n flags of d_mask down, inliers[idx[i]] = 1 where set
    int scatter_mask(const std::vector<int32_t>& idx, uint8_t* inliers)
    {
        std::vector<uint8_t> m((size_t)n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(m.data(), d_mask, (size_t)n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int i = 0; i < n; i++) if (m[i]) inliers[idx[i]] = 1;
        return ORBX_OK;
    }
};

// SetRansacParameters' iteration count (Sim3Solver.cc:122-147, PnPsolver.cc:138-157), libm on the host as the references
// call it: ceil(log(1 - p) / log(1 - epsilon^3)), 1 when every correspondence must be an inlier, inside [1, maxIterations].
// The double -> int conversion is x86's (NaN and out-of-range values give INT_MIN), which the references leave to their compiler.
static int ransac_iterations(int n, double probability, int minInliers, int maxIterations, float epsilon)
{
    int nIterations;
    if (minInliers == n)
        nIterations = 1;
    else {
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
    }
    return std::max(1, std::min(nIterations, maxIterations));
}

// a run's batch: every entry a solver, all on one matcher handle, none twice; *h: that handle, made current
template <class S>
static int ransac_batch(S* const* solvers, int count, orbm_handle** h)
{
    for (int c = 0; c < count; c++) {
        if (!solvers[c]) return fail(ORBX_E_INVALID, "solvers[%d] is null", c);
        if (solvers[c]->h != solvers[0]->h) return fail(ORBX_E_INVALID, "solvers[%d] belongs to another matcher handle", c);
        for (int e = 0; e < c; e++) if (solvers[e] == solvers[c]) return fail(ORBX_E_INVALID, "solvers[%d] repeats solvers[%d]", c, e);
    }
    *h = solvers[0]->h;
    return orbm_check(*h);
}
}  // namespace

// The calling thread's matcher handle for `device` (ORBmatcher.h:37-102: the state an ORBmatcher temporary needs but
// cannot own).  Made at the first call of a thread, returned as is afterwards; released when the thread ends.
struct ThreadHandles {
    orbm_handle* h[64] = {nullptr};
    ~ThreadHandles() { for (orbm_handle* p : h) if (p) orbm_destroy(p); }
};
extern "C" int orbm_thread_handle(int device, orbm_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    if (device < 0 || device >= 64) return fail(ORBX_E_INVALID, "device %d out of range", device);
    static thread_local ThreadHandles tl;
    if (!tl.h[device]) {
        const int rc = orbm_make_handle(device, false, &tl.h[device]);
        if (rc) return rc;
    }
    *out = tl.h[device];
    return ORBX_OK;
}

// Allocation counters of a handle (null: process-wide number of matcher handles made): device allocations (scratch growth
// + frame blocks), pinned allocations.  A steady-state loop must leave them unchanged.
extern "C" int orbm_alloc_stats(orbm_t* h, int64_t* device_allocs, int64_t* host_allocs, int64_t* handles_made)
{
    if (device_allocs) *device_allocs = h ? h->nDevAlloc.load() : 0;
    if (host_allocs) *host_allocs = h ? h->nHostAlloc.load() : 0;
    if (handles_made) *handles_made = g_orbmHandlesMade.load();
    return ORBX_OK;
}

extern "C" int orbm_distance_matrix(orbm_t* h, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* dist)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (nq < 0 || nt < 0 || (nq && !q) || (nt && !t) || !dist) return fail(ORBX_E_INVALID, "bad argument");
    if (nq == 0 || nt == 0) return ORBX_OK;
    if ((rc = orbm_reserve(h, {{S_DM_Q, (size_t)nq * 32}, {S_DM_T, (size_t)nt * 32}, {S_DM_DIST, (size_t)nq * nt * 4}}))) return rc;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_DM_Q), q, (size_t)nq * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_DM_T), t, (size_t)nt * 32, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(orbm::k_distance_matrix, dim3((nq + 255) / 256, std::min(nt, 64)), dim3(256), 0, s,
                       slot_ptr<const uint8_t>(h, S_DM_Q), nq, slot_ptr<const uint8_t>(h, S_DM_T), nt, slot_ptr<int32_t>(h, S_DM_DIST));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dist, slot_ptr(h, S_DM_DIST), (size_t)nq * nt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

extern "C" int orbm_match_bruteforce(orbm_t* h, const uint8_t* qdesc, const float* qangle, int nq,
                                     const uint8_t* tdesc, const float* tangle, int nt,
                                     float nnratio, int th_low, int check_ori, int32_t* match, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (nq < 0 || nt < 0 || (nq && (!qdesc || !qangle || !match)) || (nt && (!tdesc || !tangle))) return fail(ORBX_E_INVALID, "bad argument");
    if (nmatches) *nmatches = 0;
    if (nq == 0) return ORBX_OK;
    if ((rc = orbm_reserve(h, {{S_BF_QD, (size_t)nq * 32}, {S_BF_TD, (size_t)std::max(nt, 1) * 32}, {S_BF_QA, (size_t)nq * 4}, {S_BF_TA, (size_t)std::max(nt, 1) * 4},
                               {S_BF_CNT, 16}, {S_BF_MATCH, (size_t)nq * 4}, {S_BF_BIN, (size_t)nq}, {S_BF_HIST, 34 * 4}}))) return rc;
    hipStream_t s = h->stream;
    const int32_t counts[2] = {nq, nt};
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_BF_QD), qdesc, (size_t)nq * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_BF_QA), qangle, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    if (nt) {
        HIPCHK(hipMemcpyAsync(slot_ptr(h, S_BF_TD), tdesc, (size_t)nt * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(slot_ptr(h, S_BF_TA), tangle, (size_t)nt * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_BF_CNT), counts, sizeof counts, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(slot_ptr(h, S_BF_HIST), 0, 34 * 4, s));
    orbm::MatchIO q{slot_ptr<const uint8_t>(h, S_BF_QD), 0, slot_ptr<const float>(h, S_BF_QA), 0, 1, slot_ptr<const int32_t>(h, S_BF_CNT)};
    orbm::MatchIO t{slot_ptr<const uint8_t>(h, S_BF_TD), 0, slot_ptr<const float>(h, S_BF_TA), 0, 1, slot_ptr<const int32_t>(h, S_BF_CNT) + 1};
    int32_t* d_hist = slot_ptr<int32_t>(h, S_BF_HIST);
    if ((rc = orbm_reserve(h, S_BF_BEST2, (size_t)nq * kMatchChunks * sizeof(uint2)))) return rc;
    const bool mfma = nt < 65536;  // the MFMA scan packs the train index into 16 bits of its key
    orbm::AcceptArgs aa = {q, t, 0, 0, nnratio, th_low, check_ori, slot_ptr<int32_t>(h, S_BF_MATCH), (int64_t)nq, slot_ptr<uint8_t>(h, S_BF_BIN), d_hist};
    if (mfma) {
        const int64_t xPitch = (int64_t)align_up(std::max(nq, nt), orbm::kMfmaRowsPerBlock) * orbm::kMfmaDescBytes;
        if ((rc = orbm_reserve(h, S_BF_XDESC, (size_t)2 * xPitch))) return rc;
        hipLaunchKernelGGL(orbm::k_expand_desc, dim3((unsigned)(xPitch / 4096), 1), dim3(256), 0, s, q, 0, 0, slot_ptr<uint8_t>(h, S_BF_XDESC), xPitch);
        hipLaunchKernelGGL(orbm::k_expand_desc, dim3((unsigned)(xPitch / 4096), 1), dim3(256), 0, s, t, 0, 1, slot_ptr<uint8_t>(h, S_BF_XDESC), xPitch);
        // slot table {nq, nt}: query slot 0, train slot 1 (angles keep their own slot 0 via pitch 0)
        orbm::AcceptArgs am = aa;
        am.tslot0 = 1;
        const int nqb = (nq + orbm::kMfmaRowsPerBlock - 1) / orbm::kMfmaRowsPerBlock;
        hipLaunchKernelGGL(orbm::k_match_mfma, dim3(8 * nqb), dim3(orbm::kMfmaThreads), orbm::kMfmaLdsBytes, s, slot_ptr<const uint8_t>(h, S_BF_XDESC), xPitch, am, nqb, 1, (uint2*)nullptr, (int64_t)0);
    } else {
        hipLaunchKernelGGL(orbm::k_match_best2, dim3((nq + 255) / 256, 1, kMatchChunks), dim3(256), 0, s, q, t, 0, 0, kMatchChunks,
                           slot_ptr<uint2>(h, S_BF_BEST2), (int64_t)nq);
        hipLaunchKernelGGL(orbm::k_match_accept, dim3((nq + 255) / 256, 1), dim3(256), 0, s, aa, kMatchChunks, slot_ptr<const uint2>(h, S_BF_BEST2), (int64_t)nq);
    }
    hipLaunchKernelGGL(orbm::k_match_prune, dim3(1), dim3(256), 0, s, q, 0, check_ori, slot_ptr<int32_t>(h, S_BF_MATCH), (int64_t)nq,
                       slot_ptr<const uint8_t>(h, S_BF_BIN), d_hist, d_hist + 32);
    HIPCHK(hipGetLastError());
    int32_t nm = 0;
    HIPCHK(hipMemcpyAsync(match, slot_ptr(h, S_BF_MATCH), (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nm, d_hist + 32, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nmatches) *nmatches = nm;
    return ORBX_OK;
}

// ------------------------------------------------------------------ SearchByBoW
// One call = one packed upload from the pinned staging block (orbt_host.inc), two launches, one flag-polled download:
// no allocation, no pageable copy, no memset command (the tables' initial values ride in the block).  Until round 5 this
// was ~12 pageable copies + 3 memsets + a stream sync per call, three times what the search itself takes.
// one side of a BoW search: resident in HBM (d_* set: a device frame), or host arrays that ride in the staging block
struct BowSide {
    const uint8_t* d_desc; const float* d_ang; const int32_t *d_start, *d_idx;
    const uint32_t* node_id; int n_nodes; int n;
    const uint8_t* h_desc = nullptr; const float* h_ang = nullptr; const int32_t *h_start = nullptr, *h_idx = nullptr;
};

static int bow_core(orbm_handle* h, const BowSide& q, const uint8_t* qvalid, const BowSide& t, const uint8_t* tvalid,
                    float nnratio, int check_ori, int out_by_train, int32_t* match, int* nmatches);

extern "C" int orbm_search_by_bow(orbm_t* h,
                                  const uint8_t* qdesc, const float* qangle, const uint8_t* qvalid, int nq,
                                  const OrbmFeatVec* qfv,
                                  const uint8_t* tdesc, const float* tangle, const uint8_t* tvalid, int nt,
                                  const OrbmFeatVec* tfv,
                                  float nnratio, int check_ori, int out_by_train,
                                  int32_t* match, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (nq < 0 || nt < 0 || !qfv || !tfv || !match || (nq && (!qdesc || !qangle)) || (nt && (!tdesc || !tangle)))
        return fail(ORBX_E_INVALID, "bad argument");
    const int nout = out_by_train ? nt : nq;
    for (int i = 0; i < nout; i++) match[i] = -1;
    if (nmatches) *nmatches = 0;
    if (nq == 0 || nt == 0) return ORBX_OK;
    const int nqi = qfv->start[qfv->n_nodes], nti = tfv->start[tfv->n_nodes];
    for (int i = 0; i < nqi; i++) if (qfv->idx[i] < 0 || qfv->idx[i] >= nq) return fail(ORBX_E_INVALID, "query feature index out of range");
    for (int i = 0; i < nti; i++) if (tfv->idx[i] < 0 || tfv->idx[i] >= nt) return fail(ORBX_E_INVALID, "train feature index out of range");
    BowSide q = {nullptr, nullptr, nullptr, nullptr, qfv->node_id, qfv->n_nodes, nq};
    q.h_desc = qdesc; q.h_ang = qangle; q.h_start = qfv->start; q.h_idx = qfv->idx;
    BowSide t = {nullptr, nullptr, nullptr, nullptr, tfv->node_id, tfv->n_nodes, nt};
    t.h_desc = tdesc; t.h_ang = tangle; t.h_start = tfv->start; t.h_idx = tfv->idx;
    return bow_core(h, q, qvalid, t, tvalid, nnratio, check_ori, out_by_train, match, nmatches);
}

// ------------------------------------------------------------------ grid + SearchByProjection
// grid of n device-resident keys into (d_cnt, d_start, d_fill: ncell(+1) ints, d_idx: n ints), on stream s
static int grid_build_device(const OrbmGrid* grid, const orbm::KeyDev* dk, int n, int32_t* d_cnt, int32_t* d_start,
                             int32_t* d_fill, int32_t* d_idx, hipStream_t s, orbm::GridDev& gd)
{
    const int ncell = grid->cols * grid->rows;
    gd.minX = grid->minX; gd.minY = grid->minY; gd.invW = grid->invW; gd.invH = grid->invH; gd.cols = grid->cols; gd.rows = grid->rows;
    HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)ncell * 4, s));
    HIPCHK(hipMemsetAsync(d_fill, 0, (size_t)ncell * 4, s));
    if (n) hipLaunchKernelGGL(orbm::k_grid_count, dim3((n + 255) / 256), dim3(256), 0, s, gd, dk, n, d_cnt);
    hipLaunchKernelGGL(orbm::k_scan_small, dim3(1), dim3(1024), 0, s, (const int32_t*)d_cnt, ncell, d_start);
    if (n) {
        hipLaunchKernelGGL(orbm::k_grid_fill, dim3((n + 255) / 256), dim3(256), 0, s, gd, dk, n, (const int32_t*)d_start, d_fill, d_idx);
        hipLaunchKernelGGL(orbm::k_grid_sort, dim3((ncell + 255) / 256), dim3(256), 0, s, ncell, (const int32_t*)d_start, d_idx);
    }
    HIPCHK(hipGetLastError());
    return ORBX_OK;
}

static int orbm_build_grid(orbm_handle* h, const OrbmGrid* grid, const OrbxKeyPoint* keys, int n, orbm::GridDev& gd)
{
    if (!grid || grid->cols < 1 || grid->rows < 1 || grid->cols * grid->rows > (1 << 20)) return fail(ORBX_E_INVALID, "bad grid");
    int rc;
    const int ncell = grid->cols * grid->rows;
    if ((rc = orbm_reserve(h, {{G_KEYS, (size_t)std::max(n, 1) * sizeof(OrbxKeyPoint)}, {G_CNT, (size_t)ncell * 4}, {G_START, (size_t)(ncell + 1) * 4},
                               {G_FILL, (size_t)ncell * 4}, {G_IDX, (size_t)std::max(n, 1) * 4}}))) return rc;
    hipStream_t s = h->stream;
    if (n) HIPCHK(hipMemcpyAsync(slot_ptr(h, G_KEYS), keys, (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyHostToDevice, s));
    return grid_build_device(grid, slot_ptr<const orbm::KeyDev>(h, G_KEYS), n, slot_ptr<int32_t>(h, G_CNT), slot_ptr<int32_t>(h, G_START),
                             slot_ptr<int32_t>(h, G_FILL), slot_ptr<int32_t>(h, G_IDX), s, gd);
}

extern "C" int orbm_features_in_area(orbm_t* h, const OrbmGrid* grid, const OrbxKeyPoint* keys_un, int n,
                                     float x, float y, float r, int minLevel, int maxLevel,
                                     int32_t* out, int cap, int* n_out)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (n < 0 || (n && !keys_un) || cap < 0 || (cap && !out)) return fail(ORBX_E_INVALID, "bad argument");
    orbm::GridDev gd;
    if ((rc = orbm_build_grid(h, grid, keys_un, n, gd))) return rc;
    if ((rc = orbm_reserve(h, S_FA_OUT, (size_t)std::max(cap, 1) * 4)) || (rc = orbm_reserve(h, S_FA_CNT, 16))) return rc;
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(orbm::k_features_in_area, dim3(1), dim3(1), 0, s, gd, slot_ptr<const orbm::KeyDev>(h, G_KEYS),
                       slot_ptr<const int32_t>(h, G_START), slot_ptr<const int32_t>(h, G_IDX), x, y, r, minLevel, maxLevel,
                       slot_ptr<int32_t>(h, S_FA_OUT), cap, slot_ptr<int32_t>(h, S_FA_CNT));
    HIPCHK(hipGetLastError());
    int32_t cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, slot_ptr(h, S_FA_CNT), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_out) *n_out = cnt;
    if (cnt > cap) return fail(ORBX_E_CAPACITY, "%d features in area, capacity %d", cnt, cap);
    if (cnt) HIPCHK(hipMemcpy(out, slot_ptr(h, S_FA_OUT), (size_t)cnt * 4, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

#include "orbt_host.inc"

static int bow_core(orbm_handle* h, const BowSide& q, const uint8_t* qvalid, const BowSide& t, const uint8_t* tvalid,
                    float nnratio, int check_ori, int out_by_train, int32_t* match, int* nmatches)
{
    int rc;
    const int nq = q.n, nt = t.n;
    const int nout = out_by_train ? nt : nq;
    const bool qHost = q.h_desc != nullptr, tHost = t.h_desc != nullptr;
    const int nqi = qHost ? q.h_start[q.n_nodes] : 0, nti = tHost ? t.h_start[t.n_nodes] : 0;
    // upper bound of the node pairs the lock-step walk (ORBmatcher.cc:180-266) can find: the block is laid out before it runs
    const int pairCap = std::min(q.n_nodes, t.n_nodes);
    if (pairCap == 0) return ORBX_OK;
    Packer pk;
    const size_t oQd = qHost ? pk.take((size_t)nq * 32) : 0, oQa = qHost ? pk.take((size_t)nq * 4) : 0;
    const size_t oQs = qHost ? pk.take((size_t)(q.n_nodes + 1) * 4) : 0, oQi = qHost ? pk.take((size_t)std::max(nqi, 1) * 4) : 0;
    const size_t oTd = tHost ? pk.take((size_t)nt * 32) : 0, oTa = tHost ? pk.take((size_t)nt * 4) : 0;
    const size_t oTs = tHost ? pk.take((size_t)(t.n_nodes + 1) * 4) : 0, oTi = tHost ? pk.take((size_t)std::max(nti, 1) * 4) : 0;
    const size_t oQv = qvalid ? pk.take((size_t)nq) : 0, oTv = tvalid ? pk.take((size_t)nt) : 0;
    const size_t oPq = pk.take((size_t)pairCap * 4), oPt = pk.take((size_t)pairCap * 4);
    const size_t oMatched = pk.take((size_t)nt), oBin = pk.take((size_t)nout);
    const size_t oMatch = pk.take((size_t)nout * 4), oNm = pk.take(16);
    const size_t total = pk.off;
    if ((rc = orbm_pinned(h, total)) || (rc = orbm_reserve(h, T_STAGE, total))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    uint8_t* ds = slot_ptr<uint8_t>(h, T_STAGE);
    // lock-step walk of the two sorted node-id lists: host side, it only decides WHICH node pairs are searched
    int npairs = 0;
    {
        int32_t* pq = (int32_t*)(hs + oPq); int32_t* pt = (int32_t*)(hs + oPt);
        int a = 0, b = 0;
        while (a < q.n_nodes && b < t.n_nodes) {
            if (q.node_id[a] == t.node_id[b]) { pq[npairs] = a; pt[npairs] = b; npairs++; a++; b++; }
            else if (q.node_id[a] < t.node_id[b]) a++;
            else b++;
        }
    }
    if (npairs == 0) return ORBX_OK;
    if (qHost) {
        memcpy(hs + oQd, q.h_desc, (size_t)nq * 32); memcpy(hs + oQa, q.h_ang, (size_t)nq * 4);
        memcpy(hs + oQs, q.h_start, (size_t)(q.n_nodes + 1) * 4); if (nqi) memcpy(hs + oQi, q.h_idx, (size_t)nqi * 4);
    }
    if (tHost) {
        memcpy(hs + oTd, t.h_desc, (size_t)nt * 32); memcpy(hs + oTa, t.h_ang, (size_t)nt * 4);
        memcpy(hs + oTs, t.h_start, (size_t)(t.n_nodes + 1) * 4); if (nti) memcpy(hs + oTi, t.h_idx, (size_t)nti * 4);
    }
    if (qvalid) memcpy(hs + oQv, qvalid, (size_t)nq);
    if (tvalid) memcpy(hs + oTv, tvalid, (size_t)nt);
    memset(hs + oMatched, 0, oBin - oMatched);                 // matched flags
    memset(hs + oMatch, 0xFF, (size_t)nout * 4);               // match = -1
    memset(hs + oNm, 0, 16);
    hipStream_t s = h->stream;
    orbm::BowArgs a{};
    a.qdesc = qHost ? ds + oQd : q.d_desc; a.qang = qHost ? (const float*)(ds + oQa) : q.d_ang;
    a.qvalid = qvalid ? ds + oQv : nullptr;
    a.tdesc = tHost ? ds + oTd : t.d_desc; a.tang = tHost ? (const float*)(ds + oTa) : t.d_ang;
    a.tvalid = tvalid ? ds + oTv : nullptr;
    a.qstart = qHost ? (const int32_t*)(ds + oQs) : q.d_start; a.qidx = qHost ? (const int32_t*)(ds + oQi) : q.d_idx;
    a.tstart = tHost ? (const int32_t*)(ds + oTs) : t.d_start; a.tidx = tHost ? (const int32_t*)(ds + oTi) : t.d_idx;
    a.pairQ = (const int32_t*)(ds + oPq); a.pairT = (const int32_t*)(ds + oPt);
    a.matched = ds + oMatched;
    a.match = (int32_t*)(ds + oMatch); a.binOf = ds + oBin;
    a.nnratio = nnratio; a.thLow = 50; a.checkOri = check_ori; a.outByTrain = out_by_train;
    if ((rc = stage_up(h, s, ds, hs, total))) return rc;
    hipLaunchKernelGGL(orbm::k_bow_pairs, dim3(npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(orbm::k_prune_flat, dim3(1), dim3(256), 0, s, a.match, nout, check_ori, (const uint8_t*)a.binOf,
                       (int32_t*)(ds + oNm));
    HIPCHK(hipGetLastError());
    if ((rc = stage_down_wait(h, s, hs + oMatch, ds + oMatch, total - oMatch))) return rc;
    memcpy(match, hs + oMatch, (size_t)nout * 4);
    if (nmatches) *nmatches = *(const int32_t*)(hs + oNm);
    return ORBX_OK;
}

static int proj_check(orbm_handle* h, const OrbmProjParams* pp, const float* q_uvr, const int8_t* q_lvl, const uint8_t* qdesc,
                      const float* qangle, int nq, int nt, const uint8_t* t_occ, const int32_t* assign, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!pp || pp->mode < 3 || pp->mode > 6) return fail(ORBX_E_INVALID, "mode must be 3..6");
    if (nq < 0 || nt < 0 || (nq && (!q_uvr || !q_lvl || !qdesc)) || (nt && (!t_occ || !assign))) return fail(ORBX_E_INVALID, "bad argument");
    const bool useRot = pp->check_ori && (pp->mode == 4 || pp->mode == 5);
    if (useRot && nq && !qangle) return fail(ORBX_E_INVALID, "angles required for the rotation check");
    if (nmatches) *nmatches = 0;
    return ORBX_OK;
}

extern "C" int orbm_search_by_projection(orbm_t* h, const OrbmProjParams* pp,
                                         const float* q_uvr, const int8_t* q_lvl,
                                         const uint8_t* qdesc, const float* qangle,
                                         const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq,
                                         const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un,
                                         const uint8_t* tdesc, int nt,
                                         uint8_t* t_occ, int32_t* assign, int* nmatches)
{
    return orbm_search_by_projection_stereo(h, pp, q_uvr, nullptr, q_lvl, qdesc, qangle, qvalid, q_obs_pos, nq, grid, t_keys_un,
                                            tdesc, nullptr, nt, t_occ, assign, nmatches);
}

extern "C" int orbm_search_by_projection_stereo(orbm_t* h, const OrbmProjParams* pp,
                                                const float* q_uvr, const float* q_ur, const int8_t* q_lvl,
                                                const uint8_t* qdesc, const float* qangle,
                                                const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq,
                                                const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un,
                                                const uint8_t* tdesc, const float* t_uright, int nt,
                                                uint8_t* t_occ, int32_t* assign, int* nmatches)
{
    int rc = proj_check(h, pp, q_uvr, q_lvl, qdesc, qangle, nq, nt, t_occ, assign, nmatches);
    if (rc) return rc;
    if (nt && (!t_keys_un || !tdesc)) return fail(ORBX_E_INVALID, "bad argument");
    if ((q_ur != nullptr) != (t_uright != nullptr)) return fail(ORBX_E_INVALID, "q_ur and t_uright go together");
    if (q_ur && pp->mode != 3 && pp->mode != 4) return fail(ORBX_E_INVALID, "only modes 3 and 4 have a stereo gate");
    if (nq == 0 || nt == 0) return ORBX_OK;
    if (!grid || grid->cols < 1 || grid->rows < 1) return fail(ORBX_E_INVALID, "bad grid");
    const ProjTrainHost th = {grid, t_keys_un, tdesc};
    return proj_core(h, pp, q_uvr, q_lvl, qdesc, qangle, qvalid, q_obs_pos, nq, nullptr, &th, nt, t_occ, assign, nmatches, q_ur, t_uright);
}

// ------------------------------------------------------------------ SURVEY 8(f).3: the Frame's matcher-side state in HBM
// ONE arena block per frame (keysUn | desc | cnt | start | fill | idx | ang | rec | n | fvStart | fvIdx), taken from and
// returned to the owning handle's pool: the reference makes a Frame per image (Tracking.cc:251-259), so the per-frame path
// must not allocate.  No host sync either: the build is ordered before the owner's later calls by its stream, and a call
// that reads the frame from elsewhere (another thread's handle, a vocabulary's stream, a download) settles it first.
constexpr size_t kFramePoolBlocks = 16;   // free frame blocks a handle keeps for reuse
struct orbm_frame {
    orbm_handle* owner = nullptr;
    int n = 0;
    orbm::GridDev gd{};
    FrameBlock block{nullptr, 0};
    std::atomic<bool> settled{false};        // the build is known to have finished (a host sync happened after it); frames may be used from any thread
    orbm::KeyDev* d_keysUn = nullptr;
    uint8_t* d_desc = nullptr;
    int32_t *d_cnt = nullptr, *d_start = nullptr, *d_fill = nullptr, *d_idx = nullptr;
    uint4* d_rec = nullptr;                  // the features in grid order (orbt::FrameSetDev::rec), read by the projection searches
    int32_t* d_n = nullptr;
    float* d_ang = nullptr;                  // mvKeysUn[i].angle, contiguous (the BoW search reads angles by feature index)
    bool hasBow = false;                     // orbm_frame_compute_bow ran: FeatureVector as CSR, node ids on the host
    std::vector<uint32_t> fvNode;
    int fvNodes = 0;
    int32_t *d_fvStart = nullptr, *d_fvIdx = nullptr;
};

// a frame may be read through any handle of its device; one that is not its owner waits for the build once
static int frame_settle(orbm_frame* f)
{
    if (f->settled.load(std::memory_order_acquire)) return ORBX_OK;
    HIPCHK(hipStreamSynchronize(f->owner->stream));
    f->settled.store(true, std::memory_order_release);
    return ORBX_OK;
}
static int frame_usable(orbm_handle* h, orbm_frame* f)
{
    if (!f || !f->owner) return fail(ORBX_E_INVALID, "null frame");
    if (f->owner == h) return ORBX_OK;
    if (f->owner->device != h->device) return fail(ORBX_E_INVALID, "frame and matcher handle live on different devices");
    return frame_settle(f);
}

extern "C" int orbm_frame_destroy(orbm_frame_t* f)
{
    if (!f) return ORBX_OK;
    orbm_handle* h = f->owner;
    if (h) {
        // Every entry that reads a frame returns after its results have landed, so nothing is in flight on it but, at most,
        // its own build on the owner's stream -- and the block's next user is enqueued on that same stream.
        void* drop = nullptr;
        if (f->block.p) {
            std::lock_guard<std::mutex> lk(h->poolMu);
            h->freeBlocks.push_back(f->block);
            // a block that no later frame's size matches (need <= bytes <= 2 need) would sit here for the life of the thread: beyond
            // kFramePoolBlocks the OLDEST one goes back to the runtime (a steady stream of like-sized frames never gets here)
            if (h->freeBlocks.size() > kFramePoolBlocks) { drop = h->freeBlocks.front().p; h->freeBlocks.erase(h->freeBlocks.begin()); }
        }
        if (drop) { (void)hipSetDevice(h->device); (void)hipStreamSynchronize(h->stream); (void)hipFree(drop); }
        orbm_release(h);
    }
    delete f;
    return ORBX_OK;
}

extern "C" int orbm_frame_create(orbm_t* h, const OrbxKeyPoint* d_keys, const uint8_t* d_desc, int n,
                                 const float K[4], const float D[5], const OrbmGrid* grid, orbm_frame_t** out)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!out || n < 0 || (n && (!d_keys || !d_desc)) || !K || !D) return fail(ORBX_E_INVALID, "bad argument");
    if (!grid || grid->cols < 1 || grid->rows < 1 || grid->cols * grid->rows > (1 << 20)) return fail(ORBX_E_INVALID, "bad grid");
    *out = nullptr;
    const int ncell = grid->cols * grid->rows, nn = std::max(n, 1);
    const int ncap = align_up(nn, 512);   // blocks are recycled between frames of slightly different feature counts
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t oKeys = 0, oDesc = oKeys + pad((size_t)ncap * sizeof(OrbxKeyPoint)), oCnt = oDesc + pad((size_t)ncap * 32),
                 oStart = oCnt + pad((size_t)ncell * 4), oFill = oStart + pad((size_t)(ncell + 1) * 4), oIdx = oFill + pad((size_t)ncell * 4),
                 oAng = oIdx + pad((size_t)ncap * 4), oRec = oAng + pad((size_t)ncap * 4), oN = oRec + pad((size_t)ncap * 16),
                 oFvS = oN + 256, oFvI = oFvS + pad((size_t)(ncap + 1) * 4), need = oFvI + pad((size_t)ncap * 4);
    FrameBlock blk{nullptr, 0};
    {
        std::lock_guard<std::mutex> lk(h->poolMu);
        for (size_t i = 0; i < h->freeBlocks.size(); i++)
            if (h->freeBlocks[i].bytes >= need && h->freeBlocks[i].bytes <= 2 * need) { blk = h->freeBlocks[i]; h->freeBlocks[i] = h->freeBlocks.back(); h->freeBlocks.pop_back(); break; }
    }
    if (!blk.p) {
        HIPCHK(hipMalloc(&blk.p, need));
        blk.bytes = need;
        h->nDevAlloc++;
    }
    orbm_frame* f = new orbm_frame;
    f->owner = h; f->n = n; f->block = blk;
    h->refs++;
    uint8_t* b = (uint8_t*)blk.p;
    f->d_keysUn = (orbm::KeyDev*)(b + oKeys); f->d_desc = b + oDesc; f->d_cnt = (int32_t*)(b + oCnt); f->d_start = (int32_t*)(b + oStart);
    f->d_fill = (int32_t*)(b + oFill); f->d_idx = (int32_t*)(b + oIdx); f->d_ang = (float*)(b + oAng); f->d_rec = (uint4*)(b + oRec);
    f->d_n = (int32_t*)(b + oN); f->d_fvStart = (int32_t*)(b + oFvS); f->d_fvIdx = (int32_t*)(b + oFvI);
    hipStream_t s = h->stream;
    if (ncell <= kProjMaxCells && n <= 16384 && !((uintptr_t)d_desc & 15)) {
        // one launch: mvKeysUn, angles, descriptors, grid, grid-ordered records
        orbt::FrameBuildArgs fa{};
        fa.fs = {f->d_keysUn, f->d_desc, f->d_ang, f->d_start, f->d_idx, f->d_rec, f->d_n, nn, ncell};
        fa.srcKeys = (const orbm::KeyDev*)d_keys; fa.srcDesc = d_desc; fa.srcCount = nullptr; fa.srcCap = nn; fa.srcN = n;
        fa.slot0 = 0; fa.slotMod = 1;
        fa.grid = {grid->minX, grid->minY, grid->invW, grid->invH, grid->cols, grid->rows};
        fa.und = {K[0], K[1], K[2], K[3], D[0], D[1], D[2], D[3], D[4]};
        fa.undistort = D[0] != 0.0f;  // mvKeysUn = mvKeys otherwise (Frame.cc:406-410)
        f->gd = fa.grid;
        if ((rc = frame_build_launch(h, fa, 1))) { orbm_frame_destroy(f); return rc; }
    } else {
        if (n) {
            HIPCHK_OR(hipMemcpyAsync(f->d_desc, d_desc, (size_t)n * 32, hipMemcpyDeviceToDevice, s), orbm_frame_destroy(f));
            if (D[0] == 0.0f) {  // mvKeysUn = mvKeys (Frame.cc:406-410)
                HIPCHK_OR(hipMemcpyAsync(f->d_keysUn, d_keys, (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyDeviceToDevice, s), orbm_frame_destroy(f));
            } else {
                orbm::UndistArgs a = {K[0], K[1], K[2], K[3], D[0], D[1], D[2], D[3], D[4]};
                hipLaunchKernelGGL(orbm::k_undistort, dim3((n + 255) / 256), dim3(256), 0, s, (const orbm::KeyDev*)d_keys, n, a, f->d_keysUn);
            }
            HIPCHK_OR(hipMemcpy2DAsync(f->d_ang, 4, (const uint8_t*)d_keys + 12, sizeof(OrbxKeyPoint), 4, (size_t)n, hipMemcpyDeviceToDevice, s), orbm_frame_destroy(f));
        }
        if ((rc = grid_build_device(grid, f->d_keysUn, n, f->d_cnt, f->d_start, f->d_fill, f->d_idx, s, f->gd))) { orbm_frame_destroy(f); return rc; }
        // the grid-ordered records the projection searches walk (a frame this large is searched from memory: ProjCommon::big)
        if (n) hipLaunchKernelGGL(orbm::k_grid_records, dim3((n + 255) / 256), dim3(256), 0, s, (const orbm::KeyDev*)f->d_keysUn, (const int32_t*)f->d_start, ncell,
                                  (const int32_t*)f->d_idx, f->d_rec);
        HIPCHK_OR(hipGetLastError(), orbm_frame_destroy(f));
    }
    *out = f;
    return ORBX_OK;
}

extern "C" int orbm_frame_size(const orbm_frame_t* f) { return f ? f->n : 0; }

// waits until the frame's build has read the caller's d_keys / d_desc (orbm_frame_create returns with the build enqueued)
extern "C" int orbm_frame_settle(orbm_frame_t* f)
{
    if (!f || !f->owner) return fail(ORBX_E_INVALID, "null frame");
    int rc = orbm_check(f->owner);
    if (rc) return rc;
    return frame_settle(f);
}

extern "C" int orbm_frame_download_keys_un(orbm_frame_t* f, OrbxKeyPoint* keys_un)
{
    if (!f || !f->owner) return fail(ORBX_E_INVALID, "null frame");
    int rc = orbm_check(f->owner);
    if (rc) return rc;
    if (f->n && !keys_un) return fail(ORBX_E_INVALID, "bad argument");
    if ((rc = frame_settle(f))) return rc;
    if (f->n) HIPCHK(hipMemcpy(keys_un, f->d_keysUn, (size_t)f->n * sizeof(OrbxKeyPoint), hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbm_search_by_projection_frame(orbm_t* h, const OrbmProjParams* pp,
                                               const float* q_uvr, const int8_t* q_lvl,
                                               const uint8_t* qdesc, const float* qangle,
                                               const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq,
                                               orbm_frame_t* train, uint8_t* t_occ, int32_t* assign, int* nmatches)
{
    if (!train) return fail(ORBX_E_INVALID, "null frame");
    const int nt = train->n;
    int rc = proj_check(h, pp, q_uvr, q_lvl, qdesc, qangle, nq, nt, t_occ, assign, nmatches);
    if (rc || (rc = frame_usable(h, train))) return rc;
    if (nq == 0 || nt == 0) return ORBX_OK;
    const ProjTrain tr = {train->gd, train->d_keysUn, train->d_start, train->d_idx, train->d_desc, nt, train->d_rec};
    return proj_core(h, pp, q_uvr, q_lvl, qdesc, qangle, qvalid, q_obs_pos, nq, &tr, nullptr, nt, t_occ, assign, nmatches);
}

// train side of a windowed best search, resident in HBM
static int window_core(orbm_handle* h, const float* q_uvr, const float* q_ur, const int8_t* q_pred, const uint8_t* qdesc,
                       const uint8_t* qvalid, int nq, const ProjTrain& tr, const float* d_turight, const float* inv_sigma2,
                       int nlevels, int chi2, int32_t* best_idx, int32_t* best_dist)
{
    int rc;
    if ((rc = orbm_reserve(h, {{S_WIN_UVR, (size_t)nq * 12}, {S_WIN_UR, (size_t)nq * 4}, {S_WIN_PRED, (size_t)nq}, {S_WIN_QD, (size_t)nq * 32},
                               {S_WIN_QV, (size_t)nq}, {S_WIN_SIG, 64}, {S_WIN_BI, (size_t)nq * 4}, {S_WIN_BD, (size_t)nq * 4}}))) return rc;
    hipStream_t s = h->stream;
    if ((rc = slot_upload(h, S_WIN_UVR, q_uvr, (size_t)nq * 12)) || (rc = slot_upload(h, S_WIN_PRED, q_pred, (size_t)nq)) ||
        (rc = slot_upload(h, S_WIN_QD, qdesc, (size_t)nq * 32)) ||
        (q_ur && (rc = slot_upload(h, S_WIN_UR, q_ur, (size_t)nq * 4))) || (qvalid && (rc = slot_upload(h, S_WIN_QV, qvalid, (size_t)nq))) ||
        (chi2 && (rc = slot_upload(h, S_WIN_SIG, inv_sigma2, (size_t)nlevels * 4)))) return rc;
    orbm::WinArgs a{};
    a.grid = tr.gd;
    a.tkeys = tr.keys;
    a.cellStart = tr.cellStart; a.cellIdx = tr.cellIdx;
    a.quvr = slot_ptr<const float>(h, S_WIN_UVR); a.qur = q_ur ? slot_ptr<const float>(h, S_WIN_UR) : nullptr;
    a.qpred = slot_ptr<const int8_t>(h, S_WIN_PRED); a.qdesc = slot_ptr<const uint8_t>(h, S_WIN_QD);
    a.qvalid = qvalid ? slot_ptr<const uint8_t>(h, S_WIN_QV) : nullptr;
    a.tdesc = tr.desc; a.turight = d_turight;
    a.invSigma2 = slot_ptr<const float>(h, S_WIN_SIG);
    a.nq = nq; a.chi2 = chi2;
    a.bestIdx = slot_ptr<int32_t>(h, S_WIN_BI); a.bestDist = slot_ptr<int32_t>(h, S_WIN_BD);
    hipLaunchKernelGGL(orbm::k_window_best, dim3((nq + 63) / 64), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(best_idx, a.bestIdx, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(best_dist, a.bestDist, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

static int window_check(orbm_handle* h, const float* q_uvr, const float* q_ur, const int8_t* q_pred, const uint8_t* qdesc, int nq, int nt,
                        const float* t_uright, const float* inv_sigma2, int nlevels, int chi2, int32_t* best_idx, int32_t* best_dist)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (nq < 0 || nt < 0 || (nq && (!q_uvr || !q_pred || !qdesc || !best_idx || !best_dist))) return fail(ORBX_E_INVALID, "bad argument");
    if (chi2 && (!inv_sigma2 || nlevels < 1 || nlevels > 16)) return fail(ORBX_E_INVALID, "inv_sigma2 required for the chi-square test");
    if (chi2 && t_uright && !q_ur) return fail(ORBX_E_INVALID, "q_ur required with t_uright");
    for (int i = 0; i < nq; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    return ORBX_OK;
}

// ------------------------------------------------------------------ SURVEY 8(f).1 entry points
extern "C" int orbm_window_best(orbm_t* h, const float* q_uvr, const float* q_ur, const int8_t* q_pred,
                                const uint8_t* qdesc, const uint8_t* qvalid, int nq,
                                const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un, const uint8_t* tdesc,
                                const float* t_uright, int nt, const float* inv_sigma2, int nlevels, int chi2,
                                int32_t* best_idx, int32_t* best_dist)
{
    int rc = window_check(h, q_uvr, q_ur, q_pred, qdesc, nq, nt, t_uright, inv_sigma2, nlevels, chi2, best_idx, best_dist);
    if (rc) return rc;
    if (nt && (!t_keys_un || !tdesc)) return fail(ORBX_E_INVALID, "bad argument");
    if (nq == 0 || nt == 0) return ORBX_OK;
    ProjTrain tr;
    if ((rc = orbm_build_grid(h, grid, t_keys_un, nt, tr.gd))) return rc;
    if ((rc = orbm_reserve(h, S_WIN_TD, (size_t)nt * 32)) || (rc = orbm_reserve(h, S_WIN_TUR, (size_t)nt * 4))) return rc;
    if ((rc = slot_upload(h, S_WIN_TD, tdesc, (size_t)nt * 32)) || (t_uright && (rc = slot_upload(h, S_WIN_TUR, t_uright, (size_t)nt * 4)))) return rc;
    tr.keys = slot_ptr<const orbm::KeyDev>(h, G_KEYS);
    tr.cellStart = slot_ptr<const int32_t>(h, G_START); tr.cellIdx = slot_ptr<const int32_t>(h, G_IDX);
    tr.desc = slot_ptr<const uint8_t>(h, S_WIN_TD);
    tr.nt = nt;
    return window_core(h, q_uvr, q_ur, q_pred, qdesc, qvalid, nq, tr, t_uright ? slot_ptr<const float>(h, S_WIN_TUR) : nullptr, inv_sigma2,
                       nlevels, chi2, best_idx, best_dist);
}

// the same with a device-resident frame as train side (the KeyFrame of Fuse / SearchBySim3; mono: no right coordinates)
extern "C" int orbm_window_best_frame(orbm_t* h, const float* q_uvr, const int8_t* q_pred, const uint8_t* qdesc, const uint8_t* qvalid, int nq,
                                      orbm_frame_t* train, const float* inv_sigma2, int nlevels, int chi2,
                                      int32_t* best_idx, int32_t* best_dist)
{
    if (!train) return fail(ORBX_E_INVALID, "null frame");
    int rc = window_check(h, q_uvr, nullptr, q_pred, qdesc, nq, train->n, nullptr, inv_sigma2, nlevels, chi2, best_idx, best_dist);
    if (rc || (rc = frame_usable(h, train))) return rc;
    if (nq == 0 || train->n == 0) return ORBX_OK;
    ProjTrain tr = {train->gd, train->d_keysUn, train->d_start, train->d_idx, train->d_desc, train->n};
    return window_core(h, q_uvr, nullptr, q_pred, qdesc, qvalid, nq, tr, nullptr, inv_sigma2, nlevels, chi2, best_idx, best_dist);
}

// query side (F1) of SearchForInitialization resident in HBM: descriptors, angles, "octave 0" flags
static int init_core(orbm_handle* h, const float* q_xy, float window_size, const uint8_t* d_qdesc, const float* d_qang,
                     const uint8_t* d_qvalid, int nq, const ProjTrain& tr, float nnratio, int check_ori, int32_t* matches12, int* nmatches)
{
    int rc;
    const int nt = tr.nt;
    if ((size_t)nt * 2 > 150 * 1024) return fail(ORBX_E_UNSUPPORTED, "too many train features for the LDS distance table");
    // flatten: window query (x, y, windowSize), levels (0, 0); only octave-0 queries search (:424-426)
    std::vector<float> uvr((size_t)nq * 3);
    std::vector<int8_t> lvl((size_t)nq * 2, 0);
    for (int i = 0; i < nq; i++) { uvr[3 * i] = q_xy[2 * i]; uvr[3 * i + 1] = q_xy[2 * i + 1]; uvr[3 * i + 2] = window_size; }
    if ((rc = orbm_reserve(h, {{S_INI_UVR, (size_t)nq * 12}, {S_INI_LVL, (size_t)nq * 2}, {S_INI_CNT, (size_t)nq * 4}, {S_INI_OFF, (size_t)(nq + 1) * 4},
                               {S_INI_KEY, 16}, {S_INI_CIDX, 16}, {S_INI_M12, (size_t)nq * 4}, {S_INI_M21, (size_t)nt * 4}, {S_INI_NM, 16},
                               {S_INI_PUSHT, (size_t)nq * 4}, {S_INI_PUSHB, (size_t)nq}}))) return rc;
    hipStream_t s = h->stream;
    if ((rc = slot_upload(h, S_INI_UVR, uvr.data(), (size_t)nq * 12)) || (rc = slot_upload(h, S_INI_LVL, lvl.data(), (size_t)nq * 2))) return rc;
    orbm::ProjArgs a{};
    a.grid = tr.gd;
    a.tkeys = tr.keys;
    a.cellStart = tr.cellStart; a.cellIdx = tr.cellIdx;
    a.quvr = slot_ptr<const float>(h, S_INI_UVR); a.qlvl = slot_ptr<const int8_t>(h, S_INI_LVL);
    a.qdesc = d_qdesc; a.qang = d_qang;
    a.qvalid = d_qvalid; a.qobs = nullptr;
    a.tdesc = tr.desc;
    a.nq = nq; a.nt = nt;
    a.candCnt = slot_ptr<int32_t>(h, S_INI_CNT); a.candOff = slot_ptr<int32_t>(h, S_INI_OFF);
    a.candKey = nullptr; a.candIdx = nullptr;
    a.tocc = nullptr; a.assign = nullptr; a.nmatch = slot_ptr<int32_t>(h, S_INI_NM);
    a.pushT = slot_ptr<int32_t>(h, S_INI_PUSHT); a.pushBin = slot_ptr<uint8_t>(h, S_INI_PUSHB);
    a.mode = 7; a.nnratio = nnratio; a.checkOri = check_ori; a.thDist = 50;
    hipLaunchKernelGGL(orbm::k_proj_candidates, dim3((nq + 63) / 64), dim3(64), 0, s, a, 0);
    hipLaunchKernelGGL(orbm::k_scan_small, dim3(1), dim3(1024), 0, s, (const int32_t*)a.candCnt, nq, a.candOff);
    HIPCHK(hipGetLastError());
    int32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, a.candOff + nq, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = orbm_reserve(h, S_INI_KEY, (size_t)std::max(total, 1) * 4)) || (rc = orbm_reserve(h, S_INI_CIDX, (size_t)std::max(total, 1) * 4))) return rc;
    a.candKey = slot_ptr<uint32_t>(h, S_INI_KEY); a.candIdx = slot_ptr<int32_t>(h, S_INI_CIDX);
    hipLaunchKernelGGL(orbm::k_proj_candidates, dim3((nq + 63) / 64), dim3(64), 0, s, a, 1);
    const size_t lds = ((size_t)nt * 2 + 3) & ~(size_t)3;
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)orbm::k_init_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(orbm::k_init_resolve, dim3(1), dim3(64), lds, s, a, slot_ptr<int32_t>(h, S_INI_M12), slot_ptr<int32_t>(h, S_INI_M21));
    HIPCHK(hipGetLastError());
    int32_t nm = 0;
    HIPCHK(hipMemcpyAsync(matches12, slot_ptr(h, S_INI_M12), (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nm, a.nmatch, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nmatches) *nmatches = nm;
    return ORBX_OK;
}

extern "C" int orbm_search_for_initialization(orbm_t* h, const float* q_xy, float window_size,
                                              const OrbxKeyPoint* q_keys_un, const uint8_t* qdesc, int nq,
                                              const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un, const uint8_t* tdesc, int nt,
                                              float nnratio, int check_ori, int32_t* matches12, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (nq < 0 || nt < 0 || (nq && (!q_xy || !q_keys_un || !qdesc || !matches12)) || (nt && (!t_keys_un || !tdesc)))
        return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < nq; i++) matches12[i] = -1;
    if (nmatches) *nmatches = 0;
    if (nq == 0 || nt == 0) return ORBX_OK;
    ProjTrain tr;
    if ((rc = orbm_build_grid(h, grid, t_keys_un, nt, tr.gd))) return rc;
    std::vector<float> ang(nq);
    std::vector<uint8_t> valid(nq);
    for (int i = 0; i < nq; i++) { valid[i] = q_keys_un[i].octave <= 0; ang[i] = q_keys_un[i].angle; }
    if ((rc = orbm_reserve(h, {{S_INI_QD, (size_t)nq * 32}, {S_INI_QA, (size_t)nq * 4}, {S_INI_QV, (size_t)nq}, {S_INI_TD, (size_t)nt * 32}}))) return rc;
    if ((rc = slot_upload(h, S_INI_QD, qdesc, (size_t)nq * 32)) || (rc = slot_upload(h, S_INI_QA, ang.data(), (size_t)nq * 4)) ||
        (rc = slot_upload(h, S_INI_QV, valid.data(), (size_t)nq)) || (rc = slot_upload(h, S_INI_TD, tdesc, (size_t)nt * 32))) return rc;
    tr.keys = slot_ptr<const orbm::KeyDev>(h, G_KEYS);
    tr.cellStart = slot_ptr<const int32_t>(h, G_START); tr.cellIdx = slot_ptr<const int32_t>(h, G_IDX);
    tr.desc = slot_ptr<const uint8_t>(h, S_INI_TD);
    tr.nt = nt;
    return init_core(h, q_xy, window_size, slot_ptr<const uint8_t>(h, S_INI_QD), slot_ptr<const float>(h, S_INI_QA), slot_ptr<const uint8_t>(h, S_INI_QV), nq, tr,
                     nnratio, check_ori, matches12, nmatches);
}

/* SearchForInitialization between two device-resident frames (F1 = the initial frame, F2 = the current one) */
extern "C" int orbm_search_for_initialization_frames(orbm_t* h, const float* q_xy, float window_size, orbm_frame_t* f1, orbm_frame_t* f2,
                                                     float nnratio, int check_ori, int32_t* matches12, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!f1 || !f2) return fail(ORBX_E_INVALID, "null frame");
    if ((rc = frame_usable(h, f1)) || (rc = frame_usable(h, f2))) return rc;
    const int nq = f1->n, nt = f2->n;
    if (nq && (!q_xy || !matches12)) return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < nq; i++) matches12[i] = -1;
    if (nmatches) *nmatches = 0;
    if (nq == 0 || nt == 0) return ORBX_OK;
    if ((rc = orbm_reserve(h, S_INI_QV, (size_t)nq))) return rc;
    hipLaunchKernelGGL(orbm::k_octave0_flags, dim3((nq + 255) / 256), dim3(256), 0, h->stream, (const orbm::KeyDev*)f1->d_keysUn, nq, slot_ptr<uint8_t>(h, S_INI_QV));
    const ProjTrain tr = {f2->gd, f2->d_keysUn, f2->d_start, f2->d_idx, f2->d_desc, nt};
    return init_core(h, q_xy, window_size, f1->d_desc, f1->d_ang, slot_ptr<const uint8_t>(h, S_INI_QV), nq, tr, nnratio, check_ori, matches12, nmatches);
}

// one side of SearchForTriangulation resident in HBM (node ids on the host for the lock-step walk)
struct TriSide {
    const orbm::KeyDev* keys; const uint8_t* desc; int n;
    const int32_t* d_start; const int32_t* d_idx; const uint32_t* node_id; int n_nodes;
    const uint8_t* skip; const float* uright;   // host arrays (uploaded here), may be null
};

static int tri_core(orbm_handle* h, const TriSide& A, const TriSide& B, const float F12[9], float ex, float ey, const float* sf2,
                    const float* sigma2_2, int nlevels, int only_stereo, int check_ori, int32_t* matches12, int* nmatches)
{
    int rc;
    const int n1 = A.n, n2 = B.n;
    std::vector<int32_t> pa, pb;
    {
        int a = 0, b = 0;
        while (a < A.n_nodes && b < B.n_nodes) {
            if (A.node_id[a] == B.node_id[b]) { pa.push_back(a); pb.push_back(b); a++; b++; }
            else if (A.node_id[a] < B.node_id[b]) a++;
            else b++;
        }
    }
    const int npairs = (int)pa.size();
    if (npairs == 0) return ORBX_OK;
    if ((rc = orbm_reserve(h, {{S_TRI_S1, (size_t)n1}, {S_TRI_U1, (size_t)n1 * 4}, {S_TRI_S2, (size_t)n2}, {S_TRI_U2, (size_t)n2 * 4}, {S_TRI_PA, (size_t)npairs * 4},
                               {S_TRI_PB, (size_t)npairs * 4}, {S_TRI_M12, (size_t)n1 * 4}, {S_TRI_BIN, (size_t)n1}, {S_TRI_NMATCH, 4}}))) return rc;
    hipStream_t s = h->stream;
    if ((A.skip && (rc = slot_upload(h, S_TRI_S1, A.skip, (size_t)n1))) || (B.skip && (rc = slot_upload(h, S_TRI_S2, B.skip, (size_t)n2))) ||
        (A.uright && (rc = slot_upload(h, S_TRI_U1, A.uright, (size_t)n1 * 4))) || (B.uright && (rc = slot_upload(h, S_TRI_U2, B.uright, (size_t)n2 * 4))) ||
        (rc = slot_upload(h, S_TRI_PA, pa.data(), (size_t)npairs * 4)) || (rc = slot_upload(h, S_TRI_PB, pb.data(), (size_t)npairs * 4))) return rc;
    HIPCHK(hipMemsetAsync(slot_ptr(h, S_TRI_M12), 0xFF, (size_t)n1 * 4, s));
    orbm::TriArgs a{};
    a.k1 = A.keys; a.d1 = A.desc;
    a.skip1 = A.skip ? slot_ptr<const uint8_t>(h, S_TRI_S1) : nullptr; a.ur1 = A.uright ? slot_ptr<const float>(h, S_TRI_U1) : nullptr;
    a.k2 = B.keys; a.d2 = B.desc;
    a.skip2 = B.skip ? slot_ptr<const uint8_t>(h, S_TRI_S2) : nullptr; a.ur2 = B.uright ? slot_ptr<const float>(h, S_TRI_U2) : nullptr;
    a.start1 = A.d_start; a.idx1 = A.d_idx; a.start2 = B.d_start; a.idx2 = B.d_idx;
    a.pairA = slot_ptr<const int32_t>(h, S_TRI_PA); a.pairB = slot_ptr<const int32_t>(h, S_TRI_PB);
    for (int i = 0; i < 9; i++) a.F[i] = F12[i];
    a.ex = ex; a.ey = ey;
    for (int i = 0; i < 16; i++) { a.sf2[i] = i < nlevels ? sf2[i] : 0.f; a.sigma2[i] = i < nlevels ? sigma2_2[i] : 0.f; }
    a.onlyStereo = only_stereo; a.checkOri = check_ori;
    a.m12 = slot_ptr<int32_t>(h, S_TRI_M12); a.binOf = slot_ptr<uint8_t>(h, S_TRI_BIN);
    hipLaunchKernelGGL(orbm::k_triangulation_pairs, dim3(npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(orbm::k_prune_flat, dim3(1), dim3(256), 0, s, a.m12, n1, check_ori, (const uint8_t*)a.binOf, slot_ptr<int32_t>(h, S_TRI_NMATCH));
    HIPCHK(hipGetLastError());
    int32_t nm = 0;
    HIPCHK(hipMemcpyAsync(matches12, a.m12, (size_t)n1 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nm, slot_ptr<int32_t>(h, S_TRI_NMATCH), 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nmatches) *nmatches = nm;
    return ORBX_OK;
}

extern "C" int orbm_search_for_triangulation(orbm_t* h,
                                             const OrbxKeyPoint* k1, const uint8_t* d1, const uint8_t* skip1, const float* uright1, int n1,
                                             const OrbmFeatVec* fv1,
                                             const OrbxKeyPoint* k2, const uint8_t* d2, const uint8_t* skip2, const float* uright2, int n2,
                                             const OrbmFeatVec* fv2,
                                             const float F12[9], float ex, float ey, const float* sf2, const float* sigma2_2, int nlevels,
                                             int only_stereo, int check_ori, int32_t* matches12, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (n1 < 0 || n2 < 0 || !fv1 || !fv2 || !F12 || !sf2 || !sigma2_2 || nlevels < 1 || nlevels > 16 ||
        (n1 && (!k1 || !d1 || !matches12)) || (n2 && (!k2 || !d2)))
        return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (nmatches) *nmatches = 0;
    if (n1 == 0 || n2 == 0) return ORBX_OK;
    const int ni1 = fv1->start[fv1->n_nodes], ni2 = fv2->start[fv2->n_nodes];
    for (int i = 0; i < ni1; i++) if (fv1->idx[i] < 0 || fv1->idx[i] >= n1) return fail(ORBX_E_INVALID, "feature index out of range");
    for (int i = 0; i < ni2; i++) if (fv2->idx[i] < 0 || fv2->idx[i] >= n2) return fail(ORBX_E_INVALID, "feature index out of range");
    if ((rc = orbm_reserve(h, {{S_TRI_K1, (size_t)n1 * 28}, {S_TRI_D1, (size_t)n1 * 32}, {S_TRI_K2, (size_t)n2 * 28}, {S_TRI_D2, (size_t)n2 * 32},
                               {S_TRI_ST1, (size_t)(fv1->n_nodes + 1) * 4}, {S_TRI_I1, (size_t)std::max(ni1, 1) * 4},
                               {S_TRI_ST2, (size_t)(fv2->n_nodes + 1) * 4}, {S_TRI_I2, (size_t)std::max(ni2, 1) * 4}}))) return rc;
    if ((rc = slot_upload(h, S_TRI_K1, k1, (size_t)n1 * 28)) || (rc = slot_upload(h, S_TRI_D1, d1, (size_t)n1 * 32)) ||
        (rc = slot_upload(h, S_TRI_K2, k2, (size_t)n2 * 28)) || (rc = slot_upload(h, S_TRI_D2, d2, (size_t)n2 * 32)) ||
        (rc = slot_upload(h, S_TRI_ST1, fv1->start, (size_t)(fv1->n_nodes + 1) * 4)) || (ni1 && (rc = slot_upload(h, S_TRI_I1, fv1->idx, (size_t)ni1 * 4))) ||
        (rc = slot_upload(h, S_TRI_ST2, fv2->start, (size_t)(fv2->n_nodes + 1) * 4)) || (ni2 && (rc = slot_upload(h, S_TRI_I2, fv2->idx, (size_t)ni2 * 4)))) return rc;
    const TriSide A = {slot_ptr<const orbm::KeyDev>(h, S_TRI_K1), slot_ptr<const uint8_t>(h, S_TRI_D1), n1, slot_ptr<const int32_t>(h, S_TRI_ST1),
                       slot_ptr<const int32_t>(h, S_TRI_I1), fv1->node_id, fv1->n_nodes, skip1, uright1};
    const TriSide B = {slot_ptr<const orbm::KeyDev>(h, S_TRI_K2), slot_ptr<const uint8_t>(h, S_TRI_D2), n2, slot_ptr<const int32_t>(h, S_TRI_ST2),
                       slot_ptr<const int32_t>(h, S_TRI_I2), fv2->node_id, fv2->n_nodes, skip2, uright2};
    return tri_core(h, A, B, F12, ex, ey, sf2, sigma2_2, nlevels, only_stereo, check_ori, matches12, nmatches);
}

// SearchForTriangulation between two device-resident frames that ran orbm_frame_compute_bow (mono: no right coordinates)
extern "C" int orbm_search_for_triangulation_frames(orbm_t* h, orbm_frame_t* f1, const uint8_t* skip1, orbm_frame_t* f2, const uint8_t* skip2,
                                                    const float F12[9], float ex, float ey, const float* sf2, const float* sigma2_2, int nlevels,
                                                    int check_ori, int32_t* matches12, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!f1 || !f2) return fail(ORBX_E_INVALID, "null frame");
    if ((rc = frame_usable(h, f1)) || (rc = frame_usable(h, f2))) return rc;
    if (!f1->hasBow || !f2->hasBow) return fail(ORBX_E_INVALID, "orbm_frame_compute_bow has not run on both frames");
    if (!F12 || !sf2 || !sigma2_2 || nlevels < 1 || nlevels > 16 || (f1->n && !matches12)) return fail(ORBX_E_INVALID, "bad argument");
    for (int i = 0; i < f1->n; i++) matches12[i] = -1;
    if (nmatches) *nmatches = 0;
    if (f1->n == 0 || f2->n == 0 || f1->fvNodes == 0 || f2->fvNodes == 0) return ORBX_OK;
    const TriSide A = {f1->d_keysUn, f1->d_desc, f1->n, f1->d_fvStart, f1->d_fvIdx, f1->fvNode.data(), f1->fvNodes, skip1, nullptr};
    const TriSide B = {f2->d_keysUn, f2->d_desc, f2->n, f2->d_fvStart, f2->d_fvIdx, f2->fvNode.data(), f2->fvNodes, skip2, nullptr};
    return tri_core(h, A, B, F12, ex, ey, sf2, sigma2_2, nlevels, 0, check_ori, matches12, nmatches);
}

extern "C" int orbm_undistort_keypoints(orbm_t* h, const OrbxKeyPoint* keys, int n, const float K[4], const float D[5],
                                        OrbxKeyPoint* keys_un)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (n < 0 || !K || !D || (n && (!keys || !keys_un))) return fail(ORBX_E_INVALID, "bad argument");
    if (n == 0) return ORBX_OK;
    if (D[0] == 0.0f) { memcpy(keys_un, keys, (size_t)n * sizeof(OrbxKeyPoint)); return ORBX_OK; }  // mvKeysUn = mvKeys (Frame.cc:406-410)
    if ((rc = orbm_reserve(h, S_UND_IN, (size_t)n * sizeof(OrbxKeyPoint))) || (rc = orbm_reserve(h, S_UND_OUT, (size_t)n * sizeof(OrbxKeyPoint)))) return rc;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_UND_IN), keys, (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyHostToDevice, s));
    orbm::UndistArgs a = {K[0], K[1], K[2], K[3], D[0], D[1], D[2], D[3], D[4]};
    hipLaunchKernelGGL(orbm::k_undistort, dim3((n + 255) / 256), dim3(256), 0, s, slot_ptr<const orbm::KeyDev>(h, S_UND_IN), n, a,
                       slot_ptr<orbm::KeyDev>(h, S_UND_OUT));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(keys_un, slot_ptr(h, S_UND_OUT), (size_t)n * sizeof(OrbxKeyPoint), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

extern "C" int orbm_compute_stereo_from_rgbd(orbm_t* h, const OrbxKeyPoint* keys, const OrbxKeyPoint* keys_un, int n, const float* depth, int w, int hh,
                                             int stride, float mbf, float* uright, float* depth_out)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (n < 0 || w < 1 || hh < 1 || stride < w || !depth || (n && (!keys || !keys_un || !uright || !depth_out))) return fail(ORBX_E_INVALID, "bad argument");
    if (n == 0) return ORBX_OK;
    const size_t kb = (size_t)n * sizeof(OrbxKeyPoint), db = (size_t)stride * hh * 4;
    if ((rc = orbm_reserve(h, S_RGBD_KEYS, kb)) || (rc = orbm_reserve(h, S_RGBD_KEYSUN, kb)) || (rc = orbm_reserve(h, S_RGBD_DEPTH, db)) || (rc = orbm_reserve(h, S_RGBD_OUT, (size_t)n * 8))) return rc;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_RGBD_KEYS), keys, kb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_RGBD_KEYSUN), keys_un, kb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_RGBD_DEPTH), depth, db, hipMemcpyHostToDevice, s));
    float* out = slot_ptr<float>(h, S_RGBD_OUT);
    hipLaunchKernelGGL(orbm::k_stereo_from_rgbd, dim3((n + 255) / 256), dim3(256), 0, s, slot_ptr<const orbm::KeyDev>(h, S_RGBD_KEYS), slot_ptr<const orbm::KeyDev>(h, S_RGBD_KEYSUN), n,
                       slot_ptr<const float>(h, S_RGBD_DEPTH), w, hh, stride, mbf, out, out + n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(uright, out, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(depth_out, out + n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

extern "C" int orbm_distinctive_descriptors(orbm_t* h, const uint8_t* desc, const int32_t* start, int npoints, int32_t* best_idx)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (npoints < 0 || !start || (npoints && !best_idx)) return fail(ORBX_E_INVALID, "bad argument");
    if (npoints == 0) return ORBX_OK;
    const int total = start[npoints];
    int maxN = 0;
    for (int p = 0; p < npoints; p++) {
        if (start[p + 1] < start[p]) return fail(ORBX_E_INVALID, "start must be non-decreasing");
        maxN = std::max(maxN, start[p + 1] - start[p]);
    }
    if (total && !desc) return fail(ORBX_E_INVALID, "null descriptors");
    if ((size_t)maxN * 4 > 150 * 1024) return fail(ORBX_E_UNSUPPORTED, "more than 38400 observations of one map point");
    if ((rc = orbm_reserve(h, {{S_DIS_DESC, (size_t)std::max(total, 1) * 32}, {S_DIS_START, (size_t)(npoints + 1) * 4}, {S_DIS_BEST, (size_t)npoints * 4}}))) return rc;
    hipStream_t s = h->stream;
    if (total) HIPCHK(hipMemcpyAsync(slot_ptr(h, S_DIS_DESC), desc, (size_t)total * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(slot_ptr(h, S_DIS_START), start, (size_t)(npoints + 1) * 4, hipMemcpyHostToDevice, s));
    const size_t lds = (size_t)std::max(maxN, 1) * 4;
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)orbm::k_distinctive, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(orbm::k_distinctive, dim3(npoints), dim3(64), lds, s, slot_ptr<const uint8_t>(h, S_DIS_DESC), slot_ptr<const int32_t>(h, S_DIS_START),
                       slot_ptr<int32_t>(h, S_DIS_BEST));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(best_idx, slot_ptr(h, S_DIS_BEST), (size_t)npoints * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}
