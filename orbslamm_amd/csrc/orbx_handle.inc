// orbx_handle.inc -- extractor, part 1 of 7 (orbslamm_hip.hip lists them): environment switches, profiling spans, the host path's
// helpers (row staging, copy threads, the result block's layout, a batch's slot), the handle, its result-set accessors, check_device.

// ------------------------------------------------------------------ environment switches (their table: docs/experiments.md)
// ORBX_STAGE_NT, ORBX_LAT_PRIO, ORBX_SERIAL, ORBX_MATCH_POPCOUNT and ORBX_LAT_STREAMS are read by their first character (0 where
// the switch is not set), ORBX_COPY_THREADS as a number
static inline char env_char(const char* name) { const char* e = getenv(name); return e ? e[0] : 0; }
static inline int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }

// ------------------------------------------------------------------ profiling
enum ProfId { P_H2D = 0, P_RESIZE, P_FAST, P_DISTRIBUTE, P_BLUR, P_ORIENT_DESC, P_MATCH_BEST2, P_MATCH_ACCEPT, P_MATCH_PRUNE, P_D2H, P_COUNT };
static const char* kProfNames[P_COUNT] = {"h2d", "k_pyramid", "k_fast", "k_distribute", "k_blur",
                                          "k_orient_desc", "k_match_mfma", "k_match_accept", "k_match_prune", "d2h"};
struct ProfSpan { int id; hipEvent_t a, b; };

struct Profiler {
    bool on = false, cur = false;
    int only = -1;  // >= 0: only this kernel's launches are bracketed
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> pool;
    double ms[P_COUNT] = {0};
    int64_t launches[P_COUNT] = {0};
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    void begin(int id, hipStream_t s)
    {
        cur = on && (only < 0 || only == id);
        if (!cur) return;
        ProfSpan sp{id, get(), get()};
        (void)hipEventRecord(sp.a, s);
        spans.push_back(sp);
    }
    void end(hipStream_t s)
    {
        if (!cur) return;
        (void)hipEventRecord(spans.back().b, s);
    }
    void collect()
    {
        for (auto& sp : spans) {
            (void)hipEventSynchronize(sp.b);
            float t = 0;
            (void)hipEventElapsedTime(&t, sp.a, sp.b);
            ms[sp.id] += t;
            launches[sp.id]++;
            pool.push_back(sp.a);
            pool.push_back(sp.b);
        }
        spans.clear();
    }
    void destroy()
    {
        collect();
        for (auto e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

// ------------------------------------------------------------------ host-side helpers of the host-buffer entries
// Rows of a pageable caller frame into the pinned staging block.  The block is written once and read next by the device
// over the link, never by this core: streaming stores (no read-for-ownership of the destination's lines, nothing of the
// 30 MB per batch left in the caches) where the destination rows are 32-byte aligned; ORBX_STAGE_NT=0 keeps memcpy.
#if defined(__x86_64__)
__attribute__((target("avx2"))) static void stage_rows_nt(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t w, int rows)
{
    for (int y = 0; y < rows; y++) {
        uint8_t* d = dst + (size_t)y * dpitch;
        const uint8_t* s = src + (size_t)y * spitch;
        size_t x = 0;
        for (; x + 128 <= w; x += 128) {
            const __m256i a = _mm256_loadu_si256((const __m256i*)(s + x)), b = _mm256_loadu_si256((const __m256i*)(s + x + 32));
            const __m256i c = _mm256_loadu_si256((const __m256i*)(s + x + 64)), e = _mm256_loadu_si256((const __m256i*)(s + x + 96));
            _mm256_stream_si256((__m256i*)(d + x), a); _mm256_stream_si256((__m256i*)(d + x + 32), b);
            _mm256_stream_si256((__m256i*)(d + x + 64), c); _mm256_stream_si256((__m256i*)(d + x + 96), e);
        }
        for (; x + 32 <= w; x += 32) _mm256_stream_si256((__m256i*)(d + x), _mm256_loadu_si256((const __m256i*)(s + x)));
        if (x < w) memcpy(d + x, s + x, w - x);
    }
    _mm_sfence();
}
static const bool g_stageNt = env_char("ORBX_STAGE_NT") != '0' && __builtin_cpu_supports("avx2");
#else
static const bool g_stageNt = false;
static void stage_rows_nt(uint8_t*, size_t, const uint8_t*, size_t, size_t, int) {}
#endif
static inline void stage_rows(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t w, int rows)
{
    if (g_stageNt && w >= 128 && !(((uintptr_t)dst | dpitch) & 31)) { stage_rows_nt(dst, dpitch, src, spitch, w, rows); return; }
    for (int y = 0; y < rows; y++) memcpy(dst + (size_t)y * dpitch, src + (size_t)y * spitch, w);
}

// A few persistent threads for the bulk memcpys of the host path (pageable frames -> pinned staging, pinned results ->
// caller arrays): 30 MB per 64-frame batch is 3 ms on one core, which alone would cap the path at 20 k frames/s.
struct CopyPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cvWork, cvDone;
    std::function<void(int)> job;
    int nItems = 0, next = 0, pending = 0;
    uint64_t gen = 0;
    bool quit = false;
    void start(int n, int device)
    {
        for (int i = 0; i < n; i++)
            th.emplace_back([this, device] {
                (void)hipSetDevice(device);  // the latency path lets a worker send off the band it has just staged
                uint64_t seen = 0;
                std::unique_lock<std::mutex> lk(m);
                for (;;) {
                    cvWork.wait(lk, [&] { return quit || (gen != seen && next < nItems); });
                    if (quit) return;
                    while (next < nItems) {
                        const int i = next++;
                        lk.unlock();
                        job(i);
                        lk.lock();
                        if (--pending == 0) cvDone.notify_all();
                    }
                    seen = gen;
                }
            });
    }
    // run f(0) .. f(n-1), the caller takes part
    void run(int n, const std::function<void(int)>& f)
    {
        if (th.empty() || n <= 1) { for (int i = 0; i < n; i++) f(i); return; }
        std::unique_lock<std::mutex> lk(m);
        job = f; nItems = n; next = 0; pending = n; gen++;
        cvWork.notify_all();
        while (next < nItems) {
            const int i = next++;
            lk.unlock();
            f(i);
            lk.lock();
            --pending;
        }
        cvDone.wait(lk, [&] { return pending == 0; });
    }
    void stop()
    {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cvWork.notify_all();
        for (auto& t : th) t.join();
        th.clear();
    }
};

// The result block of a host-fed batch of B frames: [err, flag | n[B] | nmatch[B] | kps[B][maxKp] | desc[B][maxKp][32] |
// match[B][maxKp]], sections 64-byte aligned and back to back for the ticket's own B -- one contiguous piece that goes down
// in one copy (without matching: everything in front of `match`).
struct OutLayout { size_t n = 0, nm = 0, kp = 0, desc = 0, match = 0, bytes = 0; };
static OutLayout out_layout(size_t B, int maxKp)
{
    OutLayout l;
    size_t o = 64;                                                    // [0]: the device error flag, [1]: the latency mode's arrival flag
    l.n = o; o += ((B * 4) + 63) & ~(size_t)63;
    l.nm = o; o += ((B * 4) + 63) & ~(size_t)63;
    l.kp = o; o += B * (size_t)maxKp * 28; o = (o + 63) & ~(size_t)63;
    l.desc = o; o += B * (size_t)maxKp * 32;
    l.match = o; o += B * (size_t)maxKp * 4;
    l.bytes = o;
    return l;
}

// One batch in flight through the host-buffer entries (orbx_submit_batch .. orbx_release)
struct HostSlot {
    uint8_t* h_in = nullptr;    // pinned staging for pageable caller frames
    uint8_t* d_in = nullptr;    // the batch's frames in HBM (rows 64-byte aligned)
    uint8_t* h_out = nullptr;   // pinned results: [err | n[B] | nmatch[B] | kps[B][maxKp] | desc[B][maxKp][32] | match[B][maxKp]]
    uint8_t* d_out = nullptr;   // the same block in HBM: where the throughput mode gathers a batch's results for ONE copy down
    OutLayout lay;              // offsets of the sections for THIS ticket's B (the block is allocated for the handle's maxB)
    hipEvent_t evPacked = nullptr;  // gathered way down: the gather kernel has read the device result set (the copy of d_out follows)
    hipEvent_t evUp[4] = {nullptr, nullptr, nullptr, nullptr}, evOut = nullptr;  // evUp[p]: the frames of sub-batch p are in HBM
    int state = 0;              // 0 free, 1 in flight, 2 collected (a view is out)
    bool lat = false;           // results written by k_pack_host: h_out[1] holds ticket + 1 once they are all there
    int ticket = -1, B = 0;
    bool matched = false;
    bool into = false; const int32_t* intoN = nullptr; int intoCap = 0;   // orbx_submit_batch_into: results went to the caller's arrays
};

// ------------------------------------------------------------------ handle
struct orbx_handle {
    OrbxParams prm;
    int device = -1;          // -1: host-only handle (tables, no compute)
    int maxW = 0, maxH = 0, maxB = 0;
    int nlevels = 0;
    float mvScaleFactor[ORBX_MAXL], mvInvScaleFactor[ORBX_MAXL], mvLevelSigma2[ORBX_MAXL], mvInvLevelSigma2[ORBX_MAXL];
    int mnFeaturesPerLevel[ORBX_MAXL];
    int umax[16];

    // geometry of the currently configured frame shape
    Geom geom;
    int curW = 0, curH = 0;
    std::vector<Cell> cells;
    int tileStrideDw = 0, tileRows = 0, fastListCap = 0, tileRows0 = 0, fastListCap0 = 0, fastSmapPitch = 0, fastSmapPitch0 = 0;
    int nodeCap = 0;
    BlurTiles blurTiles;
    BlurRuns blurRuns;
    KpBlocks kpBlocks;
    int kpBlocksTotal = 0;
    int pyrBlocks = 0, pyrBufA = 0, pyrBufB = 0, pyrTabCap = 0;
    bool pyrFused = true;
    PyrRange* d_pyrRanges = nullptr; size_t pyrRangesCap = 0;

    hipStream_t stream = nullptr;
    static constexpr int kMaxSplit = 4;
    int nsplit = 2;                           // sub-batches per call (1, 3, 4 and more chains: docs/experiments.md)
    hipStream_t streamP[kMaxSplit] = {nullptr};  // pipeline stream of sub-batch p (p = 0 uses `stream`)
    hipEvent_t evStart = nullptr, evPart[kMaxSplit] = {nullptr}, evFast0[kMaxSplit] = {nullptr};
    bool partEverRan[kMaxSplit] = {false};
    int lastParts = 0;                        // evPart[0..lastParts) belong to the last extraction
    int prevB = 0, prevSplit = 0;             // its frame -> sub-batch partition (run_extract: join on a change)
    hipStream_t stream3 = nullptr;            // matching runs beside the next batch's pyramid/FAST
    hipEvent_t evPyr[kMaxSplit] = {nullptr}, evBlur[kMaxSplit] = {nullptr}, evMatch[2] = {nullptr, nullptr};
    bool matchPending[2] = {false, false};
    // Results (keypoints, descriptors, counts, +-32 descriptors) live in two sets of maxB + 1 slots used by alternate
    // extractions, so that the matching of batch n (set n & 1) never holds back the descriptors of batch n + 1
    int curSet = 0;
    bool serial = false;                      // ORBX_SERIAL=1: everything on one stream (profiling aid)
    hipStream_t matchStream[2] = {nullptr, nullptr}, outStream[2] = {nullptr, nullptr};  // where evMatch[s] / evOutOfSet[s] were recorded
    hipEvent_t evMatched[2] = {nullptr, nullptr};  // the batch's match tables are final (recorded before the roll of the previous frame)
    size_t partialSlots = 0;                  // (frame, chunk) slots of d_partial
    bool matchPopcount = false;               // ORBX_MATCH_POPCOUNT=1: the literal xor/popcount scan instead of the matrix-core scan (also what > 65 535 train features take)
    bool fuseExpand = true;                   // k_orient_desc writes the matrix-core scan's +-1 descriptors itself (false with the popcount scan)
    // device buffers (sized for maxW x maxH x maxB at create).  What dev_alloc / new_event made is noted here for free_device;
    // d_distScratch, d_pyrRanges and d_stereo are regrown later (regrow_exact) and freed beside the lists
    std::vector<void*> ownedBlocks; std::vector<hipEvent_t> ownedEvents;
    Geom* d_geom = nullptr;
    Cell* d_cells = nullptr; size_t cellsCap = 0;
    short4* d_tabs = nullptr; size_t tabsCap = 0;
    ResizeTabs tabs;
    size_t imgFrameBytes = 0;  // one frame of the host path's device staging (HostSlot::d_in)
    uint8_t* d_pyr = nullptr; size_t pyrCapFrame = 0;
    uint8_t* d_blur = nullptr; size_t blurCapFrame = 0;
    uint64_t* d_candRaw = nullptr; uint64_t* d_candA = nullptr; uint64_t* d_candB = nullptr; size_t candCapFrame = 0;
    int32_t* d_candCount = nullptr;
    uint32_t* d_distScratch = nullptr; size_t distScratchBytes = 0; bool distInLds = true; bool distBlurOk = false;
    int32_t* d_cellCount = nullptr;      // [maxB][cellsCap] survivors per FAST cell
    uint64_t* d_kept = nullptr; size_t keptCapFrame = 0;
    int32_t* d_keptCount = nullptr;
    int32_t* d_err = nullptr;            // [0] error flags of device-resident calls, [1] block counter of k_pack_host, [2] scratch word, [4 + slot] error flags of the host-fed batch in that slot
    int32_t* d_errCur = nullptr;         // where the kernels launched right now report (a host-fed batch: its slot's word, consumed and cleared by its own k_pack_host)
    int maxKp = 0;                       // output slot capacity (fixed at create)
    OrbxKeyPointDev* d_kps = nullptr;    // [maxB+1][maxKp]  slot 0 = previous frame of the stream
    uint8_t* d_desc = nullptr;           // [maxB+1][maxKp][32]
    int32_t* d_count = nullptr;          // [maxB+1]
    int32_t* d_match = nullptr;          // [2][maxB][maxKp]  one table per result set
    uint8_t* d_binOf = nullptr;          // [maxB][maxKp]
    int32_t* d_hist = nullptr;           // [maxB][32]
    int32_t* d_nmatch = nullptr;         // [2][maxB]
    uint2* d_partial = nullptr;          // [maxB][kMatchChunks][maxKp] chunk partials of the brute-force scan
    uint8_t* d_xdesc = nullptr;          // [maxB + 1] slots of +-32 byte descriptors in MFMA tile order (k_expand_desc)
    int64_t xPitch = 0, xAngOff = 0;   // bytes between slots of d_xdesc; where a slot's angle array begins
    // host-buffer entries: kSlots batches in flight (upload of n+1 | kernels of n | download of n-1), allocated at first use
#ifndef ORBX_HOST_SLOTS
#define ORBX_HOST_SLOTS 3
#endif
    static constexpr int kSlots = ORBX_HOST_SLOTS;
    HostSlot slot[kSlots];
    bool slotsReady = false;
    int nextTicket = 0;
    size_t outBytes = 0;  // a slot's result block (out_layout(maxB))
    hipStream_t streamUp = nullptr, streamDown = nullptr;  // upload / results of a batch submitted while nothing else is in flight
    hipStream_t streamUpQ = nullptr, streamDownQ = nullptr;  // the same for a batch submitted behind others: hardware queues of their own
    hipEvent_t evOutOfSet[2] = {nullptr, nullptr};         // the download that last read result set s
    std::vector<hipEvent_t> evExtReader[2];                // frame-set builds that read result set s and have not been waited for yet (events owned by the frame sets, which take them out again when they go)
    // latency mode with a frame set attached: the result kernel of the last submit is not in the queue yet -- the set's frame
    // build takes its work along (k_frame_build_pack); whoever else needs the results or the stream first launches it (flush_pack)
    bool packPending = false; PackArgs packPa{}; int packB = 0;
    int attachedSets = 0;                                  // frame sets attached to this handle (orbm_frameset_attach)
    int latMaxB = 2;                                       // calls of up to this many frames run the latency-mode chain (2; orbx_create_live: the handle's max_batch, up to 8)
    bool lastLat = false;                                  // the last extraction ran as one latency-mode chain on streamP[0]
    int latStreams = 0;                                    // latency mode on one stream (no event inside the chain) or two (level 0 beside the pyramid); 0 = by the number of latency handles alive on the device; ORBX_LAT_STREAMS fixes it
    int chainIdx = -1;                                     // latency handle: streamP[0] is chain stream chainIdx of the device's pool (not owned)
    bool countedLat = false;                               // counted in g_latHandles
    bool sharedStreams = false;                            // throughput handle: stream / streamP[] / stream3 belong to the device's pool (tput_streams_*)
    bool partLazy = false;                                 // evPart[0] of the last (latency-mode) extraction is not in the queue yet: whoever needs it records it on streamP[0] (flush_part_event)
    CopyPool pool;
    int matchSet = 0;                    // result set the last matching wrote (d_match / d_nmatch half)
    void* d_stereo = nullptr; size_t stereoBytes = 0;  // orbx_compute_stereo_matches: uRight | depth | SAD | count
    int lastB = 0;
    FrameSrc lastSrc{};
    Profiler prof;
};

static int match_prev_on(orbx_handle* h, hipStream_t s, float nnratio, int th_low, int check_ori, bool roll);
static int roll_prev_on(orbx_handle* h, hipStream_t s, int set);
// Up to how many frames per call a handle runs the latency-mode chain (everything in one queue, no event inside the chain,
// frames up through a copy kernel, results back by a flag-raising kernel).  Two = one robot's camera(s); a hub that puts the
// live frames of several robots through ONE chain (include/orbslamm_hub.hpp: the GPU executes about four queues at a time,
// so more than four robots per GPU share chains) creates its handle with up to kLatMaxBatchCeil (orbx_create_live).
constexpr int kLatMaxBatchCeil = 8;
static constexpr int lat_max_b() { return 2; }
static std::atomic<int> g_latHandles[64];   // latency handles (at most two frames per call) alive per device

// ------------------------------------------------------------------ result sets
static inline size_t set_slot0(const orbx_handle* h, int set) { return (size_t)set * ((size_t)h->maxB + 1); }
static inline OrbxKeyPointDev* r_kps(orbx_handle* h, int set) { return h->d_kps + set_slot0(h, set) * h->maxKp; }
static inline uint8_t* r_desc(orbx_handle* h, int set) { return h->d_desc + set_slot0(h, set) * h->maxKp * 32; }
static inline int32_t* r_count(orbx_handle* h, int set) { return h->d_count + set_slot0(h, set); }
static inline uint8_t* r_xdesc(orbx_handle* h, int set) { return h->d_xdesc + set_slot0(h, set) * (size_t)h->xPitch; }

static int check_device(orbx_handle* h)
{
    if (!h) return fail(ORBX_E_INVALID, "null handle");
    if (h->device < 0) return fail(ORBX_E_NO_DEVICE, "host-only handle: no HIP device bound, and there is no CPU fallback");
    HIPCHK(hipSetDevice(h->device));
    return ORBX_OK;
}
