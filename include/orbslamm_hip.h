/*
 * orbslamm_hip.h -- C ABI of the MI355X-native ORB front-end (liborbslamm_hip.so).
 *
 * Drop-in boundary for the per-frame hot path of HDaoud/ORBSLAMM.  Every entry
 * point names the reference interface it replaces (paths under
 * /root/reference/SingleRobotScenario/).  Plain pointers and sizes only; no
 * exceptions cross the ABI; every function returns 0 on success or a negative
 * ORBX_E_* code (orbx_last_error() gives the text).  All compute runs in HIP
 * kernels on gfx950 -- there is no CPU fallback; without a GPU every compute
 * entry returns ORBX_E_NO_DEVICE.
 *
 * Threading (mirrors the reference): one handle = one HIP stream;
 * calls on one handle must be serialised by the caller, distinct handles are
 * fully concurrent and may live on different devices.
 */
#ifndef ORBSLAMM_HIP_H
#define ORBSLAMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_MAX_LEVELS 16

enum {
    ORBX_OK = 0,
    ORBX_E_INVALID = -1,      /* bad argument */
    ORBX_E_NO_DEVICE = -2,    /* no HIP device / extension unusable: fail loudly, never fall back */
    ORBX_E_HIP = -3,          /* HIP runtime error (text in orbx_last_error) */
    ORBX_E_CAPACITY = -4,     /* caller buffer too small; nothing written past cap */
    ORBX_E_UNSUPPORTED = -5   /* image shape the reference itself cannot handle */
};

const char* orbx_last_error(void);
/* number of visible HIP devices (0 when none); never fails */
int orbx_device_count(void);
/* PCI bus id of a HIP device ("0000:c1:00.0", cap >= 16): /sys/bus/pci/devices/<id>/numa_node names the NUMA node whose
 * cores and memory sit next to it (a rank that feeds host frames should be pinned there) */
int orbx_device_pci_bus_id(int device, char* out, int cap);
/* the shader clock (MHz) the device runs at now UNDER LOAD, measured by a ~0.1 ms probe kernel that fills every SIMD (s_memtime
 * against the 100 MHz s_memrealtime in its first wave).  Diagnostics for multi-GPU launches (one robot per GPU, MultipleRobotsScenario/Examples/Monocular/
 * mono_kitti.cc:80-101): a rank that reports it right behind its timed steps tells a cold or throttled GPU from a slow
 * pipeline.  Synchronous; uses the device's null stream. */
int orbx_device_shader_clock_mhz(int device, float* mhz);

/* ---------------------------------------------------------------- extractor
 * replaces class ORBextractor (include/ORBextractor.h:45-111). */

/* ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels,
 *                            int iniThFAST, int minThFAST)  src/ORBextractor.cc:410-470 */
typedef struct {
    int32_t nfeatures;
    float scaleFactor;
    int32_t nlevels;
    int32_t iniThFAST;
    int32_t minThFAST;
} OrbxParams;

/* layout-identical to cv::KeyPoint as the reference fills it (28 bytes):
 * pt.x, pt.y, size, angle, response, octave, class_id (=-1)   src/ORBextractor.cc:841-847,1094-1103 */
typedef struct {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} OrbxKeyPoint;

typedef struct orbx_handle orbx_t;

/* Allocates every device buffer once (no allocation on the per-frame path).
 * max_w/max_h: largest frame; max_batch: frames in flight per call. */
int orbx_create(const OrbxParams* params, int max_w, int max_h, int max_batch, int device, orbx_t** out);
/* The same for the LIVE frames of up to max_cameras (1..8) cameras: every call of 1..max_cameras frames runs as ONE
 * latency-mode chain (one queue, frames up through a copy kernel, results behind a flag the caller polls) -- the handle
 * a hub creates that puts the frames of several robots' tracking threads through the GPU together
 * (include/orbslamm_hub.hpp; MultipleRobotsScenario/Examples/Monocular/mono_kitti.cc:83-101 with more robots than the
 * GPU runs queues).  orbx_create keeps the latency mode to calls of one or two frames. */
int orbx_create_live(const OrbxParams* params, int max_w, int max_h, int max_cameras, int device, orbx_t** out);
void orbx_destroy(orbx_t* h);

/* GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors /
 * GetScaleSigmaSquares / GetInverseScaleSigmaSquares  (include/ORBextractor.h:60-83).
 * Each array receives nlevels floats; NULL pointers are skipped.  Works without a GPU. */
int orbx_levels(const orbx_t* h);
float orbx_scale_factor(const orbx_t* h);
int orbx_scale_tables(const orbx_t* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);
/* mnFeaturesPerLevel (src/ORBextractor.cc:435-446) and umax[16] (:452-469) */
int orbx_features_per_level(const orbx_t* h, int32_t* out);
int orbx_umax(const orbx_t* h, int32_t out[16]);
/* upper bound of keypoints one frame can yield (sum over levels of N_l + slack) */
int orbx_max_keypoints(const orbx_t* h);

/* void ORBextractor::operator()(InputArray image, InputArray mask,
 *        vector<KeyPoint>& keypoints, OutputArray descriptors)   src/ORBextractor.cc:1043-1105
 * image: 8-bit single channel, host memory (mask is ignored by the reference).
 * kps[cap], desc[cap*32]; *n_out = number of keypoints.  Empty image (w<=0||h<=0||!img):
 * returns ORBX_OK with outputs untouched, like the reference (:1046-1047) but *n_out = 0. */
int orbx_extract(orbx_t* h, const uint8_t* img, int w, int h_, int stride,
                 OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out);

/* Batched form: B independent frames of identical shape, host memory.
 * kps[B*cap], desc[B*cap*32], n_out[B].  Synchronous: = orbx_submit_batch + orbx_collect_batch. */
int orbx_extract_batch(orbx_t* h, const uint8_t* const* imgs, int B, int w, int h_, int stride,
                       OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out);

/* ---- pipelined host-buffer entry --------------------------------------------------------------------------------
 * What a multi-robot front-end does with Frame::ExtractORB (src/Frame.cc:247-253) + the match against the previous
 * frame: up to three batches of one stream in flight, the upload of batch n+1 and the download of batch n-1 running
 * (on two copy streams) beside the kernels of batch n.  Tickets are collected in submission order.
 *   - frames in memory from orbx_host_alloc_frames (pinned, rows 64-byte aligned: the device layout) are read by the
 *     DMA engine in place; other pinned / registered memory (orbx_host_register) goes through a strided DMA;
 *     pageable frames are first copied to the handle's pinned staging (row bands over a few threads).
 *     The caller must not touch the frames of a ticket before it has been collected.
 *   - match_prev: every frame is also matched against the previous frame of the stream (rule of
 *     orbx_match_prev_batch_device) and the match tables come back with the batch. */
typedef struct {
    int32_t match_prev;   /* != 0: match vs the previous frame of the stream */
    float nnratio;        /* 0.7 */
    int32_t th_low;       /* TH_LOW = 50 */
    int32_t check_ori;
} OrbxStreamOpts;
/* results of one ticket in handle-owned pinned host memory, valid until orbx_release(ticket) */
typedef struct {
    int32_t B, cap;
    const int32_t* n;         /* [B] keypoints per frame */
    const OrbxKeyPoint* kps;  /* [B][cap] */
    const uint8_t* desc;      /* [B][cap][32] */
    const int32_t* match;     /* [B][cap] index into the previous frame or -1; NULL without match_prev */
    const int32_t* nmatch;    /* [B] */
} OrbxBatchView;
int orbx_submit_batch(orbx_t* h, const uint8_t* const* imgs, int B, int w, int h_, int stride,
                      const OrbxStreamOpts* opts /* may be NULL: extract only */, int* ticket);
/* waits for the ticket; zero-copy view of its results */
int orbx_collect_view(orbx_t* h, int ticket, OrbxBatchView* view);
int orbx_release(orbx_t* h, int ticket);
/* waits, copies the exact n entries per frame to the caller's arrays (kps[B*cap], desc[B*cap*32], match[B*cap];
 * NULL pointers are skipped) and releases the ticket */
int orbx_collect_batch(orbx_t* h, int ticket, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out,
                       int32_t* match, int* nmatch);
/* synchronous form of the pair above (the per-frame drop-in entry when B = 1) */
int orbx_extract_match_batch(orbx_t* h, const uint8_t* const* imgs, int B, int w, int h_, int stride,
                             const OrbxStreamOpts* opts, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out,
                             int32_t* match, int* nmatch);
/* Results straight into the CALLER'S containers, no second pass on the host: the result kernel writes exactly n records
 * per frame into kps[B*cap], desc[B*cap*32], n[B] (and match[B*cap], nmatch[B] with match_prev) over the link.  The
 * arrays must be memory the device can address: from orbx_host_alloc, or registered once with orbx_host_register
 * (a std::vector<cv::KeyPoint>'s storage can be registered after reserve()).  A frame with more than cap keypoints
 * gets its first cap written, n[] holds the true count, orbx_collect returns ORBX_E_CAPACITY.  orbx_collect waits for
 * the ticket and releases it. */
typedef struct {
    OrbxKeyPoint* kps; uint8_t* desc; int32_t* n;
    int32_t* match; int32_t* nmatch;   /* may be NULL without match_prev */
    int32_t cap;
} OrbxBatchOut;
int orbx_submit_batch_into(orbx_t* h, const uint8_t* const* imgs, int B, int w, int h_, int stride,
                           const OrbxStreamOpts* opts, const OrbxBatchOut* out, int* ticket);
int orbx_collect(orbx_t* h, int ticket);
/* pinned (device-addressable, coherent) host memory for such arrays; orbx_host_free releases it */
int orbx_host_alloc(orbx_t* h, size_t bytes, void** p);
/* pinned host frames in the device layout (a cv::Mat can wrap them: cv::Mat(h, w, CV_8UC1, ptr, stride)) */
int orbx_host_alloc_frames(orbx_t* h, int B, int w, int h_, uint8_t** frames, int* stride, size_t* pitch);
int orbx_host_free(orbx_t* h, void* p);
/* pin caller-owned frame memory (e.g. a capture ring buffer) for in-place DMA */
int orbx_host_register(orbx_t* h, void* p, size_t bytes);
int orbx_host_unregister(orbx_t* h, void* p);

/* Device-resident form: frames already in HBM (d_imgs + f*frame_pitch, rows `stride`
 * bytes apart; base, stride and frame_pitch must be multiples of 4).  Results stay
 * in handle-owned HBM (see orbx_device_results); asynchronous on the handle's streams (orbx_sync waits). */
int orbx_extract_batch_device(orbx_t* h, const uint8_t* d_imgs, int B, int w, int h_,
                              int stride, size_t frame_pitch);
/* device pointers of the last batch: kps[B][cap], desc[B][cap][32], counts[B].  Results alternate between two
 * sets: the pointers are those of the batch just extracted and stay untouched until the next-but-one extraction. */
int orbx_device_results(orbx_t* h, OrbxKeyPoint** d_kps, uint8_t** d_desc, int32_t** d_counts, int* cap);
/* blocking D2H copy of one frame of the last batch */
int orbx_download(orbx_t* h, int frame, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out);

/* std::vector<cv::Mat> mvImagePyramid (include/ORBextractor.h:85): lazy D2H of one
 * level (tight rows, no 19 px border -- the border is never read on the mono path).
 * dst may be NULL to query the size.  blurred!=0 returns the 7x7 Gaussian-smoothed
 * working image the descriptors were sampled from (src/ORBextractor.cc:1085-1086). */
int orbx_pyramid_level(orbx_t* h, int frame, int level, int blurred, uint8_t* dst, int* w, int* h_);
/* void Frame::ComputeStereoMatches()   src/Frame.cc:466-638, on the frames the two extractors (left, right: same
 * device, same shape and parameters -- Tracking's mpORBextractorLeft / mpORBextractorRight) extracted last: row-band
 * candidates, best descriptor within one octave and the disparity range [-3, mbf/mb], 11-position SAD search on the
 * keypoint's pyramid level (the consumer of mvImagePyramid, :561,578), parabola sub-pixel fit, median-distance filter.
 * u_right[cap] = mvuRight, depth[cap] = mvDepth (-1: no match); *n_left = left keypoints. */
int orbx_compute_stereo_matches(orbx_t* left, orbx_t* right, int frame, float mb, float mbf,
                                float* u_right, float* depth, int cap, int* n_left);

/* per-stage dump for parity tests: FAST candidates of one level, packed records
 * (see DESIGN.md "candidate record"), unordered; returns count in *n */
int orbx_level_candidates(orbx_t* h, int frame, int level, uint64_t* dst, int cap, int* n);

/* waits for everything the handle has enqueued; returns the device error flag.  The handles of one device and process share
 * their pipeline streams (four for the batched mode, a pool of four chains for the one-frame-per-call mode), so this call --
 * like a call with a new frame shape, which synchronises before it re-configures -- also waits for the work OTHER handles
 * of the device have in those streams: correct, but a robot that syncs in its loop couples its latency to its neighbours'.
 * The results of a call are published behind flags / events of their own (orbx_collect_*, orbm_track_results): a steady
 * loop needs no orbx_sync. */
int orbx_sync(orbx_t* h);

/* Convenience for hosts that do not link HIP themselves (the reference does not):
 * device buffers for the device-resident entry points, on the handle's GPU.
 * orbx_upload is a blocking host->device copy. */
int orbx_device_alloc(orbx_t* h, size_t bytes, void** d_ptr);
int orbx_device_free(orbx_t* h, void* d_ptr);
int orbx_upload(orbx_t* h, void* d_dst, const void* h_src, size_t bytes);

/* "match vs previous frame" for the stream held by this handle:
 * frame f of the last extracted batch is matched against frame f-1 (frame 0 against
 * the last frame of the previous batch; no previous frame -> no matches).
 * Brute-force best/second Hamming over ALL previous-frame descriptors in index order,
 * accept best<=th_low && (float)best < nnratio*(float)second, rotation histogram and
 * three-maxima pruning exactly as ORBmatcher::SearchByBoW does (src/ORBmatcher.cc:230-287).
 * Results stay in HBM: match[B][cap] (int32, -1 = none), nmatch[B].
 * Call it once after every orbx_extract_batch_device of the stream: it also rolls the batch's last frame into
 * the previous-frame slot the next batch is matched against. */
int orbx_match_prev_batch_device(orbx_t* h, float nnratio, int th_low, int check_ori);
int orbx_device_matches(orbx_t* h, int32_t** d_match, int32_t** d_nmatch);
int orbx_download_matches(orbx_t* h, int frame, int32_t* match, int cap, int* nmatch);
/* forget the previous frame (start of a new stream).  A call with a frame shape other than the handle's current one does
 * the same: a new shape starts a new stream (the first frame of the new shape has no previous frame). */
int orbx_reset_stream(orbx_t* h);

/* per-kernel timing with HIP events on the handle's stream.  enable=1 starts
 * collecting (adds two event records per launch); orbx_profile_read returns the
 * accumulated milliseconds and launch count per kernel since the last reset. */
#define ORBX_PROF_MAX 16
typedef struct {
    int32_t n;
    const char* name[ORBX_PROF_MAX];
    double ms[ORBX_PROF_MAX];
    int64_t launches[ORBX_PROF_MAX];
} OrbxProfile;
/* serial != 0: every kernel of a call runs on the handle's main stream (no overlap of
 * blur / matching / sub-batches); used to time kernels in isolation. */
int orbx_set_serial(orbx_t* h, int serial);
int orbx_profile_enable(orbx_t* h, int enable);
/* bracket only the launches of one kernel (name as reported by orbx_profile_read; NULL = all again): the
 * event records between dependent launches cost ~4 % of a stream-overlapped batch, one kernel's ~1 % */
int orbx_profile_select(orbx_t* h, const char* kernel);
int orbx_profile_read(orbx_t* h, OrbxProfile* out, int reset);

/* Diagnostics: which kernels slow each other down when they share the GPU (tools/pair_overlap.py).
 * Kernel i is launched back to back on one stream while kernel j keeps a second stream busy; co_ms[i * n + j] = time per
 * launch of i beside j, alone_ms[i] = alone; nb = frames per launch.  Runs on the buffers of the last extracted and
 * matched batch.  lds_bytes / wg_threads / wgs: workgroup footprint and count of each kernel at that nb. */
int orbx_debug_pair_overlap(orbx_t* h, int nb, float target_ms, int* n_kernels, const char** names,
                            float* alone_ms, float* co_ms, int32_t* lds_bytes, int32_t* wg_threads, int32_t* wgs);

/* Diagnostics: the rate of plain pinned hipMemcpyAsync copies of up_bytes (host to device) and down_bytes (device to host) on
 * this box, each direction alone and both at once on two streams -- the ceiling the host-buffer entries are read against
 * (bench.py host_path.pcie_*).  GB/s of payload. */
int orbx_debug_link_rate(orbx_t* h, size_t up_bytes, size_t down_bytes, int reps, float* h2d_gbs, float* d2h_gbs,
                         float* both_up_gbs, float* both_down_gbs);

/* Diagnostics: the row copy the host-buffer entries stage pageable frames with (streaming stores where the destination
 * rows are 32-byte aligned, memcpy otherwise) -- `rows` rows of `w` bytes from src (pitch spitch) to dst (pitch dpitch).
 * Needs no device: the CPU suite holds it to a plain copy for odd widths, unaligned sources and row tails.
 * Returns 1 if the streaming form ran, 0 for memcpy, < 0 on a bad argument. */
int orbx_debug_stage_rows(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t w, int rows);

/* Diagnostics: the four constant matrix-core operands of the Gaussian (orbx_kernels.hip make_blur_ops), 4 x 64 lanes x 4
 * dwords into dst -- walk = 0: the one-tile kernel's, 1: the column walk's.  Needs no device: the CPU suite rebuilds the
 * tables from the tap list and the slot mapping.  steps_per_run (may be NULL): the longest run a column is cut into. */
int orbx_debug_blur_ops(int walk, uint32_t* dst, int* steps_per_run);

/* ---------------------------------------------------------------- matcher
 * replaces class ORBmatcher (include/ORBmatcher.h:37-102).  The object-graph
 * walking (MapPoint flags, mutex-guarded getters, camera projection) stays in the
 * C++ adapter; these entry points take the flattened arrays (host memory). */
typedef struct orbm_handle orbm_t;
int orbm_create(int device, orbm_t** out);
void orbm_destroy(orbm_t* h);
/* The reference builds an ORBmatcher as a STACK TEMPORARY at every call site (src/Tracking.cc:639, 809, 914, 1242, 1415,
 * 1454, src/LocalMapping.cc:215, 483, src/LoopClosing.cc:245, 603, MultiMapper.cc:180, 687) holding only (mfNNratio,
 * mbCheckOrientation) -- include/ORBmatcher.h:96-97.  The device state a search needs (queue, grow-only scratch, pinned
 * staging block, the pool of frame blocks) therefore belongs to the calling THREAD: this returns the thread's handle for
 * `device`, made at the thread's first call and released when the thread ends (frames made through it keep it alive).  Its
 * queue is one of the device's four shared chain streams, not one more queue per thread (same priority as the latency
 * extractors' chains: high, or normal under ORBX_LAT_PRIO=0).  The price of sharing: the handle's synchronous entries wait on
 * a stream that other robots' chains and matcher calls are queued on too -- with more than four robot threads on a device a
 * call can wait for another robot's work (latency coupling, never a wrong result).  A caller that wants a queue of its own
 * takes orbm_create.  Never pass the thread handle to orbm_destroy. */
int orbm_thread_handle(int device, orbm_t** out);
/* Allocation counters: device allocations (scratch growth + frame blocks) and pinned allocations of handle h (0 for a
 * null h), and the number of matcher handles the process has made.  A steady-state loop leaves all three unchanged. */
int orbm_alloc_stats(orbm_t* h, int64_t* device_allocs, int64_t* host_allocs, int64_t* handles_made);

/* static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)
 * src/ORBmatcher.cc:1649-1665.  dist[nq*nt], row-major. */
int orbm_distance_matrix(orbm_t* h, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* dist);

/* brute-force matcher on host arrays (same rule as orbx_match_prev_batch_device) */
int orbm_match_bruteforce(orbm_t* h, const uint8_t* qdesc, const float* qangle, int nq,
                          const uint8_t* tdesc, const float* tangle, int nt,
                          float nnratio, int th_low, int check_ori, int32_t* match, int* nmatches);

/* DBoW2::FeatureVector flattened to CSR (Thirdparty/DBoW2/DBoW2/FeatureVector.h:21-47):
 * node ids ascending, per-node feature-index lists in stored order. */
typedef struct {
    int32_t n_nodes;
    const uint32_t* node_id;
    const int32_t* start;   /* n_nodes + 1 */
    const int32_t* idx;
} OrbmFeatVec;

/* int ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)     src/ORBmatcher.cc:159-290 (out_by_train=1)
 * int ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)  src/ORBmatcher.cc:524-657 (out_by_train=0)
 * qvalid: query feature has a good MapPoint; tvalid (KF-KF form only): train feature has one.
 * match: nt entries (query index per train feature) if out_by_train else nq entries. */
int orbm_search_by_bow(orbm_t* h,
                       const uint8_t* qdesc, const float* qangle, const uint8_t* qvalid, int nq,
                       const OrbmFeatVec* qfv,
                       const uint8_t* tdesc, const float* tangle, const uint8_t* tvalid, int nt,
                       const OrbmFeatVec* tfv,
                       float nnratio, int check_ori, int out_by_train,
                       int32_t* match, int* nmatches);

/* Frame grid: Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea
 * src/Frame.cc:230-245, 382-392, 327-380 (KeyFrame::GetFeaturesInArea src/KeyFrame.cc:618-657) */
typedef struct {
    float minX, minY;   /* mnMinX, mnMinY */
    float invW, invH;   /* mfGridElementWidthInv, mfGridElementHeightInv */
    int32_t cols, rows; /* FRAME_GRID_COLS 64, FRAME_GRID_ROWS 48 */
} OrbmGrid;

/* SearchByProjection family (projection done by the caller):
 * mode 3: SearchByProjection(Frame&, const vector<MapPoint*>&, th)        src/ORBmatcher.cc:45-129
 * mode 4: SearchByProjection(Frame& Cur, const Frame& Last, th, bMono)    src/ORBmatcher.cc:1330-1472
 * mode 5: SearchByProjection(Frame&, KeyFrame*, set<MapPoint*>&, th, ORBdist) src/ORBmatcher.cc:1474-1601
 * mode 6: SearchByProjection(KeyFrame*, cv::Mat Scw, ...)                 src/ORBmatcher.cc:292-405
 * Per query: (u, v, radius), level window [minLevel,maxLevel] with GetFeaturesInArea's
 * convention, descriptor, angle (modes 4/5), valid, obs_pos (MapPoint::Observations()>0).
 * t_occ (in/out, nt): train feature must be skipped.  assign (in/out, nt): query index
 * holding train feature t, -1 = NULL.
 * Sizes (the reference's loops take any, its frames hold 1000-5000 features): up to 8192 train features the frame's grid and
 * the resolve's tables live in one CU's LDS; beyond -- up to 65535 features per frame and 65536 queries per call, the width
 * of a feature / query index in the candidate lists (ORBX_E_UNSUPPORTED above) -- the same lists and rounds run from memory
 * (slower; frames built by the general-size kernels).  orbv_transform / orbm_frameset_compute_bow: any number of descriptors
 * (the sort's keys in memory above 8192); orbx_compute_stereo_matches: 65535 keypoints per frame. */
typedef struct {
    int32_t mode;
    float nnratio;
    int32_t check_ori;
    int32_t th_dist;
} OrbmProjParams;
int orbm_search_by_projection(orbm_t* h, const OrbmProjParams* pp,
                              const float* q_uvr, const int8_t* q_lvl,
                              const uint8_t* qdesc, const float* qangle,
                              const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq,
                              const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un,
                              const uint8_t* tdesc, int nt,
                              uint8_t* t_occ, int32_t* assign, int* nmatches);

/* The same with the stereo / RGB-D gate of modes 3 and 4 (src/ORBmatcher.cc:91-96, :1409-1415): a train feature with
 * t_uright[t] > 0 (Frame::mvuRight) is skipped when |q_ur[q] - t_uright[t]| > radius of the query (q_uvr[3q+2]);
 * q_ur = MapPoint::mTrackProjXR (mode 3) resp. u - mbf * invzc (mode 4).  Both NULL = the mono call above. */
int orbm_search_by_projection_stereo(orbm_t* h, const OrbmProjParams* pp,
                                     const float* q_uvr, const float* q_ur, const int8_t* q_lvl,
                                     const uint8_t* qdesc, const float* qangle,
                                     const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq,
                                     const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un,
                                     const uint8_t* tdesc, const float* t_uright, int nt,
                                     uint8_t* t_occ, int32_t* assign, int* nmatches);
/* Optional hint of the drop-in members (include/ORBmatcher_hip.hpp): the train side of the NEXT orbm_search_by_projection(_stereo)
 * on this handle -- the very arrays, count and grid that call will pass -- is uploaded and its grid built NOW, asynchronously, so
 * that the device works while the caller walks its MapPoints (the reference's loop head, ORBmatcher.cc:53-76, :1355-1392: mutex-
 * guarded getters, ~100 us for a frame's worth).  The search compares pointers, count and grid with what was prepared and does
 * its own upload when they differ; one search per prepare.  The arrays must not change between the two calls. */
int orbm_projection_prepare(orbm_t* h, const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un, const uint8_t* tdesc, int nt);


/* ---- the remaining ORBmatcher entry points on the same primitive ---- */

/* Independent windowed best search, the device part of
 *   int ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, float th)               src/ORBmatcher.cc:827-975  (chi2 = 1)
 *   int ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, float, vector<MapPoint*>&)  :977-1102 (chi2 = 0)
 *   int ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, s12, R12, t12, th)   :1104-1328 (both passes, chi2 = 0)
 * Per projected map point: (u, v, radius), predicted level (window [pred-1, pred]), descriptor,
 * valid flag; optional stereo terms (q_ur, t_uright = mvuRight, NULL for mono).
 * inv_sigma2 = mvInvLevelSigma2 (nlevels floats, needed when chi2).  best_idx = -1 if none
 * (best_dist = 256).  The caller applies bestDist <= TH_LOW / TH_HIGH and edits the map. */
int orbm_window_best(orbm_t* h, const float* q_uvr, const float* q_ur, const int8_t* q_pred,
                     const uint8_t* qdesc, const uint8_t* qvalid, int nq,
                     const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un, const uint8_t* tdesc,
                     const float* t_uright, int nt, const float* inv_sigma2, int nlevels, int chi2,
                     int32_t* best_idx, int32_t* best_dist);

/* int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
 *                                         vector<int>& vnMatches12, int windowSize)   src/ORBmatcher.cc:407-522
 * q_xy = vbPrevMatched (nq x 2).  matches12[nq] = index in F2 or -1; the caller refreshes
 * vbPrevMatched from it (:517-519). */
int orbm_search_for_initialization(orbm_t* h, const float* q_xy, float window_size,
                                   const OrbxKeyPoint* q_keys_un, const uint8_t* qdesc, int nq,
                                   const OrbmGrid* grid, const OrbxKeyPoint* t_keys_un, const uint8_t* tdesc, int nt,
                                   float nnratio, int check_ori, int32_t* matches12, int* nmatches);

/* int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12,
 *              vector<pair<size_t,size_t>>& vMatchedPairs, bool bOnlyStereo)          src/ORBmatcher.cc:659-825
 * skip1/skip2: the feature already has a MapPoint; uright = mvuRight (NULL for mono);
 * F12 row-major; (ex, ey) = epipole in image 2 (:666-672, cv::Mat algebra stays in the caller);
 * sf2 / sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2.  matches12[n1] = index in KF2 or -1. */
int orbm_search_for_triangulation(orbm_t* h,
                                  const OrbxKeyPoint* k1, const uint8_t* d1, const uint8_t* skip1, const float* uright1, int n1,
                                  const OrbmFeatVec* fv1,
                                  const OrbxKeyPoint* k2, const uint8_t* d2, const uint8_t* skip2, const float* uright2, int n2,
                                  const OrbmFeatVec* fv2,
                                  const float F12[9], float ex, float ey, const float* sf2, const float* sigma2_2, int nlevels,
                                  int only_stereo, int check_ori, int32_t* matches12, int* nmatches);

/* ---- a Frame's matcher-side state held in HBM ------------------------------------------------
 * The tail of Frame::Frame (src/Frame.cc:196-210: UndistortKeyPoints + AssignFeaturesToGrid) run on DEVICE-resident
 * extractor output -- e.g. d_keys = kps + f*cap, d_desc = desc + f*cap*32 from orbx_device_results -- so that the
 * projection searches consume it without a round trip through the host.  The frame copies what it needs (the
 * extractor's result sets are reused two batches later) into ONE block taken from the creating handle's pool and given
 * back by orbm_frame_destroy (from any thread): a Frame per image allocates nothing in steady state, and neither call
 * waits for the device.  Any matcher handle of the same device may search a frame; the creating handle lives until its
 * last frame is destroyed.
 * LIFETIME OF THE INPUTS: orbm_frame_create returns with the build ENQUEUED on the creating handle's stream; d_keys and
 * d_desc must stay untouched until the build has read them -- i.e. until the first search, BoW or download on the frame
 * has returned (each returns after its own results, enqueued behind the build, have landed), or until
 * orbm_frame_settle(f).  A caller that recycles the input buffers at once (orbx_upload into them, the extractor's next
 * but one batch) calls orbm_frame_settle first; Tracking's shape -- create, then search -- needs nothing. */
typedef struct orbm_frame orbm_frame_t;
int orbm_frame_create(orbm_t* h, const OrbxKeyPoint* d_keys, const uint8_t* d_desc, int n,
                      const float K[4], const float D[5], const OrbmGrid* grid, orbm_frame_t** out);
int orbm_frame_destroy(orbm_frame_t* f);
int orbm_frame_size(const orbm_frame_t* f);
/* waits (once; later calls return at once) until the frame's build has finished reading d_keys / d_desc */
int orbm_frame_settle(orbm_frame_t* f);
/* mvKeysUn for the host side of Tracking (pose optimisation reads it) */
int orbm_frame_download_keys_un(orbm_frame_t* f, OrbxKeyPoint* keys_un);
/* orbm_search_by_projection with the frame as train side (CurrentFrame of modes 3-5, the KeyFrame of mode 6) */
int orbm_search_by_projection_frame(orbm_t* h, const OrbmProjParams* pp,
                                    const float* q_uvr, const int8_t* q_lvl, const uint8_t* qdesc, const float* qangle,
                                    const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq,
                                    orbm_frame_t* train, uint8_t* t_occ, int32_t* assign, int* nmatches);

/* rounds and candidates of the handle's last projection search (diagnostics: the queries of the reference's sequential
 * loop are resolved in parallel rounds, see orbt_kernels.hip) */
int orbm_last_search_stats(orbm_t* h, int* rounds, int* candidates);

/* ---- the Tracking-shaped path, batched and without host round trips (round 3) -----------------------------------
 * A frame set holds `slots` device-resident frames of at most `cap` features: mvKeysUn, descriptors, mGrid.
 *   orbm_frameset_build*: the tail of Frame::Frame (src/Frame.cc:196-210: UndistortKeyPoints + AssignFeaturesToGrid) for
 *     n frames in ONE launch from device-resident extractor output (frame i at d_keys + i*src_cap, d_desc + i*src_cap*32,
 *     d_counts[i]; counts are read on the device), into slots (slot0 + i) % slots.  Asynchronous.
 *   orbm_track_frames: int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool bMono)
 *     src/ORBmatcher.cc:1330-1472 as Tracking::TrackWithMotionModel calls it (src/Tracking.cc:925-936, th = 15 then 30,
 *     bMono = true), for npairs (CurrentFrame, LastFrame) slot pairs in ONE launch.  Every LastFrame feature is a query
 *     (as if it held a MapPoint with observations, none an outlier) projected with the identity pose: u, v =
 *     mvKeysUn[i].pt, skipped outside `bounds` (:1375-1378), radius = th * mvScaleFactors[octave], octave window
 *     [octave-1, octave+1] (:1381-1392) -- SURVEY.md 8(d)'s grid-windowed variant.  A caller with a pose uses
 *     orbm_search_by_projection_frame on the same data.  pp->mode must be 4.  Asynchronous.
 *   orbm_track_results: waits for the last (back = 0) or an earlier (back = 1 .. 3) orbm_track_frames; assign[p*cap + t] =
 *     LastFrame feature index held by CurrentFrame feature t (or -1), nmatches[p]; both point into pinned host memory the
 *     kernel wrote (four result sets in rotation: valid until three more calls have been issued).  A search whose
 *     candidates overflowed the set's arena is run again with a larger one -- a frame-to-frame search and a query search
 *     (orbm_track_local_points, orbm_track_frame_projected) alike; ORBX_E_CAPACITY when a slot it read has been rebuilt
 *     since, or a larger query search issued behind it reallocated its staging.
 * bounds = mnMinX, mnMaxX, mnMinY, mnMaxY (Frame::ComputeImageBounds); scale_factors = mvScaleFactors. */
typedef struct orbm_frameset orbm_frameset_t;
int orbm_frameset_create(orbm_t* h, int slots, int cap, const float K[4], const float D[5], const OrbmGrid* grid,
                         const float bounds[4], const float* scale_factors, int nlevels, orbm_frameset_t** out);
int orbm_frameset_destroy(orbm_frameset_t* fs);
int orbm_frameset_build(orbm_frameset_t* fs, int slot0, int n, const OrbxKeyPoint* d_keys, const uint8_t* d_desc,
                        const int32_t* d_counts, int src_cap);
/* the frames of the extractor's last batch (orbx_extract_batch_device / orbx_submit_batch), ordered behind its kernels on
 * the device; the extractor will not reuse that result set before the build has read it. */
int orbm_frameset_build_from_extractor(orbm_frameset_t* fs, int slot0, orbx_t* ex);
int orbm_frameset_sync(orbm_frameset_t* fs);
/* The live stream -- one frame per robot per call, what the reference's main loops do
 * (MultipleRobotsScenario/Examples/Monocular/mono_kitti.cc:80-101 -> Tracking::GrabImageMonocular, src/Tracking.cc:240-267):
 * after orbm_frameset_attach(fs, ex) the frame set's kernels are enqueued on the extractor's own stream, so that
 *   orbx_submit_batch(ex, one frame)  ->  orbm_frameset_build_from_extractor(fs, slot, ex)  ->  orbm_track_frames(fs, ...)
 * is ONE chain of kernels on the device: Frame::Frame (ExtractORB, UndistortKeyPoints, AssignFeaturesToGrid, src/Frame.cc:175-210)
 * followed by TrackWithMotionModel's SearchByProjection (src/Tracking.cc:925-936) with no host round trip and no cross-stream
 * hand-over in between; the keypoints / descriptors come back through the ticket (flag-polled), the match table through
 * orbm_track_results (flag-polled for up to 8 pairs).  The search of frame t needs only the pose PREDICTED from frame t-1
 * (mVelocity * mLastFrame.mTcw, src/Tracking.cc:905), so it can be submitted together with the frame.  ex = NULL detaches.
 * Attach before the first orbm_frameset_compute_bow.  Calls on the extractor and on the attached frame set must come from
 * one thread at a time (they share a stream). */
int orbm_frameset_attach(orbm_frameset_t* fs, orbx_t* ex);
/* mvKeysUn / descriptors of one slot for the host side (pose optimisation reads mvKeysUn) */
int orbm_frameset_download(orbm_frameset_t* fs, int slot, OrbxKeyPoint* keys_un, uint8_t* desc, int cap, int* n_out);
int orbm_track_frames(orbm_frameset_t* fs, const OrbmProjParams* pp, float th, const int32_t* cur_slots,
                      const int32_t* last_slots, int npairs);
/* int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th)   src/ORBmatcher.cc:45-129
 * as Tracking::SearchLocalPoints runs it on every frame (src/Tracking.cc:1242-1249: th = 1, or 3 shortly after a
 * relocalisation, nnratio 0.8), with the frame resident in slot `slot` of the set.  Per local MapPoint in view
 * (Frame::isInFrustum, src/Frame.cc:269-325): q_uvr = mTrackProjX, mTrackProjY, r = RadiusByViewingCos(mTrackViewCos) * th *
 * mvScaleFactors[mnTrackScaleLevel]; q_lvl = mnTrackScaleLevel - 1, mnTrackScaleLevel; its descriptor; qvalid =
 * mbTrackInView && !isBad (NULL: all); q_obs_pos = Observations() > 0 (NULL: all); t_occ[cap] = F.mvpMapPoints[t] holds a
 * MapPoint with observations (NULL: none).  One pinned upload, two launches, no sync: asynchronous like orbm_track_frames,
 * the table comes back through orbm_track_results as a search of ONE pair (assign[t] = index of the MapPoint taken by
 * feature t or -1; the caller writes F.mvpMapPoints).  pp->mode 3 (modes 4 - 6 run without the rotation check: there are no
 * query angles here).  nq <= slots * cap. */
int orbm_track_local_points(orbm_frameset_t* fs, int slot, const OrbmProjParams* pp, const float* q_uvr, const int8_t* q_lvl,
                            const uint8_t* qdesc, const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq, const uint8_t* t_occ);
/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono)
 * src/ORBmatcher.cc:1330-1472 as Tracking::TrackWithMotionModel calls it (src/Tracking.cc:925-936) with a REAL pose:
 * the caller projects LastFrame's MapPoints with CurrentFrame.mTcw (:1362-1378 -- cv::Mat algebra, stays on the host) and
 * passes, per LastFrame feature i < nq: q_uvr = u, v, radius = th * mvScaleFactors[octave]; q_lvl = the octave window
 * (:1381-1392); qvalid = holds a MapPoint that is no outlier, projects with positive depth into the image bounds
 * (:1349-1378); q_obs_pos (NULL: all); t_occ[cap] as orbm_track_local_points.  LastFrame's descriptors and angles
 * (rotation check, pp->check_ori) and CurrentFrame's grid stay in HBM: 14 bytes per feature go up.  pp->mode 4 (or 5: the
 * relocalisation search, same shape).  Asynchronous; the table comes back through orbm_track_results as ONE pair. */
int orbm_track_frame_projected(orbm_frameset_t* fs, int cur_slot, int last_slot, const OrbmProjParams* pp, const float* q_uvr,
                               const int8_t* q_lvl, const uint8_t* qvalid, const uint8_t* q_obs_pos, int nq, const uint8_t* t_occ);
int orbm_track_results(orbm_frameset_t* fs, int back, const int32_t** assign, const int32_t** nmatches, int* npairs, int* cap);
int orbm_track_stats(orbm_frameset_t* fs, int pair, int* rounds, int* candidates);

/* void Frame::UndistortKeyPoints()   src/Frame.cc:404-434  (cv::undistortPoints(mat, mat, mK, mDistCoef, Mat(), mK)).
 * K = fx, fy, cx, cy; D = k1, k2, p1, p2, k3.  D[0] == 0: plain copy (:406-410).  Only pt changes. */
int orbm_undistort_keypoints(orbm_t* h, const OrbxKeyPoint* keys, int n, const float K[4], const float D[5],
                             OrbxKeyPoint* keys_un);

/* void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth)   src/Frame.cc:641-663 (the RGB-D Frame constructor, :104-142).
 * depth: the CV_32F depth image (w x hh floats, rows `stride` floats apart, already scaled by mDepthMapFactor as Tracking::
 * GrabImageRGBD does, src/Tracking.cc:215-216); keys = mvKeys (the lookup uses the DISTORTED position, float -> int by
 * truncation like Mat::at<float>(v, u)), keys_un = mvKeysUn.  uright[i] = kpU.pt.x - mbf / d and depth_out[i] = d where
 * d > 0, else both -1.  A keypoint outside the depth image (the reference reads out of bounds) counts as d = 0. */
int orbm_compute_stereo_from_rgbd(orbm_t* h, const OrbxKeyPoint* keys, const OrbxKeyPoint* keys_un, int n, const float* depth, int w, int hh,
                                  int stride, float mbf, float* uright, float* depth_out);

/* void MapPoint::ComputeDistinctiveDescriptors()   src/MapPoint.cc:242-307, batched over map points.
 * desc = the observations' descriptors of all points back to back, start[npoints+1] = CSR.
 * best_idx[p] = index (inside point p's list) of the descriptor with the least median distance
 * to the others, -1 for a point without observations. */
int orbm_distinctive_descriptors(orbm_t* h, const uint8_t* desc, const int32_t* start, int npoints, int32_t* best_idx);

/* The descriptor text of the map file: `os << pKF->mDescriptors`, `os << pMP->GetDescriptor()`  src/MapSerializer.cc:344-347,
 * 429-431 (cv::Mat's stream operator, OpenCV 3.0 default formatter: "[%3d, %3d, ...;\n %3d, ...]").  Host-side
 * formatting of host data; needs no device.  out == NULL queries *len (bytes without the terminating 0). */
int orbm_descriptors_to_text(const uint8_t* desc, int n, int cols, char* out, size_t cap, size_t* len);
/* the inverse, for map loaders (desc == NULL counts the rows) */
int orbm_descriptors_from_text(const char* text, uint8_t* desc, int cap_rows, int cols, int* n_rows);

/* GetFeaturesInArea on the device grid, for tests: out[cap] indices in reference order */
int orbm_features_in_area(orbm_t* h, const OrbmGrid* grid, const OrbxKeyPoint* keys_un, int n,
                          float x, float y, float r, int minLevel, int maxLevel,
                          int32_t* out, int cap, int* n_out);

/* ---------------------------------------------------------------- vocabulary
 * replaces ORBVocabulary::transform as called by Frame::ComputeBoW (src/Frame.cc:395-402):
 *   void TemplatedVocabulary::transform(const vector<TDescriptor>&, BowVector&, FeatureVector&, int levelsup)
 *   Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194 (+ :1218-1259)
 * The tree is uploaded once; nodes come in loadFromTextFile order (:1338-1425): entry i is node
 * id i+1 (root = 0), leaves receive word ids in file order.  scoring/weighting are DBoW2's enums. */
typedef struct orbv_handle orbv_t;
int orbv_create(int device, int k, int L, int scoring, int weighting, int n_nodes,
                const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc /* n x 32 */,
                const double* weight, orbv_t** out);
/* bool TemplatedVocabulary::loadFromTextFile(const std::string&)  (ORBvoc.txt format) */
int orbv_load_text(int device, const char* path, orbv_t** out);
void orbv_destroy(orbv_t* v);
/* BowVector as (word id ascending, value); FeatureVector as CSR (node id ascending, feature
 * indices ascending).  Capacities: n for word_id/word_value/fv_node/fv_idx, n+1 for fv_start. */
int orbv_transform(orbv_t* v, const uint8_t* desc, int n, int levelsup,
                   uint32_t* word_id, double* word_value, int* n_words,
                   uint32_t* fv_node, int32_t* fv_start, int32_t* fv_idx, int* n_fv_nodes);

/* Frame::ComputeBoW (src/Frame.cc:394-402) on a device-resident frame: BowVector to the host (word id ascending,
 * value; capacity orbm_frame_size), FeatureVector kept with the frame.  Vocabulary and frame must share the device. */
int orbm_frame_compute_bow(orbm_frame_t* f, orbv_t* voc, int levelsup, uint32_t* word_id, double* word_value, int* n_words);
/* orbm_search_by_bow between two frames that ran orbm_frame_compute_bow (query = KeyFrame / pKF1, train = Frame / pKF2) */
int orbm_search_by_bow_frames(orbm_t* h, orbm_frame_t* q, const uint8_t* qvalid, orbm_frame_t* t, const uint8_t* tvalid,
                              float nnratio, int check_ori, int out_by_train, int32_t* match, int* nmatches);

/* ---- the BoW side of the Tracking-shaped path on a frame set (round 3) ----
 * orbm_frameset_compute_bow: void Frame::ComputeBoW() (src/Frame.cc:394-402: mpORBvocabulary->transform(vCurrentDesc, mBowVec,
 *   mFeatVec, 4)) for slots (slot0 + i) % slots, i < n, in two launches; asynchronous.  FeatureVectors stay in HBM;
 *   orbm_frameset_bow_vector hands one slot's mBowVec to the host (word id ascending, value).
 * orbm_bow_frames: int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 *   src/ORBmatcher.cc:159-290 as Tracking::TrackReferenceKeyFrame calls it (src/Tracking.cc:805-812), for npairs
 *   (KeyFrame slot, Frame slot) pairs in two launches; every KeyFrame feature counts as holding a good MapPoint.
 *   Asynchronous.  orbm_bow_results as orbm_track_results: match[p*cap + t] = KeyFrame feature matched to Frame feature
 *   t or -1, nmatches[p], in pinned host memory (four result sets in rotation). */
int orbm_frameset_compute_bow(orbm_frameset_t* fs, orbv_t* voc, int slot0, int n, int levelsup);
int orbm_frameset_bow_vector(orbm_frameset_t* fs, int slot, uint32_t* word_id, double* word_value, int cap, int* n_words);
int orbm_bow_frames(orbm_frameset_t* fs, const int32_t* kf_slots, const int32_t* frame_slots, int npairs, float nnratio, int check_ori);
int orbm_bow_results(orbm_frameset_t* fs, int back, const int32_t** match, const int32_t** nmatches, int* npairs, int* cap);

/* orbm_window_best with a device-resident frame as train side (the KeyFrame of Fuse / Fuse(Scw) / SearchBySim3; mono) */
int orbm_window_best_frame(orbm_t* h, const float* q_uvr, const int8_t* q_pred, const uint8_t* qdesc, const uint8_t* qvalid, int nq,
                           orbm_frame_t* train, const float* inv_sigma2, int nlevels, int chi2,
                           int32_t* best_idx, int32_t* best_dist);
/* orbm_search_for_triangulation between two device-resident frames that ran orbm_frame_compute_bow (mono);
 * skip1 / skip2 (host): the feature already has a MapPoint */
int orbm_search_for_triangulation_frames(orbm_t* h, orbm_frame_t* f1, const uint8_t* skip1, orbm_frame_t* f2, const uint8_t* skip2,
                                         const float F12[9], float ex, float ey, const float* sf2, const float* sigma2_2, int nlevels,
                                         int check_ori, int32_t* matches12, int* nmatches);

/* orbm_search_for_initialization between two device-resident frames (F1 = the initial frame, F2 = the current one);
 * q_xy = vbPrevMatched (host, F1 size), matches12: F1 size */
int orbm_search_for_initialization_frames(orbm_t* h, const float* q_xy, float window_size, orbm_frame_t* f1, orbm_frame_t* f2,
                                          float nnratio, int check_ori, int32_t* matches12, int* nmatches);

/* ---------------------------------------------------------------- keyframe database
 * replaces KeyFrameDatabase (src/KeyFrameDatabase.cc, identical in both scenarios) and ORBVocabulary::score
 * (DBoW2 L1Scoring::score, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp).  Results equal the reference bit for bit: the same
 * keyframes in the same order, the same float scores, the reference's stateful quirks included.
 * Only L1_NORM scoring (ORBvoc.txt's) is implemented: any other vocabulary is refused with ORBX_E_UNSUPPORTED.
 *
 * orbv_score: double ORBVocabulary::score(const BowVector& v1, const BowVector& v2); word ids ascending. */
int orbv_score(orbv_t* voc, const uint32_t* a_ids, const double* a_vals, int na, const uint32_t* b_ids, const double* b_vals, int nb, double* out);

/* A pool holds keyframes by slot (one per KeyFrame): its mBowVec in HBM and the six query fields of KeyFrame.h:162-167
 * (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore), which belong to the keyframe and so
 * persist across queries and across the databases over the pool.  They start at 0 (the reference leaves the two scores
 * uninitialised: 0.0f is this library's defined choice).  Slots grow on demand: orbk_pool_set_bow on slot s makes slots
 * [0, s] exist (a slot never given a BowVector has an empty one).  A slot's BowVector cannot change while a database
 * holds it.  Every pool and database call holds the pool's lock for its duration; calls from any thread are serialised.
 * orbk_pool_set_bow_from_frameset copies a frame set slot's mBowVec (orbm_frameset_compute_bow) device to device, in
 *   order with the frame set's stream.  The slot must have been transformed with the pool's vocabulary (else
 *   ORBX_E_INVALID).  The frame set is a handle of its matcher: as for every call on it, the caller serialises this one
 *   (and orbk_detect_relocalization_candidates_frameset) with the other calls on the frame set and its matcher.
 * BowVectors live in an arena that grows: a new BowVector for a slot reuses the slot's range when it fits, else it is
 *   appended (the old range stays unused); a frame set slot reserves the set's per-frame capacity.
 * orbk_pool_score: out[i] = (float)score(slot's mBowVec, others[i]'s) -- the minScore loop of LoopClosing::DetectLoop
 *   (src/LoopClosing.cc:127-147) and MultiMapper::DetectLoop (MultipleRobotsScenario/src/MultiMapper.cc:140-152).
 * orbk_pool_set_covisibility: the slot's GetBestCovisibilityKeyFrames(10) for orbk_detect_loop_batch and for queries
 *   given no neighbour callback.
 * orbk_pool_read_state: the six fields of slots [0, n) (any pointer may be NULL); ORBX_E_CAPACITY when cap < n. */
typedef struct orbk_pool orbk_pool_t;
typedef struct orbk_db orbk_db_t;
int orbk_pool_create(orbv_t* voc, int slots_hint, orbk_pool_t** out);
void orbk_pool_destroy(orbk_pool_t* pool);
int orbk_pool_size(orbk_pool_t* pool, int* n_slots);
int orbk_pool_set_bow(orbk_pool_t* pool, int slot, const uint32_t* word_id, const double* word_value, int n);
int orbk_pool_set_bow_from_frameset(orbk_pool_t* pool, int slot, orbm_frameset_t* fs, int fs_slot);
int orbk_pool_score(orbk_pool_t* pool, int slot, const int32_t* others, int n, float* out);
int orbk_pool_set_covisibility(orbk_pool_t* pool, int slot, const int32_t* best, int n /* <= 10 */);
int orbk_pool_read_state(orbk_pool_t* pool, uint64_t* reloc_query, int32_t* reloc_words, float* reloc_score,
                         uint64_t* loop_query, int32_t* loop_words, float* loop_score, int cap);

/* KeyFrameDatabase over a pool: add / erase / clear / size / empty as the reference (add twice = every shared word counts
 * twice, erase removes the earliest copy, size counts adds minus erases floored at 0, clear keeps that count). */
int orbk_db_create(orbk_pool_t* pool, orbk_db_t** out);
void orbk_db_destroy(orbk_db_t* db);
int orbk_db_add(orbk_db_t* db, int slot);
int orbk_db_erase(orbk_db_t* db, int slot);
int orbk_db_clear(orbk_db_t* db);
int orbk_db_size(orbk_db_t* db, int* n);
int orbk_db_empty(orbk_db_t* db, int* empty);
/* lScoreAndMatch of the database's last single query: the scored slots in list order and their float scores */
int orbk_db_last_scored(orbk_db_t* db, int32_t* slots, float* scores, int cap, int* n);

/* The neighbours of a scored keyframe at the point the reference reads them (pKFi->GetBestCovisibilityKeyFrames(10)):
 * writes at most 10 pool slots to out and returns how many, or a negative value to abort the query.  It runs while the
 * pool is locked and must not call into the pool or its databases.  NULL: the pool's covisibility table. */
typedef int (*orbk_neighbours_fn)(void* user, int32_t slot, int32_t* out);

/* vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F) (src/KeyFrameDatabase.cc:211-303): F->mnId = query_id,
 * F->mBowVec from host arrays or from a frame set slot.  out: candidate slots in the reference's order; ORBX_E_CAPACITY
 * with the true count in *n_out when cap is short. */
int orbk_detect_relocalization_candidates(orbk_db_t* db, uint64_t query_id, const uint32_t* word_id, const double* word_value, int n,
                                          orbk_neighbours_fn neighbours, void* user, int32_t* out, int cap, int* n_out);
int orbk_detect_relocalization_candidates_frameset(orbk_db_t* db, uint64_t query_id, orbm_frameset_t* fs, int fs_slot,
                                                   orbk_neighbours_fn neighbours, void* user, int32_t* out, int cap, int* n_out);
/* vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) (:97-209): pKF = slot, pKF->mnId = query_id,
 * connected = pKF->GetConnectedKeyFrames() */
int orbk_detect_loop_candidates(orbk_db_t* db, int slot, uint64_t query_id, const int32_t* connected, int n_connected, float min_score,
                                orbk_neighbours_fn neighbours, void* user, int32_t* out, int cap, int* n_out);
/* MultiMapper::DetectLoop's inner scan (MultiMapper.cc:117-157) for n keyframes: minScore from each keyframe's covisible
 * list (GetVectorCovisibleKeyFrames() without the bad ones, CSR cov_start / cov_idx), then DetectLoopCandidates with the
 * connected set (CSR conn_start / conn_idx) -- identical to the n queries issued one after another, enqueued with no
 * host synchronisation in between; neighbours from the pool's covisibility table.  Candidates of query q:
 * out[out_start[q] .. out_start[q + 1]); ORBX_E_CAPACITY (out_start complete) when out_start[n] > cap. */
int orbk_detect_loop_batch(orbk_db_t* db, int n, const int32_t* slots, const uint64_t* query_ids,
                           const int32_t* conn_start, const int32_t* conn_idx, const int32_t* cov_start, const int32_t* cov_idx,
                           int32_t* out_start, int32_t* out, int cap);

/* ---------------------------------------------------------------- Initializer
 * replaces Initializer (src/Initializer.cc): the H / F RANSAC and the two-view reconstruction of monocular map
 * initialisation.  ORBI_MODEL_HF is SingleRobotScenario's (FindHomography and FindFundamental, ReconstructH when
 * RH = SH/(SH+SF) > 0.45, else ReconstructF); ORBI_MODEL_F is MultipleRobotsScenario's (FindFundamental, ReconstructF).
 * Results equal the reference's bit for bit given the same sets (its OpenCV arithmetic is restated, unpinned: §2).
 *
 * orbi_create: Initializer(ReferenceFrame, sigma, iterations) with ReferenceFrame.mvKeysUn = keys1_un (host) and
 *   mK = [fx 0 cx; 0 fy cy; 0 0 1], K = (fx, fy, cx, cy); frame 1's Normalize is computed once here.  The handle runs on
 *   the matcher handle's device and stream and holds a reference to it.  orbi_create_frame takes mvKeysUn from a
 *   device-resident frame (copied device to device).
 * orbi_initialize: bool Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) with CurrentFrame.mvKeysUn =
 *   keys2_un; matches12 (host, n1 long): vMatches12 (-1: none); sets (host, iterations x 8): the RANSAC sets as indices
 *   into the compacted match list (the entries i with matches12[i] >= 0, in order), which the reference draws with
 *   DUtils::Random (Initializer.cc:80-97) -- the caller draws them the same way.  res: the return value, R21 / t21 and
 *   diagnostics.  p3d (n1 x 3) and triangulated (n1) are written only where the reference writes vP3D / vbTriangulated:
 *   on success (res->ok).  orbi_initialize_frame reads mvKeysUn from a device-resident frame.
 * Refusals (nothing computed): ORBX_E_UNSUPPORTED for fewer than 8 matches (the reference would draw from an empty
 *   vector; Tracking never calls it below 100), iterations above ORBI_MAX_ITERATIONS, or more than ORBI_MAX_FEATURES
 *   keys in a frame; ORBX_E_INVALID for a null argument, iterations < 1, an unknown model, a match index outside
 *   frame 2, or a set index outside [0, matches).
 * Defined outcome: when the model to reconstruct has best score 0 (no hypothesis beat score = 0.0) the result is false
 *   with every output untouched (the reference would run OpenCV on an empty cv::Mat). */
#define ORBI_MODEL_HF 0
#define ORBI_MODEL_F 1
#define ORBI_MAX_ITERATIONS 4096
#define ORBI_MAX_FEATURES 65535
typedef struct {
    int32_t ok;                /* Initialize's return value */
    int32_t reconstructed_h;   /* 1: ReconstructH ran; 0: ReconstructF ran (or neither: n_candidates == 0, rt_state == 0) */
    int32_t rt_state;          /* R21 / t21: 0 untouched, 1 emptied (ReconstructF's failure), 2 written */
    float R21[9], t21[3];      /* row-major 3x3, 3x1 (rt_state == 2) */
    float SH, SF, RH;          /* scores (SH = 0 and RH = 0 under ORBI_MODEL_F) */
    float H21[9], F21[9];      /* the winning hypotheses (zeros where no iteration beat 0) */
    int32_t it_H, it_F;        /* their iterations (-1: none) */
    int32_t inliers_H, inliers_F;
    int32_t n_matches;         /* N: the entries of matches12 >= 0 */
    int32_t n_inliers;         /* inliers of the model reconstructed */
    int32_t n_candidates;      /* 4 (F), 8 (H) or 0 (ReconstructH's singular-value test failed, or no model) */
    int32_t best;              /* the candidate whose points are returned (-1: none) */
    int32_t n_good[8];         /* CheckRT's nGood of every candidate */
    float parallax[8];         /* and its parallax (degrees) */
} OrbiResult;
typedef struct orbi_init orbi_t;
int orbi_create(orbm_t* h, const OrbxKeyPoint* keys1_un, int n1, const float K[4], float sigma, int iterations, int model, orbi_t** out);
int orbi_create_frame(orbm_t* h, orbm_frame_t* f1, const float K[4], float sigma, int iterations, int model, orbi_t** out);
int orbi_initialize(orbi_t* ini, const OrbxKeyPoint* keys2_un, int n2, const int32_t* matches12, const int32_t* sets,
                    OrbiResult* res, float* p3d, uint8_t* triangulated);
int orbi_initialize_frame(orbi_t* ini, orbm_frame_t* f2, const int32_t* matches12, const int32_t* sets,
                          OrbiResult* res, float* p3d, uint8_t* triangulated);
/* frame 1's size and its Normalize: (meanX, meanY, sX, sY) */
int orbi_size(orbi_t* ini, int* n1);
int orbi_normalization(orbi_t* ini, float out[4]);
void orbi_destroy(orbi_t* ini);

/* ---------------------------------------------------------------- Sim3Solver
 * replaces Sim3Solver (src/Sim3Solver.cc, the same in both scenarios): Horn's closed-form similarity from three
 * correspondences under RANSAC, as MultiMapper::Run and LoopClosing::ComputeSim3 use it on every loop / merge candidate.
 * Every hypothesis of every solver of a batch is evaluated in one chain (orbs_run); iterate / find are then replayed on
 * the host over the per-hypothesis table, with the reference's state.  Results equal the reference's bit for bit given
 * the same sets (its OpenCV arithmetic is restated, unpinned: §2); the binary64 atan2 / cos / sin of each hypothesis are
 * taken on the host through libm, as the reference takes them.
 *
 * orbs_create: the constructor after its pointer chasing.  The caller walks vpMatched12 (skipping null / bad points and
 *   negative GetIndexInKeyFrame) and passes the n survivors: idx1 = mvnIndices1 (positions in vpMatched12, n1 long),
 *   X1w / X2w (n x 3) = GetWorldPos of pMP1 / pMP2, Rcw / tcw = the keyframes' GetRotation / GetTranslation (row-major),
 *   K = (fx, fy, cx, cy) of mK, sigma2_1 / sigma2_2 = mvLevelSigma2[kp.octave].  Rcw*Xw + tcw, FromCameraToImage and the
 *   thresholds ((size_t)(9.210*sigma2): truncated, as mvnMaxError1/2 are vector<size_t>) are computed on the device.  It
 *   ends, as the constructor does, in SetRansacParameters(0.99, 6, 300).  The handle runs on the matcher handle's device
 *   and stream and holds a reference to it.
 * orbs_set_ransac: SetRansacParameters (libm on the host); orbs_max_iterations reads mRansacMaxIts back.  It resets
 *   mnIterations (not mnBestInliers, as in the reference) and drops the table.
 * orbs_run: every hypothesis 0 .. mRansacMaxIts-1 of every solver, in one chain of launches with one host step in the
 *   middle.  sets[c] (host, mRansacMaxIts x 3): the RANSAC sets of solvers[c] as indices into its n correspondences,
 *   which the reference draws with DUtils::Random inside iterate (Sim3Solver.cc:163-177; its draw can repeat a point) --
 *   the caller draws them the same way.  A solver with n < min_inliers never draws: its sets[c] may be null.  All solvers
 *   must belong to one matcher handle.  orbs_hypotheses copies a solver's table out.
 * orbs_iterate: cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers) over the table; find is
 *   orbs_iterate(mRansacMaxIts).  inliers (n1 bytes) is cleared, then set at idx1[i] for the inliers of the returning
 *   hypothesis (recomputed on the device for that hypothesis).  Needs orbs_run first unless n < min_inliers.
 * orbs_points: the constructor's products, n x 3 planes of 4 floats: (X1c, maxError1), (X2c, maxError2), (p1im1, p2im2).
 * Refusals (nothing computed): ORBX_E_UNSUPPORTED for more than ORBS_MAX_POINTS correspondences, more than
 *   ORBS_MAX_ITERATIONS iterations, or n < 3 with n >= min_inliers (the reference would draw from an emptied vector);
 *   ORBX_E_INVALID for a null argument, idx1 outside [0, n1), a set index outside [0, n), solvers of different handles
 *   or repeated in a batch, orbs_iterate / orbs_hypotheses without a table. */
#define ORBS_MAX_POINTS 65535
#define ORBS_MAX_ITERATIONS 4096
typedef struct {
    int32_t n_inliers;         /* mnInliersi */
    float s12;                 /* ms12i */
    float T12[16], R12[9], t12[3];   /* mT12i (row-major 4x4), mR12i, mt12i */
} OrbsHypothesis;
typedef struct {
    int32_t returned;          /* 1: iterate returned T12 (else the empty cv::Mat) */
    int32_t no_more;           /* bNoMore */
    int32_t n_inliers;         /* nInliers */
    int32_t hypothesis;        /* the iteration that returned (0-based), -1: none */
    int32_t iterations;        /* mnIterations after the call */
    int32_t best_inliers;      /* mnBestInliers after the call */
    int32_t has_best;          /* 1: some hypothesis has passed `>= mnBestInliers` (the best fields are written) */
    float T12[16];             /* the returned matrix (returned == 1) */
    float best_R[9], best_t[3], best_s;   /* GetEstimatedRotation / Translation / Scale */
} OrbsResult;
typedef struct orbs_solver orbs_t;
int orbs_create(orbm_t* h, int n1, const int32_t* idx1, int n, const float* X1w, const float* X2w, const float Rcw1[9],
                const float tcw1[3], const float Rcw2[9], const float tcw2[3], const float K1[4], const float K2[4],
                const float* sigma2_1, const float* sigma2_2, int fix_scale, orbs_t** out);
int orbs_set_ransac(orbs_t* s, double probability, int min_inliers, int max_iterations);
int orbs_max_iterations(orbs_t* s, int* iterations);
int orbs_size(orbs_t* s, int* n, int* n1);
int orbs_points(orbs_t* s, float* out);
int orbs_run(orbs_t* const* solvers, int count, const int32_t* const* sets);
int orbs_hypotheses(orbs_t* s, OrbsHypothesis* out, int cap, int* n_out);
int orbs_iterate(orbs_t* s, int n_iterations, OrbsResult* res, uint8_t* inliers);
/* host-clock milliseconds of the legs of the last orbs_run this solver took part in: upload + fit + quaternions down,
 * the host's libm step, rotations up + pose + score + table down (tools/sim3_bench.py) */
int orbs_last_run_ms(orbs_t* s, double ms[3]);
void orbs_destroy(orbs_t* s);

/* ---------------------------------------------------------------- PnPsolver
 * replaces PnPsolver (src/PnPsolver.cc, the same in both scenarios): EPnP from four correspondences under RANSAC with an
 * n-point Refine, as Tracking::Relocalization runs it on every relocalisation candidate of every lost frame.  Every
 * hypothesis of every solver of a frame is evaluated in one chain (orbp_run: fit, score, records, Refine of every record);
 * iterate / find are then replayed on the host over the per-hypothesis table, with the reference's state.  Results equal
 * the reference's bit for bit given the same sets (its OpenCV arithmetic is restated, unpinned: §2).
 *
 * orbp_create: the constructor after its pointer chasing.  The caller walks vpMapPointMatches (skipping null and bad
 *   points) and passes the n survivors: idx = mvKeyPointIndices (positions in vpMapPointMatches, n_all long), P2D (n x 2)
 *   = mvKeysUn[idx].pt, sigma2 (n) = mvLevelSigma2[kp.octave], P3Dw (n x 3) = GetWorldPos, K = (fx, fy, cx, cy).  It ends,
 *   as the constructor does, in SetRansacParameters(0.99, 8, 300, 4, 0.4, 5.991).  The handle runs on the matcher
 *   handle's device and stream and holds a reference to it.
 * orbp_create_frame: the same from a device-resident frame (orbm_frame_create): n_all is
 *   the frame's size, P2D and sigma2 are gathered on the device from its undistorted keys (pt, and level_sigma2[octave], a
 *   host table of n_levels entries): nothing of the frame crosses the link, the caller sends idx and P3Dw.
 * orbp_set_ransac: SetRansacParameters (libm on the host): min_inliers raised to (int)(N*epsilon) and to min_set, epsilon
 *   raised to min_inliers/N, pow(epsilon, 3) in the iteration count, mvMaxError = sigma2*th2 as a float product.  As in
 *   the reference it rewinds neither mnIterations nor the best; it drops the table.  orbp_max_iterations /
 *   orbp_min_inliers read mRansacMaxIts / mRansacMinInliers back.
 * orbp_run: hypotheses 0 .. n_sets[c]-1 of every solver, in one chain of launches.  sets[c] (host, n_sets[c] x 4): the
 *   RANSAC sets of solvers[c] as indices into its n correspondences, which the reference draws with DUtils::Random inside
 *   iterate (PnPsolver.cc:191-201; its draw can repeat a point) -- the caller draws them the same way.  iterate's loop is
 *   an OR (`mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`), so a solver can need up to
 *   mRansacMaxIts + nIterations - 1 hypotheses: n_sets[c] may exceed mRansacMaxIts (iterate(5) reaches
 *   mRansacMaxIts + 4).  A solver with n < min_inliers never draws: its sets[c] may be null.  All solvers must belong to
 *   one matcher handle.  A solver that has not iterated gets a new table; one that has iterated CONTINUES its table: the
 *   sets given are those of the hypotheses behind the last one it holds, the records go on from the table's largest, the
 *   state stays (what a caller does when the reference's loop runs past the sets drawn so far).
 *   orbp_hypotheses copies a solver's table out.
 * orbp_iterate: cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers) over the table; find is
 *   orbp_iterate(mRansacMaxIts).  inliers (n_all bytes) is cleared, then set at idx[i] for the inliers of the returned
 *   pose (Refine's, or the best's at exhaustion), recomputed on the device for that pose.  Needs orbp_run first unless
 *   n < min_inliers.  A call whose loop would step past the table returns ORBX_E_CAPACITY with the solver's state as
 *   before the call.
 * Refusals (nothing computed): ORBX_E_UNSUPPORTED for n == 0, min_set != 4, more than ORBP_MAX_POINTS correspondences,
 *   more than ORBP_MAX_ITERATIONS iterations, a table beyond 2 * ORBP_MAX_ITERATIONS hypotheses, orbp_run on a solver that
 *   has iterated and whose table orbp_set_ransac dropped; ORBX_E_INVALID for a null argument,
 *   idx outside [0, n_all), a set index outside [0, n), n_sets outside [1, 2 * ORBP_MAX_ITERATIONS], solvers of
 *   different handles or repeated in a batch, orbp_iterate / orbp_hypotheses without a table. */
#define ORBP_MAX_POINTS 65535
#define ORBP_MAX_ITERATIONS 4096
typedef struct {
    int32_t n_inliers;         /* mnInliersi */
    int32_t is_record;         /* 1: count >= mRansacMinInliers and > mnBestInliers: it became the running best */
    int32_t refine_inliers;    /* is_record: mnRefinedInliers of Refine() on its mask */
    int32_t refine_ok;         /* is_record: Refine()'s return (refine_inliers > mRansacMinInliers) */
    double R[9], t[3];         /* mRi (row-major), mti */
    double refine_R[9], refine_t[3];   /* is_record: mRi, mti after Refine() */
} OrbpHypothesis;
typedef struct {
    int32_t returned;          /* 1: iterate returned Tcw (else the empty cv::Mat) */
    int32_t no_more;           /* bNoMore */
    int32_t n_inliers;         /* nInliers */
    int32_t hypothesis;        /* the iteration whose Refine returned, or the best's at exhaustion (0-based); -1: none */
    int32_t refined;           /* 1: Tcw is mRefinedTcw (a Refine returned), 0: mBestTcw (exhaustion) */
    int32_t iterations;        /* mnIterations after the call */
    int32_t best_inliers;      /* mnBestInliers after the call */
    int32_t best_hypothesis;   /* the iteration that holds the best, -1: none yet */
    float Tcw[16];             /* the returned matrix (returned == 1), row-major 4x4 CV_32F */
    float best_Tcw[16];        /* mBestTcw */
} OrbpResult;
typedef struct orbp_solver orbp_t;
int orbp_create(orbm_t* h, int n_all, const int32_t* idx, int n, const float* P2D, const float* sigma2, const float* P3Dw,
                const float K[4], orbp_t** out);
int orbp_create_frame(orbm_t* h, orbm_frame_t* f, const int32_t* idx, int n, const float* P3Dw, const float* level_sigma2, int n_levels,
                      const float K[4], orbp_t** out);
int orbp_set_ransac(orbp_t* s, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2);
int orbp_max_iterations(orbp_t* s, int* iterations);
int orbp_min_inliers(orbp_t* s, int* min_inliers);
int orbp_size(orbp_t* s, int* n, int* n_all);
int orbp_run(orbp_t* const* solvers, int count, const int32_t* const* sets, const int32_t* n_sets);
int orbp_hypotheses(orbp_t* s, OrbpHypothesis* out, int cap, int* n_out);
int orbp_iterate(orbp_t* s, int n_iterations, OrbpResult* res, uint8_t* inliers);
/* the last orbp_run this solver took part in: ms[0] the whole chain on the host's clock (upload to table down), then
 * its legs on the device's (events on the stream): ms[1] fit, ms[2] score + records, ms[3] Refine (tools/pnp_bench.py) */
int orbp_last_run_ms(orbp_t* s, double ms[4]);
void orbp_destroy(orbp_t* s);

/* ---------------------------------------------------------------- CreateNewMapPoints
 * replaces LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452, the same in both scenarios), the only caller of
 * SearchForTriangulation: one call searches the current keyframe against ALL its covisible neighbours, triangulates
 * every pair (the reference's 4x4 cv::SVD), applies its five gates and returns the new points in the reference's order
 * (neighbours ascending, idx1 ascending inside a neighbour).  Results equal the reference's loop bit for bit (its
 * OpenCV arithmetic is restated, unpinned: §2).
 *
 * MONOCULAR ONLY: mbMonocular == true, bStereo1 == bStereo2 == false, bOnlyStereo == false.  The stereo branches
 * (:311-316, :340-347, :377-387, :403-413) call binary64 atan2 / cos and are not built; the entries take no uright.
 *
 * The serial dependency.  In the reference a success with neighbour i calls mpCurrentKeyFrame->AddMapPoint(pMP, idx1),
 * and SearchForTriangulation with neighbour i + 1 skips idx1.  The batch computes every (neighbour, feature) in parallel
 * and then keeps, per feature, the first neighbour in order that was not skipped by the baseline gate and passed every
 * gate; the same feature reads "feature skipped" in every later neighbour.  That equals the serial loop because without
 * the orientation histogram (the reference builds ORBmatcher(0.6, false)) and with vbMatched2 never set, a query
 * feature's result against a neighbour depends on no other query -- and because every neighbour is a DIFFERENT
 * keyframe, so its AddMapPoint touches no later search.  Hence:
 *   - check_ori != 0 is refused (ORBX_E_UNSUPPORTED): the histogram prunes a bin by counting ALL matches of a neighbour,
 *     which would couple the queries and, through skip1, the neighbours;
 *   - a frame handle given twice, or a neighbour that is the current keyframe, is refused (ORBX_E_INVALID).
 *
 * OrblKeyFrame: the pose and the camera centre as the reference's getters return them (GetRotation, GetTranslation,
 *   GetCameraCenter: Ow is taken from the caller, not recomputed), K = (fx, fy, cx, cy); invfx = 1.0f/fx and invfy =
 *   1.0f/fy are formed in the library as Frame.cc does.  median_depth: KeyFrame::ComputeSceneMedianDepth(2) of a
 *   neighbour (it reads MapPoint positions from the object graph: the caller's); unused for the current keyframe.
 * OrblNewPoint: pos is the x3D passed to `new MapPoint`; normal, min_distance, max_distance restate what
 *   MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371) computes for a point with exactly these two observations and
 *   mpRefKF the current keyframe: normal = (n1 * (float)(1/|n1|) + n2 * (float)(1/|n2|)) * 0.5, each `normal +
 *   normali/norm` taken as cv::scaleAdd on CV_32F (float scale, float product, float sum; OpenCV's arithmetic is restated
 *   and unpinned, §2: equal to the restatement bit for bit, not verified against an OpenCV build), so that the sum of two
 *   floats does not depend on the std::map's pointer order; max_distance = dist1 *
 *   mvScaleFactors[octave1], min_distance = max_distance / mvScaleFactors[nlevels - 1].  ComputeDistinctiveDescriptors
 *   of a two-observation point picks by pointer order in the reference and is not produced here.
 * status (optional, n_neighbours x n1 bytes): one ORBL_ST_* code per (neighbour, feature): which gate ended the pair.
 * f12_used (optional, n_neighbours x 11 floats): F12 (9) and the epipole (2) the search of each processed neighbour used
 *   (zeros for a neighbour under the baseline gate): what orbl_compute_f12 returns.
 *
 * orbl_compute_f12: ComputeF12 (:536-553) and SearchForTriangulation's epipole (ORBmatcher.cc:666-672) in cv::Mat
 *   arithmetic, on the host; needs no GPU.  The batched entries call it themselves.
 * orbl_create_new_map_points: host arrays.  keys: mvKeysUn; fv: mFeatVec as CSR (node ids ascending, every feature in
 *   at most one node); skip: 1 where GetMapPoint(idx) is non-null (may be null: none), skip2 itself may be null;
 *   scale_factors / level_sigma2: mvScaleFactors / mvLevelSigma2 (nlevels entries, octaves are taken modulo 16);
 *   scale_factor: mfScaleFactor (ratioFactor = 1.5f * scale_factor).
 * orbl_create_new_map_points_frames: the same on device-resident frames that ran orbm_frame_compute_bow: only the skip
 *   flags and the keyframe records go up.
 * Limits and refusals: ORBX_E_UNSUPPORTED for check_ori != 0 and more than ORBL_MAX_NEIGHBOURS neighbours (the
 *   reference asks for 20); ORBX_E_INVALID for more than 65535 features in a keyframe (both entries), a malformed feature vector,
 *   repeated frames, frames without BoW; ORBX_E_CAPACITY when capacity is too small, with *n_new the needed count and
 *   nothing written (n1 always suffices: a feature yields at most one point).  Zero neighbours, zero features or no
 *   shared vocabulary node: ORBX_OK with *n_new = 0.  Without a HIP device no matcher handle exists: no CPU fallback. */
#define ORBL_MAX_NEIGHBOURS 32
#define ORBL_ST_NEIGHBOUR_SKIPPED 0   /* baseline / median_depth < 0.01 (the float quotient compared in double, :256-260) */
#define ORBL_ST_FEATURE_SKIPPED 1     /* skip1, or taken by an earlier neighbour */
#define ORBL_ST_NO_MATCH 2            /* SearchForTriangulation found no partner */
#define ORBL_ST_PARALLAX 3            /* !(cosParallaxRays > 0 && cosParallaxRays < 0.9998) */
#define ORBL_ST_X3D_ZERO 4            /* x3D(3) == 0 */
#define ORBL_ST_Z1 5                  /* z1 <= 0 */
#define ORBL_ST_Z2 6                  /* z2 <= 0 */
#define ORBL_ST_REPROJ1 7             /* reprojection error in the current keyframe above 5.991 sigma2 */
#define ORBL_ST_REPROJ2 8             /* reprojection error in the neighbour */
#define ORBL_ST_DIST_ZERO 9           /* dist1 == 0 || dist2 == 0 */
#define ORBL_ST_SCALE 10              /* the scale-ratio gate */
#define ORBL_ST_ACCEPTED 11           /* a new point */
typedef struct {
    float Rcw[9], tcw[3], Ow[3], K[4];
    float median_depth;
} OrblKeyFrame;
typedef struct {
    int32_t neighbour, idx1, idx2;
    float pos[3];
    float normal[3];
    float min_distance, max_distance;
} OrblNewPoint;
int orbl_compute_f12(const OrblKeyFrame* kf1, const OrblKeyFrame* kf2, float F12[9], float epipole[2]);
int orbl_create_new_map_points(orbm_t* h, const OrbxKeyPoint* keys1, const uint8_t* desc1, int n1, const OrbmFeatVec* fv1,
                               const uint8_t* skip1, const OrblKeyFrame* kf1, const OrbxKeyPoint* const* keys2,
                               const uint8_t* const* desc2, const int32_t* n2, const OrbmFeatVec* fv2, const uint8_t* const* skip2,
                               const OrblKeyFrame* kf2, int n_neighbours, const float* scale_factors, const float* level_sigma2,
                               int nlevels, float scale_factor, int check_ori, OrblNewPoint* out, int capacity, int* n_new,
                               uint8_t* status, float* f12_used);
int orbl_create_new_map_points_frames(orbm_t* h, orbm_frame_t* f1, const uint8_t* skip1, const OrblKeyFrame* kf1,
                                      orbm_frame_t* const* f2, const uint8_t* const* skip2, const OrblKeyFrame* kf2, int n_neighbours,
                                      const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor,
                                      int check_ori, OrblNewPoint* out, int capacity, int* n_new, uint8_t* status, float* f12_used);

#ifdef __cplusplus
}
#endif

/* LocalMapping::SearchInNeighbors: the batched Fuse (orbl_level_breaks, orbl_fuse_batch, orbl_fuse_batch_frames) is the same
 * library's and is declared in orbslamm_fuse.h, which rides along with this header. */
#include "orbslamm_fuse.h"

/* LoopClosing::SearchAndFuse and MultiMapper::SearchAndFuse: the dense Sim3 Fuse over all corrected keyframes is the same
 * library's and is declared in orbslamm_loopfuse.h. */
#include "orbslamm_loopfuse.h"

/* Optimizer::PoseOptimization: the batched motion-only Levenberg (orbo_pose_optimize, orbo_pose_optimize_frames) is the same
 * library's and is declared in orbslamm_poseopt.h. */
#include "orbslamm_poseopt.h"

/* Optimizer::OptimizeSim3: the batched 7-dof Levenberg for loop and merge candidates (orbz_optimize_sim3) is the same
 * library's and is declared in orbslamm_sim3opt.h. */
#include "orbslamm_sim3opt.h"

/* Tracking::SearchLocalPoints and TrackWithMotionModel's projections from a map-point pool in HBM (orbw_pool_*,
 * orbw_view_project, orbw_track_local_map, orbw_track_frame_pose) are the same library's and are declared in orbslamm_mappool.h. */
#include "orbslamm_mappool.h"
/* Tracking::UpdateLocalMap from a keyframe store beside that pool (orbu_*, orbw_track_local_map_resident): orbslamm_localmap.h. */
#include "orbslamm_localmap.h"
/* KeyFrame::UpdateConnections and KeyFrameCulling's counts over that store (orbn_*, orbu_kf_set_octaves): orbslamm_covis.h. */
#include "orbslamm_covis.h"
/* PoseOptimization behind those searches, fed from the pool, the frame set and the search's own table (orbq_track_pose):
 * orbslamm_trackpose.h. */
#include "orbslamm_trackpose.h"
/* Tracking::Relocalization behind PnPsolver::iterate, per candidate: three PoseOptimizations and two keyframe projections from the
 * pool, the store and the frame set (orbq_relocalize): orbslamm_reloc.h. */
#include "orbslamm_reloc.h"
/* Tracking::TrackWithMotionModel from the predicted pose to the counts its verdicts read: the pose product, the frame/frame
 * search and its retry, PoseOptimization and the discard loop from the pool and the frame set (orbq_track_motion_model):
 * orbslamm_motion.h. */
#include "orbslamm_motion.h"
/* LoopClosing::ComputeSim3 behind the Sim3Solver, per candidate: SearchBySim3 and OptimizeSim3 from the pool, the store and the
 * frame set (orby_compute_sim3): orbslamm_computesim3.h. */
#include "orbslamm_computesim3.h"
/* MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth over that store, refreshing the pool's records in place
 * (orbr_refresh_points, orbu_kf_set_descriptors / _centres, orbw_debug_pool_get): orbslamm_refresh.h. */
#include "orbslamm_refresh.h"
/* LoopClosing::CorrectLoop's correction and MultiMapper::UpdatePosesAndAdd's over that store: the Sim3 propagated, the points
 * moved once, their normals and depths, the new poses and centres (orbe_correct_sim3, orbu_point_set_ref_kf): orbslamm_correct.h. */
#include "orbslamm_correct.h"
/* Tracking::CreateInitialMapMonocular from its bundle adjustment on: the two-keyframe Schur Levenberg, the median depth, the
 * verdict and the rescaling (orbb_initial_map, orbb_initial_map_frames): orbslamm_initmap.h. */
#include "orbslamm_initmap.h"
#endif
