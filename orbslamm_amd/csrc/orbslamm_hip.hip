// orbslamm_hip.hip -- C ABI of the MI355X ORB front-end (see include/orbslamm_hip.h).
//
// Host side of the extractor: per-instance tables exactly as the reference
// constructor builds them (/root/reference/SingleRobotScenario/src/ORBextractor.cc:410-470),
// level / cell / quadtree-root geometry (:765-806, :543-563), cv::resize coefficient
// tables, one-time device allocation, kernel launches on the handle's stream.
// No CPU compute path exists: without a HIP device every compute entry fails.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#if defined(__x86_64__)
#include <immintrin.h>  // streaming stores of the pageable-frame staging (orbx_handle.inc: stage_rows)
#endif

#include "../../include/orbslamm_hip.h"
#include "orbx_common.hpp"
#include "orbx_cvmath.hpp"   // OpenCV 3.0 float arithmetic shared by the solver families (orbi, orbs, orbp, orbl, orbf)

#include "orbx_kernels.hip"
#include "orbm_kernels.hip"
#include "orbt_kernels.hip"
#include "orbv_kernels.hip"
#include "orbk_kernels.hip"
#include "orbi_kernels.hip"
#include "orbs_kernels.hip"
#include "orbp_kernels.hip"
#include "orbf_kernels.hip"   // the Fuse pieces shared by orbl's k_fuse_batch and orbc's k_loopfuse_search
#include "orbl_kernels.hip"
#include "orbc_kernels.hip"
#include "orbg_kernels.hip"   // the g2o / Eigen pieces shared by orbo's k_pose_optimize and orbz's k_sim3_optimize
#include "orbo_kernels.hip"
#include "orbz_kernels.hip"
#include "orbw_kernels.hip"   // the map-point pool and the projections of the two tracking searches
#include "orbu_kernels.hip"   // UpdateLocalMap: the keyframe vote, the local keyframe list, the local point list
#include "orbn_kernels.hip"   // covisibility: UpdateConnections' counter and ordered list, KeyFrameCulling's counts, over the store
#include "orbq_kernels.hip"   // PoseOptimization from the pool: merge, ordered edge list, orbo's solve, Tracking's loop behind it
#include "orbq_reloc_kernels.hip"   // Relocalization behind the PnP pose: the stage kernel on orbq's pieces, the keyframe projection, sFound
#include "orbq_motion_kernels.hip"  // TrackWithMotionModel: the pose product, the retry decision and the solve as a stage kernel, the frame/frame projection from the device-made pose
#include "orbr_kernels.hip"   // the map-point refresh: ComputeDistinctiveDescriptors and UpdateNormalAndDepth over the store, into the pool
#include "orbe_kernels.hip"   // the loop correction: the Sim3 propagated, the points moved once, orbr's normals with mixed centres, the commit
#include "orbg_schur.hip"    // the g2o pieces of a bundle adjustment with marginalised points: the two-vertex edge, the Schur share, the reduced LDLt, Levenberg over the full system
#include "orbb_kernels.hip"   // the initial map: the two-keyframe bundle adjustment on orbg_schur's pieces, the median depth, the verdict, the rescaling
#include "orby_kernels.hip"   // ComputeSim3 behind the solver: SearchBySim3's two passes, the agreement, OptimizeSim3's walk, orbz's solve

using namespace orbx;

static_assert(sizeof(OrbxKeyPoint) == 28, "cv::KeyPoint layout");
static_assert(sizeof(OrbxKeyPointDev) == 28, "cv::KeyPoint layout");

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(ORBX_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

extern "C" const char* orbx_last_error(void) { return g_err.c_str(); }

#include "orbx_hostutil.inc"   // HIPCHK_OR, the grow-only device and pinned blocks, Packer

// live handles: objects that point at another handle (a frame set at its matcher and at the extractor it last read
// from) check here before touching it in their destructor -- handles may be destroyed in any order
static std::mutex g_liveMu;
static std::vector<const void*> g_live;
static void live_add(const void* h) { std::lock_guard<std::mutex> l(g_liveMu); g_live.push_back(h); }
static void live_remove(const void* h)
{
    std::lock_guard<std::mutex> l(g_liveMu);
    for (size_t i = 0; i < g_live.size(); i++) if (g_live[i] == h) { g_live[i] = g_live.back(); g_live.pop_back(); return; }
}
static bool live_has(const void* h)
{
    std::lock_guard<std::mutex> l(g_liveMu);
    for (const void* p : g_live) if (p == h) return true;
    return false;
}

extern "C" int orbx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// PCI bus id ("0000:c1:00.0") of a device: lets a launcher pin a rank to the GPU's NUMA node (bench.py)
extern "C" int orbx_device_pci_bus_id(int device, char* out, int cap)
{
    if (!out || cap < 16) return fail(ORBX_E_INVALID, "bad argument");
    HIPCHK(hipDeviceGetPCIBusId(out, cap, device));
    return ORBX_OK;
}

// The shader clock the device runs at NOW, UNDER LOAD: a ~0.1 ms kernel that fills every SIMD with FMA chains
// (tools/ubench/clock_ramp.hip's measurement as a library call) reads s_memtime (the shader clock's counter) against
// s_memrealtime (a constant 100 MHz counter) in its first wave.  (A one-wave probe reads the governor's light-load boost,
// 2.43 GHz whatever came before.)  After an idle gap an MI355X starts a loaded kernel at ~2.0 GHz and needs ~40 ms of load to
// reach its ~2.37 GHz; a rank of a multi-GPU job that reports its clock right behind its timed region tells a cold or
// throttled GPU from a slow pipeline (bench.py, per rank).
__global__ __launch_bounds__(256) void k_clock_probe(uint64_t* out, float* sink, int iters)
{
    uint64_t c0 = 0, r0 = 0;
    const bool stamp = blockIdx.x == 0 && threadIdx.x == 0;
    if (stamp) { c0 = __builtin_readcyclecounter(); r0 = __builtin_amdgcn_s_memrealtime(); }
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = (float)threadIdx.x * 0.5f + (float)i;
    for (int it = 0; it < iters; it++)
#pragma unroll
        for (int i = 0; i < 8; i++) a[i] = __builtin_fmaf(a[i], 1.0001f, 0.5f);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) s += a[i];
    if (s == 12345.f) sink[0] = s;   // (keeps the chains alive)
    if (stamp) { out[0] = __builtin_readcyclecounter() - c0; out[1] = __builtin_amdgcn_s_memrealtime() - r0; }
}
extern "C" int orbx_device_shader_clock_mhz(int device, float* mhz)
{
    if (!mhz) return fail(ORBX_E_INVALID, "bad argument");
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(device));
    uint64_t* d = nullptr;
    uint64_t h[2] = {0, 0};
    hipError_t e = hipMalloc(&d, sizeof h + 8);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_clock_probe, dim3(2048), dim3(256), 0, nullptr, d, (float*)(d + 2), 1000);
        e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
        (void)hipFree(d);
    }
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(ORBX_E_HIP, "clock probe failed: %s", hipGetErrorString(e));
    *mhz = h[1] ? (float)((double)h[0] / (double)h[1] * 100.0) : 0.f;
    return ORBX_OK;
}

// spin-wait hint of the latency path's poll
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    std::this_thread::yield();
#endif
}

// Waits for a flag a kernel raises in coherent pinned memory behind a call's results: a tight poll first (the common case:
// microseconds), then a yielding poll for up to five seconds.  Only after that does the caller fall back to synchronising
// the stream -- which, for the chain streams several handles share, would also wait for the OTHER handles' work queued
// behind this call's: a late chain (a profiler, an oversubscribed host) must not turn into cross-robot coupling.
static inline bool wait_flag(volatile int32_t* flag, int32_t want)
{
    for (int spin = 0; spin < 400000; spin++) { if (*flag == want) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; } cpu_relax(); }
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::steady_clock::now() - t0 < std::chrono::seconds(5)) {
        for (int spin = 0; spin < 256; spin++) { if (*flag == want) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return true; } cpu_relax(); }
        std::this_thread::yield();
    }
    return false;
}

static inline int cv_round(double v) { return (int)lrint(v); }  // cvRound: half to even
static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

// The library is ONE translation unit (every kernel is a template or inline function of a header-like .hip file); its host
// side is split by family (orbx_hostutil.inc above: what they share):
// the extractor, in seven parts by concern; each depends on the ones above it only (two forward declarations in orbx_handle.inc)
#include "orbx_handle.inc"       // environment switches, profiler, staging helpers, the handle and its result-set accessors
#include "orbx_geometry.inc"     // constructor tables, level / cell / resize geometry, LDS footprints, table queries
#include "orbx_streams.inc"      // the two stream pools, create / destroy (what a handle owns), draining and joining
#include "orbx_pipeline.inc"     // configure_shape, Launcher, run_extract (the event graph), device-resident entries
#include "orbx_hostpath.inc"     // copy streams, slots, pinned memory, submit_core, collect / release, blocking entries
#include "orbx_streammatch.inc"  // the stream matcher's launches, the roll of the previous frame, match downloads
#include "orbx_probe.inc"        // stereo, pyramid / candidate read-back, reset, serial, profile entries, orbx_debug_*
#include "orbm_host.inc"   // matchers (includes orbt_host.inc: the Tracking-shaped searches and frame sets)
#include "orbv_host.inc"   // vocabulary

#include "orbt_bow_host.inc"
#include "orbk_host.inc"   // keyframe database
#include "orbi_host.inc"   // Initializer
#include "orbs_host.inc"   // Sim3Solver
#include "orbp_host.inc"   // PnPsolver
#include "orbf_host.inc"   // the Fuse staging shared by orbl_fuse_batch* and orbc_search_and_fuse*
#include "orbl_host.inc"   // CreateNewMapPoints, SearchInNeighbors' batched Fuse
#include "orbc_host.inc"   // SearchAndFuse
#include "orbo_host.inc"   // PoseOptimization
#include "orbz_host.inc"   // OptimizeSim3
#include "orbx_poolutil.inc"   // the pool and the store as the host holds them; what orbw, orbu, orbn and orbq share on the host
#include "orbw_host.inc"   // the map-point pool: SearchLocalPoints and TrackWithMotionModel's search from resident MapPoints
#include "orbu_host.inc"   // the keyframe store beside the pool and every setter of it: UpdateLocalMap, and SearchLocalPoints from its resident list
#include "orbn_host.inc"   // the covisibility entries over the store: batched UpdateConnections and KeyFrameCulling counts
#include "orbr_host.inc"   // the refresh entry and its blocks, orbw_debug_pool_get
#include "orbe_host.inc"   // the loop correction's entry and its blocks
#include "orbq_scaffold.inc"   // what the four orbq entries below share on the host: the checks, the solver block, the arena replay, the drained tail
#include "orbq_host.inc"   // PoseOptimization behind the pool searches: TrackWithMotionModel's and TrackLocalMap's verdicts
#include "orbq_reloc_host.inc"   // Relocalization behind PnPsolver::iterate: three solves and two keyframe projections per candidate
#include "orbq_motion_host.inc"  // TrackWithMotionModel from the predicted pose to the counts: both searches, the gate, the solve and the loop in one call
#include "orbb_host.inc"   // CreateInitialMapMonocular from its bundle adjustment on: two poses and their shared points per problem
#include "orby_host.inc"   // SearchBySim3 and OptimizeSim3 from the pool, the store and the frame set: ComputeSim3's verdict per candidate
