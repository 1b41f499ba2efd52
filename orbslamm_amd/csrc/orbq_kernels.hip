// orbq_kernels.hip -- PoseOptimization fed from the map-point pool (part of orbslamm_hip.hip; host side: orbq_host.inc, ABI:
// include/orbslamm_trackpose.h): the line behind the search in Tracking::TrackWithMotionModel and
// Tracking::TrackLocalMap, for a batch of frames in ONE launch, one wave a frame (orbo_kernels.hip's layout).
//   prologue   merged[t] = the search's match (ids[assign[t]], ORBmatcher.cc:123 / :1430: a match overwrites) or the frame's id
//              before the search; per 64 features, an ORDERED compaction of the features that hold a point into the edge list
//              (ballot + prefix, the chunks in ascending order: edge e is the e-th such feature, as vpEdgesMono is built,
//              Optimizer.cc:302-341); Xw from the pool record, the observation from the resident mvKeysUn
//   solve      orbo::solve_frame, the body of k_pose_optimize
//   epilogue   per feature: mvbOutlier, the frame's ids after the discard loop, the two counts
// The prologue writes edge e from the lane of its FEATURE (t % 64); the solve reads it from lane e % 64, and the epilogue reads an
// edge's outlier byte from its feature's lane again: a workgroup barrier (one wave: its fence is what counts) stands between the
// three.  No atomics; every loop is bounded by the job's n.
#pragma once

namespace orbq {

constexpr int kLanes = orbo::kLanes;
constexpr int kBatch = 8;   // chunks of 64 features whose reads are in flight together (prologue and epilogue)

struct JobDev {
    float Tcw[16];
    float K[4];
    const orbm::KeyDev* keys;   // the slot's mvKeysUn
    const int32_t* nKeys;       // the slot's device count
    const int32_t* assign;      // the search's table (the set's pinned result block), or null: no search is merged
    const int32_t* ids;         // the search's query ids where it left them: its pinned staging, or a keyframe store's S
    const int32_t* base;        // the frame's ids before the search (device), or null: all -1
    int32_t nq, n, f0, discard; // f0: where the job's features (and its edges) start in the call's arrays
};
struct Args {
    orbo::Args o;               // pw, uv, outlier (per edge, at f0 + e), the sigma table
    const JobDev* jobs;
    orbw::PoolDev pool;
    int32_t* merged;            // per feature: written and read by the feature's lane
    int32_t* idsOut;
    uint8_t* outlierOut;
    OrbqResult* out;
};

__device__ __forceinline__ int below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(kLanes) void k_track_pose(Args a, int nJobs)
{
    __shared__ orbg::LmShared<6> sLm;
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= nJobs) return;
    const JobDev& J = a.jobs[j];
    const int n = J.n, f0 = J.f0, nDev = *J.nKeys;
    bool bad = false;
    // kBatch chunks of 64 features a step: each stage's reads of all the chunks are issued before any is used, so that one wave's
    // walk over a frame's features pays a memory latency (for the table and a host-listed search's ids, a trip over the link) per
    // stage and step, not per chunk.  The chunks are consumed in ascending order: the edge list ascends by feature.
    int nEdges = 0;
    for (int c = 0; c < n; c += kBatch * kLanes) {
        int q[kBatch], id[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            q[k] = t < n && J.assign ? J.assign[t] : -1;
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            id[k] = -1;
            if (q[k] >= 0) {
                // (a match names a query of the search, and a query that matched held a point)
                if (q[k] < J.nq) id[k] = J.ids[q[k]];
                bad |= id[k] < 0;
            } else if (t < n && J.base) id[k] = J.base[t];
            // a point outside the pool, or at a feature the resident frame does not hold: refused after the kernel
            if (id[k] >= a.pool.cap || (id[k] >= 0 && t >= nDev)) { bad = true; id[k] = -1; }
        }
        float4 A[kBatch];
        float u[kBatch], v[kBatch];
        int oct[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            A[k] = make_float4(0.f, 0.f, 0.f, 0.f); u[k] = 0.f; v[k] = 0.f; oct[k] = 0;
            if (id[k] >= 0) { A[k] = a.pool.a[id[k]]; u[k] = J.keys[t].x; v[k] = J.keys[t].y; oct[k] = J.keys[t].octave; }
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            if (t < n) a.merged[f0 + t] = id[k];
            const bool has = id[k] >= 0;
            const unsigned long long m = __ballot(has);
            if (has) {
                const int e = nEdges + below(m, lane);
                const bool okOct = oct[k] >= 0 && oct[k] < a.o.nlevels;
                bad |= !okOct;
                a.o.pw[f0 + e] = make_float4(A[k].x, A[k].y, A[k].z, okOct ? a.o.invSigma2[oct[k]] : 0.f);
                a.o.uv[f0 + e] = make_float2(u[k], v[k]);
                a.o.outlier[f0 + e] = 0;
            }
            nEdges += __popcll(m);
        }
    }
    const bool anyBad = __any(bad);
    __syncthreads();
    orbo::solve_frame(a.o, J.Tcw, J.K, f0, nEdges, anyBad, &a.out[j].opt, sLm, lane);
    __syncthreads();
    if (anyBad) return;
    // Tracking.cc:950-969 (discard) and :993-1013 (monocular: outliers keep their point)
    int e0 = 0, nMatch = 0, nMap = 0;
    for (int c = 0; c < n; c += kBatch * kLanes) {
        int id[kBatch], e[kBatch];
        unsigned long long m[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            id[k] = t < n ? a.merged[f0 + t] : -1;
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            m[k] = __ballot(id[k] >= 0);
            e[k] = e0 + below(m[k], lane);
            e0 += __popcll(m[k]);
        }
        uint8_t o[kBatch];
        uint32_t fl[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            o[k] = 0; fl[k] = 0;
            if (id[k] >= 0) { o[k] = a.o.outlier[f0 + e[k]]; fl[k] = a.pool.flags[id[k]]; }
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            const bool has = id[k] >= 0, out = has && o[k] != 0;
            if (t < n) {
                a.outlierOut[f0 + t] = out ? 1 : 0;
                a.idsOut[f0 + t] = out && J.discard ? -1 : id[k];
            }
            const bool in = has && !out;
            const bool inMap = in && (fl[k] & 2u) != 0;   // ORBW_FLAG_OBSERVED: Observations() > 0
            nMatch += __popcll(__ballot(in));
            nMap += __popcll(__ballot(inMap));
        }
    }
    if (lane == 0) { a.out[j].n_matches = nMatch; a.out[j].n_matches_map = nMap; }
}

}  // namespace orbq
