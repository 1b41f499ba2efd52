// orbq_kernels.hip -- PoseOptimization fed from the map-point pool (part of orbslamm_hip.hip; host side: orbq_host.inc, ABI:
// include/orbslamm_trackpose.h): the line behind the search in Tracking::TrackWithMotionModel and
// Tracking::TrackLocalMap, for a batch of frames in ONE launch, one wave a frame (orbo_kernels.hip's layout).
//   prologue   merged[t] = the search's match (ids[assign[t]], ORBmatcher.cc:123 / :1430: a match overwrites) or the frame's id
//              before the search; per 64 features, an ORDERED compaction of the features that hold a point into the edge list
//              (ballot + prefix, the chunks in ascending order: edge e is the e-th such feature, as vpEdgesMono is built,
//              Optimizer.cc:302-341); Xw from the pool record, the observation from the resident mvKeysUn
//   solve      orbo::solve_frame, the body of k_pose_optimize
//   epilogue   per feature: mvbOutlier, the frame's ids after the discard loop, the two counts
// The prologue (merge_and_gather) and the epilogue (loop_behind_solve, or leave_unsolved where a gate said no) are device functions over an id SOURCE: k_track_pose's is a
// pool search's table, k_track_reference's (Tracking::TrackReferenceKeyFrame) SearchByBoW's table over the keyframe
// store's entries row.
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

// Where a kernel's merged ids come from, in the two stages of the prologue's walk: first(t) is the search's table entry for feature t
// (the reads of all the chunks of a step are issued together), id(t, q, bad) the pool id behind it, or -1.
// k_track_pose: a pool search's table over its query ids, or the frame's ids before the search.
struct SearchSource {
    const int32_t* assign; const int32_t* ids; const int32_t* base; int32_t nq;
    __device__ __forceinline__ int first(int t, int n) const { return t < n && assign ? assign[t] : -1; }
    __device__ __forceinline__ int id(int t, int n, int q, bool& bad) const
    {
        int v = -1;
        if (q >= 0) {
            // (a match names a query of the search, and a query that matched held a point)
            if (q < nq) v = ids[q];
            bad |= v < 0;
        } else if (t < n && base) v = base[t];
        return v;
    }
};
// k_track_reference: SearchByBoW's table over the keyframe's features, and the keyframe's match list in the store behind it
// (ORBmatcher.cc:236 vpMapPointMatches[bestIdxF] = pMP; Tracking.cc:817 replaces mvpMapPoints whole: there are no base ids)
struct KeyFrameSource {
    const int32_t* table; const int32_t* entries; int32_t nTable, stride;
    __device__ __forceinline__ int first(int t, int n) const { return t < n && t < nTable ? table[t] : -1; }
    __device__ __forceinline__ int id(int, int, int q, bool& bad) const
    {
        int v = -1;
        if (q >= 0) {
            // (a match names a keyframe feature that passed the validity rule: below the stride, with a point)
            if (q < stride) v = entries[q];
            bad |= v < 0;
            if (v >= 0) v &= ~orbu::kNoVote;
        }
        return v;
    }
};

// merged[t] from `src`, and per 64 features the ordered compaction of the features that hold a point into the edge list from f0 on
// (Optimizer.cc:302-341); returns the edge count.  edges = false (k_track_reference's gate, wave-uniform): the merge alone.
template <class Source>
__device__ __forceinline__ int merge_and_gather(const Args& a, const Source& src, const orbm::KeyDev* keys, int n, int f0, int nDev, int lane,
                                                bool edges, bool& bad)
{
    // kBatch chunks of 64 features a step: each stage's reads of all the chunks are issued before any is used, so that one wave's
    // walk over a frame's features pays a memory latency (for the table and a host-listed search's ids, a trip over the link) per
    // stage and step, not per chunk.  The chunks are consumed in ascending order: the edge list ascends by feature.
    int nEdges = 0;
    for (int c = 0; c < n; c += kBatch * kLanes) {
        int q[kBatch], id[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            q[k] = src.first(t, n);
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            id[k] = src.id(t, n, q[k], bad);
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
            if (edges && id[k] >= 0) { A[k] = a.pool.a[id[k]]; u[k] = keys[t].x; v[k] = keys[t].y; oct[k] = keys[t].octave; }
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const int t = c + k * kLanes + lane;
            if (t < n) a.merged[f0 + t] = id[k];
            const bool has = edges && id[k] >= 0;
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
    return nEdges;
}

// Tracking.cc:950-969 (discard; TrackReferenceKeyFrame's :824-841 is the same loop) and :993-1013 (monocular: outliers keep their
// point): per feature mvbOutlier and the frame's id after the loop, and the two counts into `out`
__device__ __forceinline__ void loop_behind_solve(const Args& a, int n, int f0, int discard, int lane, OrbqResult* out)
{
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
            const bool has = id[k] >= 0, outl = has && o[k] != 0;
            if (t < n) {
                a.outlierOut[f0 + t] = outl ? 1 : 0;
                a.idsOut[f0 + t] = outl && discard ? -1 : id[k];
            }
            const bool in = has && !outl;
            const bool inMap = in && (fl[k] & 2u) != 0;   // ORBW_FLAG_OBSERVED: Observations() > 0
            nMatch += __popcll(__ballot(in));
            nMap += __popcll(__ballot(inMap));
        }
    }
    if (lane == 0) { out->n_matches = nMatch; out->n_matches_map = nMap; }
}

// The gate said no (k_track_reference, k_motion_stage: wave-uniform): the reference returns before it touches the frame.  The pose as
// it came, no round (-1: the merge met something the host refuses), the table's ids as they merged, no outlier
__device__ __forceinline__ void leave_unsolved(const Args& a, int n, int f0, int lane, bool anyBad, const float* Tcw, int nMatches, OrbqResult* out)
{
    if (lane == 0) {
        for (int i = 0; i < 16; i++) out->opt.Tcw[i] = Tcw[i];
        out->opt.rounds = anyBad ? -1 : 0;
        out->n_matches = nMatches; out->n_matches_map = 0;
    }
    if (anyBad) return;
    for (int t = lane; t < n; t += kLanes) { a.idsOut[f0 + t] = a.merged[f0 + t]; a.outlierOut[f0 + t] = 0; }
}

// The overflow protocol of the chains that search through a candidate arena (k_reloc_stage, k_motion_stage): a search's count nm below
// 0 says its share was too small and holds -(entries needed) - 1.  One lane of the job writes the need and stops the job in `overflow`;
// the host grows the arena to the largest need and runs the whole call again
__device__ __forceinline__ void report_overflow(int nm, int32_t* need, int32_t* state, int32_t overflow) { *need = -nm - 1; *state = overflow; }

__global__ __launch_bounds__(kLanes) void k_track_pose(Args a, int nJobs)
{
    __shared__ orbg::LmShared<6> sLm;
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= nJobs) return;
    const JobDev& J = a.jobs[j];
    const int n = J.n, f0 = J.f0, nDev = *J.nKeys;
    bool bad = false;
    const SearchSource src = {J.assign, J.ids, J.base, J.nq};
    const int nEdges = merge_and_gather(a, src, J.keys, n, f0, nDev, lane, true, bad);
    const bool anyBad = __any(bad);
    __syncthreads();
    orbo::solve_frame(a.o, J.Tcw, J.K, f0, nEdges, anyBad, &a.out[j].opt, sLm, lane);
    __syncthreads();
    if (anyBad) return;
    loop_behind_solve(a, n, f0, J.discard, lane, &a.out[j]);
}

// ------------------------------------------------------------------ Tracking::TrackReferenceKeyFrame (Tracking.cc:802-844)
// One job: SearchByBoW(pKF = slot kfSlot, F = slot `slot`) with the validity of ORBmatcher.cc:191-197 taken from the keyframe
// store's entries row and the pool's flag word; the merge through the match table; the gate of :814 / :1436; §8s's solve and loop.
struct RefJobDev {
    float Tcw[16];
    float K[4];
    const orbm::KeyDev* keys;   // the current slot's mvKeysUn
    const int32_t* nKeys;       // ... and its device count
    const int32_t* entries;     // the keyframe's row of the store: entries[q] = pool id of its feature q, bit 30 aside, or -1
    uint8_t* valid;             // [cap] of the job's pair: k_ref_valid writes it, k_bow_set reads it
    const int32_t* table;       // [cap] the pruned table of the job's pair (k_bow_prune_set), -1 behind the frame's device count
    const int32_t* nBow;        // ... and its count over the whole slot (the kernel counts over the job's n itself)
    int32_t n, f0, solve, cap;
    int32_t matchAt, pad;       // where the job's table goes in the call's match block, or -1: not asked for
};
struct RefArgs {
    Args q;                     // q.jobs and q.out unused
    const RefJobDev* jobs;
    OrbqRefResult* out;
    int32_t* matchOut;
    int32_t stride, minMatches;
};

// ORBmatcher.cc:191-197: MapPoint* pMP = vpMapPointsKF[realIdxKF]; if(!pMP) continue; if(pMP->isBad()) continue;
// One thread a keyframe feature, consecutive threads consecutive features of the row.  A feature at or above the store's stride
// holds no point; bit 30 (a point in the match slot that does not vote) is not part of the id.
__global__ __launch_bounds__(256) void k_ref_valid(const RefJobDev* __restrict__ jobs, orbw::PoolDev pool, int stride)
{
    const RefJobDev& J = jobs[blockIdx.y];
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= J.cap) return;
    uint8_t ok = 0;
    if (q < stride) {
        const int e = J.entries[q];
        if (e >= 0) {
            const int id = e & ~orbu::kNoVote;
            ok = id < pool.cap && (pool.flags[id] & 1u) == 0;   // ORBW_FLAG_BAD: isBad()
        }
    }
    J.valid[q] = ok;
}

__global__ __launch_bounds__(kLanes) void k_track_reference(RefArgs r, int nJobs)
{
    __shared__ orbg::LmShared<6> sLm;
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= nJobs) return;
    const RefJobDev& J = r.jobs[j];
    const Args& a = r.q;
    const int n = J.n, f0 = J.f0, nDev = *J.nKeys, nTable = min(nDev, J.cap);
    OrbqRefResult* out = r.out + j;
    // n_bow: the matches among the job's n features (the prune kernel's count covers the whole slot: the same number when n is the
    // slot's count, as Tracking passes it); the table goes down on the same walk where it was asked for
    int nBow = 0;
    for (int c = 0; c < n; c += kLanes) {
        const int t = c + lane;
        const int m = t < n && t < nTable ? J.table[t] : -1;
        if (t < n && J.matchAt >= 0) r.matchOut[J.matchAt + t] = m;
        nBow += __popcll(__ballot(m >= 0));
    }
    // Tracking.cc:814 if(nmatches<15) return false; :1436 (Relocalization's first loop stops behind the search): wave-uniform
    const bool gate = nBow < r.minMatches, solve = !gate && J.solve != 0;
    bool bad = false;
    const KeyFrameSource src = {J.table, J.entries, nTable, r.stride};
    const int nEdges = merge_and_gather(a, src, J.keys, n, f0, nDev, lane, solve, bad);
    const bool anyBad = __any(bad);
    if (lane == 0) { out->n_bow = nBow; out->status = gate ? ORBQ_REF_TOO_FEW : J.solve ? ORBQ_REF_TRACKED : ORBQ_REF_SEARCH_ONLY; }
    __syncthreads();
    if (!solve) { leave_unsolved(a, n, f0, lane, anyBad, J.Tcw, nBow, &out->track); return; }
    orbo::solve_frame(a.o, J.Tcw, J.K, f0, nEdges, anyBad, &out->track.opt, sLm, lane);
    __syncthreads();
    if (anyBad) return;
    loop_behind_solve(a, n, f0, 1, lane, &out->track);
}

}  // namespace orbq
