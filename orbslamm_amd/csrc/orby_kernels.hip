// orby_kernels.hip -- LoopClosing::ComputeSim3's chain behind the Sim3Solver, per candidate, closed on the device (part of
// orbslamm_hip.hip; host side: orby_host.inc, ABI: include/orbslamm_computesim3.h): ORBmatcher::SearchBySim3
// (ORBmatcher.cc:1104-1328, monocular) and Optimizer::OptimizeSim3 (Optimizer.cc:1348-1543) for a batch of (pKF1, pKF2, Sim3) jobs.
//   k_sim3_marks     vbAlreadyMatched2 from the entering matches (:1131-1144): one thread an entering match; several may write
//                    the same byte, all of them a 1
//   k_sim3_search    the two passes (:1150-1227, :1230-1307): one workgroup per (job, direction, tile of 64 features), one lane a
//                    feature: validity from the store's row and the pool's flag word, orbf::sim3_gates, orbf::window_best<1> over
//                    the resident slot's grid; vnMatch1 | vnMatch2 and the status bytes stay in HBM
//   k_compute_sim3   one wave a job, k_track_reference's layout: the agreement (:1309-1325), OptimizeSim3's walk (Optimizer.cc:
//                    1401-1440) with the ORDERED compaction of the correspondences (ballot + prefix, chunks of 64 features in
//                    ascending order), the gather into orbz's edge arrays, orbz::solve_problem (the body of k_sim3_optimize), the
//                    epilogue (:1497, :1532: the matches either check nulled)
// The walk writes the two edges of correspondence c from the lane of its FEATURE (i % 64); the solve reads edge e from lane e % 64,
// and the epilogue reads a correspondence's removed byte from its feature's lane again: a workgroup barrier (one wave: its fence is
// what counts) stands between the three.  No atomics; every loop is bounded by the job's n1 / n2.
#pragma once

namespace orby {

constexpr int kLanes = 64;
constexpr int kThHigh = 100;   // ORBmatcher::TH_HIGH
// the status codes of include/orbslamm_computesim3.h (ORBY_ST_*)
enum : uint8_t { ST_NO_POINT = 0, ST_MARKED, ST_BAD, ST_DEPTH, ST_OUTSIDE_IMAGE, ST_DISTANCE, ST_LEVEL_RANGE, ST_NO_CANDIDATE, ST_FOUND };

// one keyframe of a job: its slot of the frame set, its row of the store
struct SideDev {
    const orbm::KeyDev* keys; const uint8_t* desc; const int32_t* cellStart; const int32_t* cellIdx;
    const int32_t* nKeys;     // the slot's device count
    const int32_t* entries;   // entries[q] = pool id of its feature q, bit 30 aside, or -1
    float bounds[4];          // mnMinX, mnMaxX, mnMinY, mnMaxY
    int32_t n, pad;
};
struct JobDev {
    OrbzProblem p;
    double delta;             // (double)sqrtf(th2), taken on the host as orbz_host.inc takes it
    SideDev kf[2];            // pKF1, pKF2
    orbm::GridDev grid;       // the frame set's
    float sR[2][9], t[2][3];  // [0]: sR21, t21 (pass 1->2); [1]: sR12, t12 (pass 2->1)
    float th;
    int32_t f1, f2, f12;      // where the job's n1-arrays, its n2-array (already2) and its (n1 + n2)-arrays start in the call's
};
struct Args {
    orbz::Args z;             // pw, uv, off per edge at 2 f1 + e; removed per correspondence at f1 + c; the sigma tables; nlevels
    const JobDev* jobs;
    orbw::PoolDev pool;
    const int32_t* m12Id; const int32_t* m12Idx2;     // [sum n1] the entering matches
    uint8_t* already2;        // [sum n2]
    int32_t* vn;              // [sum n1 + n2] vnMatch1 | vnMatch2 per job
    uint8_t* status;          // [sum n1 + n2]
    int32_t* match; int32_t* id2; int32_t* corrOf;    // [sum n1]: written and read by the feature's lane
    int32_t* matchOut; int32_t* idsOut;               // [sum n1]
    OrbyResult* out;
    int32_t* bad;             // [n_jobs]: a finding the host refuses the call for
    float sf[2][16], breaks[2][17];                   // per keyframe: mvScaleFactors, orbl_level_breaks' table
    int32_t stride;           // the store's
};

__device__ __forceinline__ int below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(256) void k_sim3_marks(Args a)
{
    const JobDev& J = a.jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.kf[0].n) return;
    const int idx2 = a.m12Idx2[J.f1 + i];
    if (a.m12Id[J.f1 + i] >= 0 && idx2 >= 0 && idx2 < J.kf[1].n) a.already2[J.f2 + idx2] = 1;
}

__global__ __launch_bounds__(kLanes) void k_sim3_search(Args a)
{
    const JobDev& J = a.jobs[blockIdx.z];
    const int dir = blockIdx.y, i = blockIdx.x * kLanes + threadIdx.x;
    const SideDev& F = J.kf[dir];        // the points' keyframe
    const SideDev& T = J.kf[1 - dir];    // the keyframe searched
    if (i >= F.n) return;
    const int at = J.f12 + (dir ? J.kf[0].n : 0) + i;
    const int e = i < a.stride ? F.entries[i] : -1;
    const int id = e & ~orbu::kNoVote;
    uint8_t st = ST_NO_POINT;
    int found = -1;
    if (e >= 0 && id < a.pool.cap) {     // :1154 / :1234 if(!pMP || vbAlreadyMatched[i]) continue;
        const bool marked = dir ? a.already2[J.f2 + i] != 0 : a.m12Id[J.f1 + i] >= 0;
        st = ST_MARKED;
        if (!marked) {
            st = ST_BAD;
            if ((a.pool.flags[id] & 1u) == 0) {   // :1157 / :1237 ORBW_FLAG_BAD: isBad()
                const float4 A = a.pool.a[id], B = a.pool.b[id];
                const float* Rfw = dir ? J.p.R2w : J.p.R1w;
                const float* tfw = dir ? J.p.t2w : J.p.t1w;
                float pf[3];
#pragma unroll
                for (int r = 0; r < 3; r++) pf[r] = cvm::gemm3_elem(Rfw[3 * r], Rfw[3 * r + 1], Rfw[3 * r + 2], A.x, A.y, A.z, 1.0, tfw[r], 1.0);
                float u, v;
                int level, failed;
                const int to = 1 - dir;
                if (!orbf::sim3_gates(J.sR[dir], J.t[dir], pf, J.p.K1, T.bounds, A.w, B.w, a.z.nlevels, a.breaks[to], u, v, level, failed))
                    st = (uint8_t)(ST_DEPTH + failed);
                else {
                    orbf::FuseTgt tg;
                    tg.keys = T.keys; tg.desc = T.desc; tg.cellStart = T.cellStart; tg.cellIdx = T.cellIdx;
                    int bestDist, bestIdx;
                    orbf::window_best<1>(tg, J.grid, (const uint32_t*)(a.pool.desc + 2 * (size_t)id), 0, u, v, level, J.th * a.sf[to][level], bestDist, bestIdx);
                    st = ST_NO_CANDIDATE;
                    if (bestDist <= kThHigh) {   // :1223 / :1303
                        st = ST_FOUND; found = bestIdx;
                        if (bestIdx >= T.n) a.bad[blockIdx.z] = 1;   // the table of the other pass holds T.n entries: refused behind the call
                    }
                }
            }
        }
    }
    a.vn[at] = found;
    a.status[at] = st;
}

__global__ __launch_bounds__(kLanes) void k_compute_sim3(Args a, int nJobs)
{
    __shared__ double sRec[orbz::kRecords * 8];
    __shared__ orbg::LmShared<7> sLm;
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= nJobs) return;
    const JobDev& J = a.jobs[j];
    const int n1 = J.kf[0].n, n2 = J.kf[1].n, f1 = J.f1;
    const int nDev1 = *J.kf[0].nKeys, nDev2 = *J.kf[1].nKeys;
    const int32_t* vn1 = a.vn + J.f12;
    const int32_t* vn2 = vn1 + n1;
    bool bad = a.bad[j] != 0;   // the search's finding
    int nFound = 0, nCorr = 0;
    for (int c = 0; c < n1; c += kLanes) {
        const int i = c + lane;
        const bool live = i < n1;
        // the agreement (ORBmatcher.cc:1309-1325)
        const int idx2 = live ? vn1[i] : -1;
        const bool isNew = idx2 >= 0 && idx2 < n2 && vn2[idx2] == i;
        const int mId = live ? a.m12Id[f1 + i] : -1, mIdx = live ? a.m12Idx2[f1 + i] : -1;
        int match = -1, id2 = -1, i2 = -1;
        if (isNew) {
            // (pass 2->1 matched from this feature: it is below the stride and holds a point of the pool)
            const int e2 = idx2 < a.stride ? J.kf[1].entries[idx2] : -1;
            bad |= e2 < 0;
            if (e2 >= 0) { match = idx2; id2 = e2 & ~orbu::kNoVote; i2 = (e2 & orbu::kNoVote) ? -1 : idx2; }
        } else if (mId >= 0) { match = mIdx; id2 = mId; i2 = mIdx; }
        if (id2 >= a.pool.cap) { bad = true; id2 = -1; match = -1; }   // (the host has checked the entering ids, the search the entries)
        nFound += __popcll(__ballot(isNew));
        // the walk (Optimizer.cc:1401-1440)
        const int e1 = live && i < a.stride ? J.kf[0].entries[i] : -1;
        const int id1 = e1 >= 0 && (e1 & ~orbu::kNoVote) < a.pool.cap ? e1 & ~orbu::kNoVote : -1;
        bool has = id2 >= 0 && id1 >= 0 && i2 >= 0;
        if (has) has = ((a.pool.flags[id1] | a.pool.flags[id2]) & 1u) == 0;   // :1421
        // a correspondence at a feature the resident slots do not hold: refused after the kernel
        if (has && (i >= nDev1 || i2 >= nDev2 || i2 >= n2)) { bad = true; has = false; }
        const unsigned long long m = __ballot(has);
        const int cIdx = nCorr + below(m, lane);
        if (has) {
            const orbm::KeyDev k1 = J.kf[0].keys[i], k2 = J.kf[1].keys[i2];
            const float4 X1 = a.pool.a[id1], X2 = a.pool.a[id2];
            const bool ok1 = k1.octave >= 0 && k1.octave < a.z.nlevels, ok2 = k2.octave >= 0 && k2.octave < a.z.nlevels;
            bad |= !ok1 || !ok2;
            // edge 2c (e12): pKF2's point against pKF1's observation; edge 2c + 1 (e21): pKF1's point against pKF2's.  The points go
            // down in WORLD coordinates: the edge's own lane moves them into the camera frame behind the barrier
            const int e = 2 * f1 + 2 * cIdx;
            a.z.pw[e] = make_float4(X2.x, X2.y, X2.z, ok1 ? a.z.invSigma2[k1.octave] : 0.f);
            a.z.uv[e] = make_float2(k1.x, k1.y);
            a.z.off[e] = 0;
            a.z.pw[e + 1] = make_float4(X1.x, X1.y, X1.z, ok2 ? a.z.invSigma2[ORBX_MAX_LEVELS + k2.octave] : 0.f);
            a.z.uv[e + 1] = make_float2(k2.x, k2.y);
            a.z.off[e + 1] = 0;
            a.z.removed[f1 + cIdx] = 0;
        }
        if (live) { a.match[f1 + i] = match; a.id2[f1 + i] = id2; a.corrOf[f1 + i] = has ? cIdx : -1; }
        nCorr += __popcll(m);
    }
    const bool anyBad = __any(bad);
    if (lane == 0) { a.out[j].n_found = nFound; a.out[j].n_corr = nCorr; if (anyBad) a.bad[j] = 1; }
    __syncthreads();
    if (anyBad) return;
    // k_sim3_optimize's gather (Optimizer.cc:1421, :1429): the OTHER keyframe's point in ITS camera frame, R * Xw + t through gemm's
    // small branch, by the lane that owns the edge in the solve
    {
        const int side = lane & 1;
        const float* R = side ? J.p.R1w : J.p.R2w;
        const float* t = side ? J.p.t1w : J.p.t2w;
        for (int e = lane; e < 2 * nCorr; e += kLanes) {
            const float4 X = a.z.pw[2 * f1 + e];
            float P[3];
#pragma unroll
            for (int r = 0; r < 3; r++) P[r] = cvm::gemm3_elem(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], X.x, X.y, X.z, 1.0, t[r], 1.0);
            a.z.pw[2 * f1 + e] = make_float4(P[0], P[1], P[2], X.w);
        }
    }
    orbz::solve_problem(a.z, J.p, J.delta, f1, nCorr, &a.out[j].opt, sRec, sLm, lane);
    __syncthreads();
    // :1497, :1532: vpMatches1[idx] = NULL for a pair either check removed; every other match stays, with or without an edge
    for (int c = 0; c < n1; c += kLanes) {
        const int i = c + lane;
        if (i >= n1) break;
        const int cc = a.corrOf[f1 + i];
        const bool gone = cc >= 0 && a.z.removed[f1 + cc] != 0;
        a.matchOut[f1 + i] = gone ? -1 : a.match[f1 + i];
        a.idsOut[f1 + i] = gone ? -1 : a.id2[f1 + i];
    }
}

}  // namespace orby
