// orbq_reloc_kernels.hip -- Tracking::Relocalization behind PnPsolver::iterate (Tracking.cc:1486-1547) on the device (part of
// orbslamm_hip.hip; host side: orbq_reloc_host.inc, ABI: include/orbslamm_reloc.h), for a batch of jobs in a fixed
// chain of launches:
//   k_reloc_stage(BEGIN)    one wave a job: the ids as they came into the frame's point list and into sFound, solve 1, the gates
//                           of :1505 and :1513, the discard of :1508-1510, the occupancy the wide search starts from
//   k_reloc_project(wide)   one thread a row entry: the gates of ORBmatcher.cc:1490-1530 into the query block and a device-made
//                           orbt::ProjPair (nq = 0 for a job that has left)
//   k_proj_candidates + k_proj_resolve (orbt_kernels.hip, mode 5, ORBdist 100)
//   k_reloc_stage(MIDDLE)   the matches into the point list, the gate of :1517, solve 2, the gate of :1523, sFound rebuilt
//   k_reloc_project(narrow), the two search kernels again (ORBdist 64)
//   k_reloc_stage(END)      the matches, the gate of :1532, solve 3 with the discard
// Every kernel is launched whatever the jobs' exits: a job that has left makes its pair empty and touches nothing more.
// The stage kernel is §8s's: merge_and_gather over an id source (the point list itself), orbo::solve_frame, and a loop behind the
// solve that keeps the outlier byte of a feature no solve had as an edge.  sFound is a per-job open-addressed table of 2 *
// pow2ceil(n) words (-1: empty), filled by compare-and-swap by the stage kernel and read by the projection kernel, behind a kernel
// boundary; membership does not depend on the order of insertion.  No other atomics; every loop is bounded by the job's n, the
// table's size, the stride or a constant.
#pragma once

namespace orbq {

enum : int32_t { RELOC_REJECTED = 0, RELOC_FIRST, RELOC_WIDE_SHORT, RELOC_SECOND, RELOC_NARROW_SHORT, RELOC_THIRD };
enum : uint8_t { RST_NOT_RUN = 0, RST_NO_POINT, RST_BAD, RST_FOUND, RST_OUT_OF_IMAGE, RST_DISTANCE, RST_LEVEL_RANGE, RST_IN_VIEW };
enum : int32_t { RELOC_BEGIN = 0, RELOC_MIDDLE, RELOC_END };
enum : int32_t { RELOC_LIVE = 0, RELOC_LEFT, RELOC_OVERFLOW };
constexpr uint8_t kRelocKeep = 0xff;   // ORBQ_RELOC_KEEP
constexpr int kRelocThreads = 256;

struct RelocJobDev {
    float Tcw[16];
    float K[4];
    float bounds[4];            // mnMinX, mnMaxX, mnMinY, mnMaxY
    orbt::TrainSide cur;        // the current slot: its mvKeysUn and device count (the merge reads them), the search's train side
    const float* kfAng;         // the keyframe slot's angles
    const int32_t* nKf;         // ... and its device count
    const int32_t* entries;     // the keyframe's row of the store
    const int32_t* ids;         // [n] the job's ids as they came (the call's upload)
    int32_t n, f0;              // f0: where the job's features (and its edges) start in the call's per-feature arrays
    int32_t cap, c0;            // the set's cap; where the job's share of the per-train arrays starts
    int32_t tab0, tabMask;      // the job's sFound table: tabMask + 1 words from tab0
    int32_t t0, pad;            // where the job's share of the resolve's per-train tables starts (ProjCommon::big), in ints
};
struct RelocArgs {
    Args q;                     // q.jobs, q.out unused; q.merged and q.idsOut are ONE array: the frame's point list
    const RelocJobDev* jobs;
    OrbqRelocResult* out;
    int32_t* state;             // [job] RELOC_LIVE / _LEFT / _OVERFLOW
    int32_t* need;              // [job][2] candidate entries a search that overflowed asked for
    int32_t* bad;               // [job] a row entry with a point at or above the keyframe slot's device count
    int32_t* table;             // the sFound tables
    // the searches' blocks: per train feature from c0, per row entry from job * stride
    uint8_t* tocc; uint8_t* toccOut; int32_t* assign;
    float* quvr; int8_t* qlvl; uint4* qdesc; uint8_t* qvalid; uint8_t* status;   // status: [job][2][stride]
    int32_t* candOff; int32_t* candCnt; int32_t* qres; int32_t* qscr; int32_t* tscr; int32_t* total; int32_t* nmatch;
    uint2* cand; int32_t candCap;   // the arena: candCap entries a job
    orbt::ProjPair* pairs;
    int32_t stride;
    float scale[ORBX_MAX_LEVELS], breaks[ORBX_MAX_LEVELS + 1];
};

// the frame's point list as its own id source: first(t) is the id, id() hands it on
struct ListSource {
    const int32_t* list;
    __device__ __forceinline__ int first(int t, int n) const { return t < n ? list[t] : -1; }
    __device__ __forceinline__ int id(int, int, int q, bool&) const { return q; }
};

__device__ __forceinline__ uint32_t reloc_hash(int id, int mask) { return ((uint32_t)id * 2654435761u >> 7) & (uint32_t)mask; }

// (one wave) the job's table cleared when `clear`, then every id of the list put in
__device__ __forceinline__ void found_fill(int32_t* tab, int mask, const int32_t* list, int n, int lane, bool clear)
{
    if (clear) {
        for (int i = lane; i <= mask; i += kLanes) tab[i] = -1;
        __syncthreads();
    }
    for (int t = lane; t < n; t += kLanes) {
        const int id = list[t];
        if (id < 0) continue;
        uint32_t s = reloc_hash(id, mask);
        for (int probe = 0; probe <= mask; probe++, s = (s + 1) & (uint32_t)mask) {   // (at most half the words are ever taken)
            const int old = atomicCAS(&tab[s], -1, id);
            if (old == -1 || old == id) break;
        }
    }
}
__device__ __forceinline__ bool found_has(const int32_t* tab, int mask, int id)
{
    uint32_t s = reloc_hash(id, mask);
    for (int probe = 0; probe <= mask; probe++, s = (s + 1) & (uint32_t)mask) {
        const int v = tab[s];
        if (v == id) return true;
        if (v == -1) return false;
    }
    return false;
}

// Optimizer.cc:410 / :416 mvbOutlier[idx] for every feature that was an edge of the solve just run (the others keep their byte);
// with `discard` Tracking.cc:1508-1510 / :1536-1538: an outlier loses its point
__device__ __forceinline__ void reloc_behind_solve(const Args& a, int n, int f0, bool discard, int lane)
{
    int e0 = 0;
    for (int c = 0; c < n; c += kLanes) {
        const int t = c + lane;
        const int id = t < n ? a.merged[f0 + t] : -1;
        const unsigned long long m = __ballot(id >= 0);
        if (id >= 0) {
            const uint8_t o = a.o.outlier[f0 + e0 + below(m, lane)];
            a.outlierOut[f0 + t] = o ? 1 : 0;
            if (o && discard) a.merged[f0 + t] = -1;
        }
        e0 += __popcll(m);
    }
}

__global__ __launch_bounds__(kLanes) void k_reloc_stage(RelocArgs r, int nJobs, int stage)
{
    __shared__ orbg::LmShared<6> sLm;
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= nJobs) return;
    const RelocJobDev& J = r.jobs[j];
    const Args& a = r.q;
    const int n = J.n, f0 = J.f0, nDev = *J.cur.n, nt = min(nDev, J.cap);
    OrbqRelocResult* out = r.out + j;
    int32_t* list = a.merged + f0;
    int32_t* tab = r.table + J.tab0;
    if (stage != RELOC_BEGIN && r.state[j] != RELOC_LIVE) return;   // (wave-uniform)
    int nGoodBefore = 0, nAdd = 0;
    if (stage == RELOC_BEGIN) {
        // :1492-1501 mvpMapPoints[j] = vvpMapPointMatches[i][j] or NULL; sFound.insert
        for (int t = lane; t < n; t += kLanes) list[t] = J.ids[t];
        __syncthreads();
        found_fill(tab, J.tabMask, list, n, lane, false);
    } else {
        const int s = stage - 1;
        const int nm = r.nmatch[j];
        if (nm < 0) {
            if (lane == 0) report_overflow(nm, &r.need[2 * j + s], &r.state[j], RELOC_OVERFLOW);
            return;
        }
        // ORBmatcher.cc:1559 CurrentFrame.mvpMapPoints[bestIdx2] = pMP, behind the pruning of :1587-1597
        for (int t = lane; t < min(n, nt); t += kLanes) {
            const int q = r.assign[J.c0 + t];
            if (q >= 0 && q < r.stride) list[t] = J.entries[q] & ~orbu::kNoVote;
        }
        nAdd = nm; nGoodBefore = out->n_good[s];
        const bool shortOf = nAdd + nGoodBefore < 50;   // :1517 / :1532
        if (lane == 0) {
            out->n_additional[s] = nAdd;
            if (shortOf) { out->exit = s == 0 ? RELOC_WIDE_SHORT : RELOC_NARROW_SHORT; r.state[j] = RELOC_LEFT; }
        }
        if (shortOf) return;
        __syncthreads();
    }
    // :1503 / :1519 / :1534 PoseOptimization(&mCurrentFrame), from the pose the frame holds
    bool bad = false;
    const ListSource src = {list};
    const int nEdges = merge_and_gather(a, src, J.cur.keys, n, f0, nDev, lane, true, bad);
    const bool anyBad = __any(bad);
    __syncthreads();
    OrboResult* opt = &out->opt[stage];
    orbo::solve_frame(a.o, stage == RELOC_BEGIN ? J.Tcw : out->Tcw, J.K, f0, nEdges, anyBad, opt, sLm, lane);
    __syncthreads();
    if (anyBad) {   // (the host refuses the call: opt[0].rounds says so)
        if (lane == 0) { out->opt[0].rounds = -1; r.state[j] = RELOC_LEFT; }
        return;
    }
    const int nGood = opt->n_good;   // (written by lane 0 in front of the barrier)
    // solve 1: nGood < 10 leaves before the discard (:1505); solve 2 discards nothing (:1519-1523); solve 3 discards (:1536-1538)
    const bool discard = stage == RELOC_BEGIN ? nGood >= 10 : stage == RELOC_END;
    reloc_behind_solve(a, n, f0, discard, lane);
    int exit = -1;
    if (stage == RELOC_BEGIN) exit = nGood < 10 ? RELOC_REJECTED : nGood >= 50 ? RELOC_FIRST : -1;
    else if (stage == RELOC_MIDDLE) exit = nGood >= 50 || nGood <= 30 ? RELOC_SECOND : -1;   // :1523 if(nGood>30 && nGood<50)
    else exit = RELOC_THIRD;
    if (lane == 0) {
        for (int i = 0; i < 16; i++) out->Tcw[i] = opt->Tcw[i];
        out->n_good[stage] = nGood;
        if (exit >= 0) { out->exit = exit; r.state[j] = RELOC_LEFT; }
    }
    if (exit >= 0) return;
    __syncthreads();
    // :1525-1528 sFound.clear(); insert every point the frame holds (solve 2's outliers included)
    if (stage == RELOC_MIDDLE) found_fill(tab, J.tabMask, list, n, lane, true);
    // :1543 if(CurrentFrame.mvpMapPoints[i2]) continue;  a feature at or above n takes no part
    for (int t = lane; t < J.cap; t += kLanes) r.tocc[J.c0 + t] = t >= n || list[t] >= 0 ? 1 : 0;
}

// ORBmatcher.cc:1490-1530 for entry q of job blockIdx.y's row, at the pose the job's frame holds; thread 0 of the job's first
// workgroup makes the pair record the two search kernels read
__global__ __launch_bounds__(kRelocThreads) void k_reloc_project(RelocArgs r, int search, float th)
{
    const int j = blockIdx.y;
    const RelocJobDev& J = r.jobs[j];
    const bool live = r.state[j] == RELOC_LIVE;
    const int64_t q0 = (int64_t)j * r.stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        orbt::ProjPair P;
        proj_train(P, J.cur);
        proj_unused(P);
        P.quvr = r.quvr + 3 * q0; P.qlvl = r.qlvl + 2 * q0; P.qdesc = (const uint8_t*)(r.qdesc + 2 * q0); P.qang = J.kfAng;
        P.qvalid = r.qvalid + q0; P.qobs = nullptr;
        P.nqPtr = nullptr; P.nq = live ? r.stride : 0;
        P.toccIn = r.tocc + J.c0; P.toccOut = r.toccOut + J.c0;
        P.assign = r.assign + J.c0; P.initAssign = 1;
        P.nmatch = r.nmatch + j;
        P.total = r.total + j;
        P.candOff = r.candOff + q0; P.candCnt = r.candCnt + q0;
        P.cand = r.cand + (int64_t)j * r.candCap; P.candCap = r.candCap;
        P.qres = r.qres + q0; P.qscr = r.qscr + 3 * q0;
        P.tscr = r.tscr ? r.tscr + J.t0 : nullptr;
        r.pairs[j] = P;
    }
    const int q = blockIdx.x * kRelocThreads + threadIdx.x;
    if (!live || q >= r.stride) return;
    const float* T = r.out[j].Tcw;
    float u = 0.f, v = 0.f, rad = 0.f;
    int level = -1;
    uint8_t st = RST_NO_POINT;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    const int e = J.entries[q];
    const int id = e & ~orbu::kNoVote;
    if (e >= 0 && id < r.q.pool.cap && q >= *J.nKf) r.bad[j] = 1;   // (the keyframe slot holds no key q: refused behind the call)
    else if (e >= 0 && id < r.q.pool.cap) {
        const uint32_t flags = r.q.pool.flags[id];
        st = RST_BAD;
        if (!(flags & 1u)) {                                                                   // :1496 !pMP->isBad()
            st = RST_FOUND;
            if (!found_has(r.table + J.tab0, J.tabMask, id)) {                                 // :1496 !sAlreadyFound.count(pMP)
                const float4 A = r.q.pool.a[id], B = r.q.pool.b[id];
                d0 = r.q.pool.desc[2 * (size_t)id]; d1 = r.q.pool.desc[2 * (size_t)id + 1];
                float Ow[3], pc[3];
#pragma unroll
                for (int i = 0; i < 3; i++) {                                                  // :1480 Ow = -Rcw.t()*tcw
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 3; k++) s += (double)T[4 * k + i] * (double)T[4 * k + 3];
                    Ow[i] = (float)(s * -1.0);
                    pc[i] = cvm::gemm3_elem(T[4 * i], T[4 * i + 1], T[4 * i + 2], A.x, A.y, A.z, 1.0, T[4 * i + 3], 1.0);   // :1500
                }
                const float invzc = (float)(1.0 / (double)pc[2]);                              // :1504 (no depth gate)
                u = J.K[0] * pc[0] * invzc + J.K[2]; v = J.K[1] * pc[1] * invzc + J.K[3];      // :1506-1507
                st = RST_OUT_OF_IMAGE;
                if (u >= J.bounds[0] && u <= J.bounds[1] && v >= J.bounds[2] && v <= J.bounds[3]) {   // :1509-1512
                    const float PO[3] = {A.x - Ow[0], A.y - Ow[1], A.z - Ow[2]};               // :1515
                    const float dist = (float)cvm::norm3(PO);                                  // :1516
                    const float maxDistance = 1.2f * B.w, minDistance = 0.8f * A.w;            // :1518-1519
                    st = RST_DISTANCE;
                    if (!(dist < minDistance || dist > maxDistance)) {                         // :1522
                        st = RST_LEVEL_RANGE;
                        if (orbf::predict_level(B.w, dist, r.q.o.nlevels, r.breaks, level)) {           // :1525 PredictScale by the break table
                            st = RST_IN_VIEW;
                            rad = th * r.scale[level];                                         // :1528
                        }
                    }
                }
            }
        }
    }
    r.quvr[3 * (q0 + q)] = u; r.quvr[3 * (q0 + q) + 1] = v; r.quvr[3 * (q0 + q) + 2] = rad;
    r.qlvl[2 * (q0 + q)] = (int8_t)(level - 1); r.qlvl[2 * (q0 + q) + 1] = (int8_t)(level + 1);   // :1530
    r.qdesc[2 * (q0 + q)] = d0; r.qdesc[2 * (q0 + q) + 1] = d1;                                   // :1535 pMP->GetDescriptor()
    r.qvalid[q0 + q] = st == RST_IN_VIEW ? 1 : 0;
    r.status[(2 * (int64_t)j + search) * r.stride + q] = st;
}

}  // namespace orbq
