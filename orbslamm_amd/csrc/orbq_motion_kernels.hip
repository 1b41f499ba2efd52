// orbq_motion_kernels.hip -- Tracking::TrackWithMotionModel (Tracking.cc:925-969, monocular) on the device (part of
// orbslamm_hip.hip; host side: orbq_motion_host.inc, ABI: include/orbslamm_motion.h), for a batch of jobs in a fixed
// chain of launches:
//   k_motion_stage(BEGIN)    one wave a job: Tcw_pred = mVelocity * mLastFrame.mTcw (:925), the occupancy both searches start from
//   k_motion_project(0)      one thread a last-frame feature: the frame/frame gates (orbw::frame_gate) from the device-made pose into
//                            the query block and a device-made orbt::ProjPair
//   k_proj_candidates + k_proj_resolve (orbt_kernels.hip, mode 4, TH_HIGH 100)
//   k_motion_stage(MIDDLE)   the count of :935 and the retry decision of :938
//   k_motion_project(1), the two search kernels again: 2 * th for the jobs that retry, an empty pair for the others
//   k_motion_stage(END)      the merge of the table that stands, the gate of :944, §8s's solve and discard loop
// Every kernel is launched whatever the jobs do: a job that does not retry, or whose arena share overflowed, makes its pair empty.
// The stage kernel is §8s's: merge_and_gather over k_track_pose's own id source (the search's table over the job's last_ids),
// orbo::solve_frame, loop_behind_solve.  No atomics of its own; every loop is bounded by the job's n, nq, the cap or a constant.
#pragma once

namespace orbq {

enum : int32_t { MM_TRACKED = 0, MM_TOO_FEW = 1 };
enum : int32_t { MM_BEGIN = 0, MM_MIDDLE, MM_END };
enum : int32_t { MM_LIVE = 0, MM_OVERFLOW };
constexpr uint8_t kMotionNotRun = 0xff;   // ORBQ_MM_ST_NOT_RUN
constexpr int kMotionThreads = 256;

struct MotionJobDev {
    float V[16], T[16];         // mVelocity, mLastFrame.mTcw
    float K[4];
    float bounds[4];            // mnMinX, mnMaxX, mnMinY, mnMaxY
    orbt::TrainSide cur;        // the current slot: its mvKeysUn and device count (the merge reads them), the search's train side
    const orbm::KeyDev* lastKeys;   // the last slot's mvKeysUn: the octaves
    const int32_t* nLast;       // ... and its device count
    const float* lastAng; const uint8_t* lastDesc;   // ... its angles and descriptors: the search's query side
    const int32_t* ids;         // [nq] the job's last_ids (the call's upload)
    int32_t n, nq;
    int32_t f0;                 // where the job's features (and its edges) start in the call's per-feature arrays
    int32_t cap, c0;            // the set's cap; where the job's share of the per-train and per-query arrays starts
    int32_t t0;                 // where the job's share of the resolve's per-train tables starts (ProjCommon::big), in ints
};
struct MotionArgs {
    Args q;                     // q.jobs, q.out unused
    const MotionJobDev* jobs;
    OrbqMotionResult* out;
    int32_t* state;             // [job] MM_LIVE / MM_OVERFLOW
    int32_t* need;              // [job][2] candidate entries a search that overflowed asked for
    int32_t* assignOut;         // per feature: the table that stands
    // the searches' blocks, per train feature and per query from c0; assign and status: search 1's block, then search 2's
    uint8_t* tocc; uint8_t* toccOut; int32_t* assign;
    float* quvr; int8_t* qlvl; uint8_t* qvalid; uint8_t* qobs; uint8_t* status;
    int32_t* candOff; int32_t* candCnt; int32_t* qres; int32_t* qscr; int32_t* tscr; int32_t* total; int32_t* nmatch;   // nmatch: [job][2]
    uint2* cand; int32_t candCap;   // the arena: candCap entries a job
    orbt::ProjPair* pairs;
    int32_t sumCap, minMatches;
    float th;
    float scale[ORBX_MAX_LEVELS];
};

__global__ __launch_bounds__(kLanes) void k_motion_stage(MotionArgs r, int nJobs, int stage)
{
    __shared__ orbg::LmShared<6> sLm;
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= nJobs) return;
    const MotionJobDev& J = r.jobs[j];
    const Args& a = r.q;
    OrbqMotionResult* out = r.out + j;
    if (stage == MM_BEGIN) {
        // :925 mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw): gemm's small branch, one element a lane
        if (lane < 16) {
            const int row = lane >> 2, c = lane & 3;
            out->Tcw_pred[lane] = cvm::gemm4_elem(J.V[4 * row], J.V[4 * row + 1], J.V[4 * row + 2], J.V[4 * row + 3],
                                                  J.T[c], J.T[4 + c], J.T[8 + c], J.T[12 + c], 1.0, 0.f, 0.0);
        }
        // :927 / :940 every point NULL: nothing is occupied but the features at or above n, which take no part
        for (int t = lane; t < J.cap; t += kLanes) r.tocc[J.c0 + t] = t >= J.n ? 1 : 0;
        return;
    }
    if (r.state[j] != MM_LIVE) return;   // (wave-uniform)
    if (stage == MM_MIDDLE) {
        if (lane != 0) return;
        const int nm = r.nmatch[2 * j];
        if (nm < 0) { report_overflow(nm, &r.need[2 * j], &r.state[j], MM_OVERFLOW); return; }
        const int wide = nm < r.minMatches ? 1 : 0;   // :938 if(nmatches<20)
        out->n_search[0] = nm; out->n_search[1] = -1; out->wide = wide;
        return;
    }
    const int wide = out->wide;   // (written by the MIDDLE launch)
    const int nm = r.nmatch[2 * j + wide];
    if (nm < 0) {
        if (lane == 0) report_overflow(nm, &r.need[2 * j + 1], &r.state[j], MM_OVERFLOW);
        return;
    }
    const int n = J.n, f0 = J.f0, nDev = *J.cur.n;
    const int32_t* assign = r.assign + (size_t)wide * r.sumCap + J.c0;   // the table that stands (-1 behind the slot's device count)
    for (int t = lane; t < n; t += kLanes) r.assignOut[f0 + t] = assign[t];
    // :944 if(nmatches<20) return false: wave-uniform
    const bool gate = nm < r.minMatches;
    bool bad = false;
    const SearchSource src = {assign, J.ids, nullptr, J.nq};
    const int nEdges = merge_and_gather(a, src, J.cur.keys, n, f0, nDev, lane, !gate, bad);
    const bool anyBad = __any(bad);
    if (lane == 0) {
        if (wide) out->n_search[1] = nm;
        out->status = gate ? MM_TOO_FEW : MM_TRACKED;
    }
    __syncthreads();
    // (the reference returns with the matches and the predicted pose in the frame)
    if (gate) { leave_unsolved(a, n, f0, lane, anyBad, out->Tcw_pred, nm, &out->track); return; }
    orbo::solve_frame(a.o, out->Tcw_pred, J.K, f0, nEdges, anyBad, &out->track.opt, sLm, lane);   // :948
    __syncthreads();
    if (anyBad) return;
    loop_behind_solve(a, n, f0, 1, lane, &out->track);   // :950-969
}

// ORBmatcher.cc:1353-1392 for last-frame feature q of job blockIdx.y, at the pose the BEGIN stage made; pass 1 only for the jobs
// that retry.  Thread 0 of the job's first workgroup makes the pair record the two search kernels read
__global__ __launch_bounds__(kMotionThreads) void k_motion_project(MotionArgs r, int pass)
{
    const int j = blockIdx.y;
    const MotionJobDev& J = r.jobs[j];
    const bool live = r.state[j] == MM_LIVE && (pass == 0 || r.out[j].wide != 0);
    const int nq = live ? J.nq : 0;
    const int64_t c0 = J.c0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        orbt::ProjPair P;
        proj_train(P, J.cur);
        proj_unused(P);
        P.quvr = r.quvr + 3 * c0; P.qlvl = r.qlvl + 2 * c0; P.qdesc = J.lastDesc; P.qang = J.lastAng;
        P.qvalid = r.qvalid + c0; P.qobs = r.qobs + c0;
        P.nqPtr = nq > 0 ? J.nLast : nullptr; P.nq = nq;   // (a null count with nq = 0: no query at all)
        P.toccIn = r.tocc + c0; P.toccOut = r.toccOut + c0;
        P.assign = r.assign + (int64_t)pass * r.sumCap + c0; P.initAssign = 1;
        P.nmatch = r.nmatch + 2 * j + pass;
        P.total = r.total + j;
        P.candOff = r.candOff + c0; P.candCnt = r.candCnt + c0;
        P.cand = r.cand + (int64_t)j * r.candCap; P.candCap = r.candCap;
        P.qres = r.qres + c0; P.qscr = r.qscr + 3 * c0;
        P.tscr = r.tscr ? r.tscr + J.t0 : nullptr;
        r.pairs[j] = P;
    }
    const int q = blockIdx.x * kMotionThreads + threadIdx.x;
    if (q >= nq) return;
    const float* T = r.out[j].Tcw_pred;
    const float Rcw[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, tcw[3] = {T[3], T[7], T[11]};   // :1353-1354
    float u = 0.f, v = 0.f, rad = 0.f;
    int lo = 0, hi = 0;
    uint8_t st = orbw::ST_NO_POINT, obs = 0;
    const int id = J.ids[q];
    if (id >= 0 && id < r.q.pool.cap && q < *J.nLast) {   // :1357-1360 (the host has checked the ids)
        const int octave = J.lastKeys[q].octave;
        obs = (r.q.pool.flags[id] >> 1) & 1;
        lo = octave - 1; hi = octave + 1;
        st = orbw::frame_gate(Rcw, tcw, J.K[0], J.K[1], J.K[2], J.K[3], J.bounds[0], J.bounds[1], J.bounds[2], J.bounds[3],
                              pass == 0 ? r.th : 2.0f * r.th, r.scale, r.q.pool.a[id], octave, u, v, rad);
    }
    r.quvr[3 * (c0 + q)] = u; r.quvr[3 * (c0 + q) + 1] = v; r.quvr[3 * (c0 + q) + 2] = rad;
    r.qlvl[2 * (c0 + q)] = (int8_t)lo; r.qlvl[2 * (c0 + q) + 1] = (int8_t)hi;
    r.qvalid[c0 + q] = st == orbw::ST_IN_VIEW ? 1 : 0;
    r.qobs[c0 + q] = obs;
    r.status[2 * c0 + (int64_t)pass * J.nq + q] = st;
}

}  // namespace orbq
