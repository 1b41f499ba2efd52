// orbe_kernels.hip -- the device side of the correction of LoopClosing::CorrectLoop (src/LoopClosing.cc:455-524) and of
// MultiMapper::UpdatePosesAndAdd (src/MultiMapper.cc:523-595) over the keyframe store and the pool beside it (part of
// orbslamm_hip.hip; ABI: include/orbslamm_correct.h, whose rules 1 to 6 the comments cite; host side: orbe_host.inc).
//   k_ref_scatter     orbu_point_set_ref_kf's staged pairs into the store's resident mpRefKF array
//   k_poses           one thread per listed keyframe, by rank: the two Sim3, the inverse of the corrected one, the corrected pose
//                     and the new centre (rule 2); the skipped ids take the claim word nothing beats
//   k_claim           one wave per listed keyframe, its entry row once in 16-byte reads: a 64-bit atomic max of
//                     (tag, ~((rank << 13) | index)) per point (rule 3), so the owner does not depend on arrival order
//   k_rows            the same walk: pass 0 counts the entries that hold their point's claim, pass 1 places them from the row's start
//                     by ballot prefixes, in index order
//   k_scan            one workgroup: the rows' starts (rule 6's visiting order) and the total
//   k_move            one thread per moved point: rule 4, and mpRefKF gathered beside it
//   (orbr's k_mark, k_walk, k_segments, k_refresh_short / _long as they are, over the moved points with their new positions: rule 5.
//    Every centre that rule reads is the store's present one -- a listed observer of a point holds it, so its rank is not below
//    the owner's -- which is what those kernels read; the new centres reach the store in k_commit, behind them)
//   k_records         one thread per moved point: the OrbePoint record from orbr's
//   k_commit          the records into the pool's arrays, the new centres into the store's
// The claim words are never cleared per call: a later tag beats any stale word, and the host clears them when the tag wraps.
// Arithmetic: one IEEE operation per source operation (-ffp-contract=off); Eigen's quaternion pieces are orbg_kernels.hip's,
// OpenCV's orbx_cvmath.hpp's.
#pragma once

namespace orbe {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQBits = orbr::kQBits;     // a claim's key is (rank << 13) | index, below 2^30
constexpr int kNoVote = orbu::kNoVote;
constexpr int kPointWords = 13;          // OrbePoint as 32-bit words
enum { H_TOTAL = 0, H_INTS = 4 };
enum { P_ID = 0, P_SLOT, P_IDX, P_POS, P_NORMAL = 6, P_MIN = 9, P_MAX, P_NOBS, P_STATUS };

struct Sim3 { double q[4], t[3], s; };   // q: x y z w
struct KfRec {                           // OrbeKeyFrame
    Sim3 cor, non;
    float Tiw[12], Ow[3];
    int32_t nPts;
};

struct Dev {
    unsigned long long* own;    // [poolCap] the claim of a point
    const int32_t* refKf;       // [poolCap] the resident mpRefKF, or null: every id -1
    KfRec* kf;                  // [K] by rank
    Sim3* inv;                  // [K] CorrectedSwi
    int32_t* rowCnt;            // [K]
    int32_t* rowStart;          // [K]
    int32_t* hdr;               // [H_INTS]
    int32_t* ids;               // [n] the moved points in visiting order
    int32_t* ownerRank;         // [n]
    int32_t* ownerIdx;          // [n]
    int32_t* ref;               // [n]
    float* newPos;              // [3 n]
    uint32_t* out;              // [n * kPointWords]
    float* ctr;                 // the store's centres [kfcap * 3]
    orbw::PoolDev pool;
    uint32_t gen;
};
// a call's arguments where the host staged them (pinned memory, read where it lies), the keyframes by rank
struct Call {
    const int32_t* slots; const float* Tiw; const double* Scw; const int32_t* skip;
    int32_t K, anchorRank, nSkip;
};

// staged: {id, slot}; ids are distinct within a launch and inside the pool (checked on the host)
__global__ __launch_bounds__(kThreads) void k_ref_scatter(int32_t* __restrict__ refKf, int poolCap, const int2* __restrict__ staged, int n)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int2 p = staged[i];
    if (p.x >= 0 && p.x < poolCap) refKf[p.x] = p.y;
}

// Sim3(R, t, 1.0) of a float pose's rows (LoopClosing.cc:464-466, :472-474): toMatrix3d / toVector3d widen, Quaterniond(R)
__device__ __forceinline__ Sim3 sim3_of_pose(const float* T)
{
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
    const orbg::Quat q = orbg::quat_of_matrix(R);
    Sim3 o;
    o.q[0] = q.x; o.q[1] = q.y; o.q[2] = q.z; o.q[3] = q.w;
    o.t[0] = (double)T[3]; o.t[1] = (double)T[7]; o.t[2] = (double)T[11];
    o.s = 1.0;
    return o;
}

__device__ __forceinline__ orbg::Quat quat_of(const Sim3& S) { orbg::Quat q; q.x = S.q[0]; q.y = S.q[1]; q.z = S.q[2]; q.w = S.q[3]; return q; }

// Sim3::map (sim3.h:144-146): s*(r*xyz) + t
__device__ __forceinline__ void sim3_map(const Sim3& S, const double* p, double* o)
{
    double r[3];
    orbg::rotate(quat_of(S), p[0], p[1], p[2], r[0], r[1], r[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = S.s * r[i] + S.t[i];
}

// KeyFrame::SetPose (src/KeyFrame.cc:99-106) of a pose's rows: Rwc = Rcw.t(), Ow = -Rwc*tcw (gemm with alpha = -1)
__device__ __forceinline__ void set_pose(const float* T, float* Rwc, float* Ow)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rwc[3 * i + j] = T[4 * j + i];
#pragma unroll
    for (int i = 0; i < 3; i++) Ow[i] = cvm::gemm3_elem(Rwc[3 * i], Rwc[3 * i + 1], Rwc[3 * i + 2], T[3], T[7], T[11], -1.0, 0.f, 0.0);
}

__global__ __launch_bounds__(kThreads) void k_poses(Dev d, Call c)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r == 0) d.hdr[H_TOTAL] = 0;
    if (r < c.nSkip) {   // :496 mnCorrectedByKF == mpCurrentKF->mnId: the word no claim reaches
        const int id = c.skip[r];
        if (id >= 0 && id < d.pool.cap) d.own[id] = ((unsigned long long)d.gen << 32) | 0xffffffffu;
    }
    if (r >= c.K) return;
    const float* T = c.Tiw + 12 * (size_t)r;                      // :459
    KfRec o;
    o.non = sim3_of_pose(T);                                      // :472-476
    if (r == c.anchorRank) {                                      // :445, :461
#pragma unroll
        for (int k = 0; k < 4; k++) o.cor.q[k] = c.Scw[k];
#pragma unroll
        for (int k = 0; k < 3; k++) o.cor.t[k] = c.Scw[4 + k];
        o.cor.s = c.Scw[7];
    } else {
        float Twc[16], Rwc[9], Owc[3];
        set_pose(c.Tiw + 12 * (size_t)c.anchorRank, Rwc, Owc);    // :446 GetPoseInverse
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) Twc[4 * i + j] = Rwc[3 * i + j];
            Twc[4 * i + 3] = Owc[i];
        }
        Twc[12] = 0.f; Twc[13] = 0.f; Twc[14] = 0.f; Twc[15] = 1.f;
        float Tic[12];                                            // :463 Tiw*Twc, the rows that are read
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                Tic[4 * i + j] = cvm::gemm4_elem(T[4 * i], T[4 * i + 1], T[4 * i + 2], T[4 * i + 3], Twc[j], Twc[4 + j], Twc[8 + j], Twc[12 + j], 1.0, 0.f, 0.0);
        const Sim3 Sic = sim3_of_pose(Tic);                       // :464-466
        Sim3 Scw;
#pragma unroll
        for (int k = 0; k < 4; k++) Scw.q[k] = c.Scw[k];
#pragma unroll
        for (int k = 0; k < 3; k++) Scw.t[k] = c.Scw[4 + k];
        Scw.s = c.Scw[7];
        const orbg::Quat q = orbg::quat_mul(quat_of(Sic), quat_of(Scw));   // :467, sim3.h:266-272
        o.cor.q[0] = q.x; o.cor.q[1] = q.y; o.cor.q[2] = q.z; o.cor.q[3] = q.w;
        double rt[3];
        orbg::rotate(quat_of(Sic), Scw.t[0], Scw.t[1], Scw.t[2], rt[0], rt[1], rt[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) o.cor.t[k] = Sic.s * rt[k] + Sic.t[k];
        o.cor.s = Sic.s * Scw.s;
    }
    {   // :484 inverse(), sim3.h:233-236
        Sim3 v;
        v.q[0] = -o.cor.q[0]; v.q[1] = -o.cor.q[1]; v.q[2] = -o.cor.q[2]; v.q[3] = o.cor.q[3];
        const double f = -1. / o.cor.s;
        orbg::rotate(quat_of(v), f * o.cor.t[0], f * o.cor.t[1], f * o.cor.t[2], v.t[0], v.t[1], v.t[2]);
        v.s = 1. / o.cor.s;
        d.inv[r] = v;
    }
    {   // :512-518 toRotationMatrix() of the un-normalised quaternion, eigt *= (1./s), Converter::toCvSE3 narrows
        const double qx = o.cor.q[0], qy = o.cor.q[1], qz = o.cor.q[2], qw = o.cor.q[3];
        const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
        const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
        const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
        const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
        const double is = 1. / o.cor.s;
        float* M = o.Tiw;
        M[0] = (float)(1.0 - (tyy + tzz)); M[1] = (float)(txy - twz); M[2] = (float)(txz + twy); M[3] = (float)(o.cor.t[0] * is);
        M[4] = (float)(txy + twz); M[5] = (float)(1.0 - (txx + tzz)); M[6] = (float)(tyz - twx); M[7] = (float)(o.cor.t[1] * is);
        M[8] = (float)(txz - twy); M[9] = (float)(tyz + twx); M[10] = (float)(1.0 - (txx + tyy)); M[11] = (float)(o.cor.t[2] * is);
    }
    float Rwc[9];
    set_pose(o.Tiw, Rwc, o.Ow);                                   // :520
    o.nPts = 0;
    d.kf[r] = o;
}

// the claim word of entry `idx` of the keyframe of rank r: below the skipped ids' 0xffffffff, above every higher (rank, index)
__device__ __forceinline__ unsigned long long claim_word(uint32_t gen, int r, int idx)
{
    return ((unsigned long long)gen << 32) | (0xfffffffeu - (((uint32_t)r << kQBits) | (uint32_t)idx));
}
// the point an entry holds for rule 3, or -1: :492 not null, bit 30 stripped, :494 not bad
__device__ __forceinline__ int held_point(const Dev& d, int raw)
{
    if (raw < 0) return -1;
    const int id = raw & ~kNoVote;
    if (id >= d.pool.cap || (d.pool.flags[id] & 1)) return -1;
    return id;
}

__global__ __launch_bounds__(kThreads) void k_claim(orbu::StoreDev s, Dev d, Call c)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= c.K) return;   // (a whole wave)
    const int slot = c.slots[r];
    if (slot < 0 || slot >= s.kfcap) return;   // (never: checked on the host)
    const int4* row = (const int4*)(s.entries + (size_t)slot * s.pitch);
    const int n4 = s.pitch / 4;
    for (int e = lane; e < n4; e += 64) {
        const int4 v = row[e];
        const int raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int id = held_point(d, raw[q]);
            if (id >= 0) atomicMax(&d.own[id], claim_word(d.gen, r, 4 * e + q));
        }
    }
}

// place == 0: rowCnt[r] = the entries of the row that hold their point's claim; else their points into ids from rowStart[r] on
__global__ __launch_bounds__(kThreads) void k_rows(orbu::StoreDev s, Dev d, Call c, int place, int n)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= c.K) return;   // (a whole wave)
    const int slot = c.slots[r];
    if (slot < 0 || slot >= s.kfcap) return;   // (never)
    const int4* row = (const int4*)(s.entries + (size_t)slot * s.pitch);
    const int n4 = s.pitch / 4;
    const unsigned long long below = (1ull << lane) - 1;
    int base = place ? d.rowStart[r] : 0;
    for (int e0 = 0; e0 < n4; e0 += 64) {   // (the same turns for the whole wave)
        const int e = e0 + lane;
        int4 v = make_int4(-1, -1, -1, -1);
        if (e < n4) v = row[e];
        const int raw[4] = {v.x, v.y, v.z, v.w};
        int id[4], before = 0, all = 0;
        unsigned long long b[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            id[q] = held_point(d, raw[q]);
            if (id[q] >= 0 && d.own[id[q]] != claim_word(d.gen, r, 4 * e + q)) id[q] = -1;
            b[q] = __ballot(id[q] >= 0);
            before += __popcll(b[q] & below);
            all += __popcll(b[q]);
        }
        if (place) {
            int at = base + before;   // the entries of the lanes below come first, then this lane's in q order
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (id[q] < 0) continue;
                if (at >= 0 && at < n) { d.ids[at] = id[q]; d.ownerRank[at] = r; d.ownerIdx[at] = 4 * e + q; }
                at++;
            }
        }
        base += all;
    }
    if (!place && lane == 0) d.rowCnt[r] = base;
}

// rowStart = the exclusive sums of rowCnt in rank order; one workgroup, K in pieces of kThreads
__global__ __launch_bounds__(kThreads) void k_scan(Dev d, int K)
{
    __shared__ int sSum[kThreads];
    __shared__ int sRun;
    const int t = threadIdx.x;
    if (t == 0) sRun = 0;
    __syncthreads();
    for (int b0 = 0; b0 < K; b0 += kThreads) {
        const int r = b0 + t;
        const int v = r < K ? d.rowCnt[r] : 0;
        sSum[t] = v;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const int add = t >= off ? sSum[t - off] : 0;
            __syncthreads();
            sSum[t] += add;
            __syncthreads();
        }
        const int run = sRun;
        if (r < K) { d.rowStart[r] = run + sSum[t] - v; d.kf[r].nPts = v; }
        __syncthreads();
        if (t == kThreads - 1) sRun = run + sSum[t];
        __syncthreads();
    }
    if (t == 0) d.hdr[H_TOTAL] = sRun;
}

__global__ __launch_bounds__(kThreads) void k_move(Dev d, int n, int K)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int id = d.ids[i], r = d.ownerRank[i];
    if (id < 0 || id >= d.pool.cap || r < 0 || r >= K) return;   // (never: k_rows placed them)
    const float4 A = d.pool.a[id];
    const double P[3] = {(double)A.x, (double)A.y, (double)A.z};   // :500-501
    double m[3], o[3];
    sim3_map(d.kf[r].non, P, m);                                   // :502 g2oSiw.map
    sim3_map(d.inv[r], m, o);                                      //      g2oCorrectedSwi.map
#pragma unroll
    for (int k = 0; k < 3; k++) d.newPos[3 * (size_t)i + k] = (float)o[k];   // :504 toCvMat narrows
    d.ref[i] = d.refKf ? d.refKf[id] : -1;
}

__global__ __launch_bounds__(kThreads) void k_records(Dev d, const uint32_t* __restrict__ res, const int32_t* __restrict__ slots, int n, int K)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t* r = res + (size_t)i * orbr::kRecWords;
    uint32_t* o = d.out + (size_t)i * kPointWords;
    const int rk = d.ownerRank[i];
    o[P_ID] = (uint32_t)d.ids[i];
    o[P_SLOT] = (uint32_t)(rk >= 0 && rk < K ? slots[rk] : -1);   // :507
    o[P_IDX] = (uint32_t)d.ownerIdx[i];
#pragma unroll
    for (int k = 0; k < 3; k++) { o[P_POS + k] = r[orbr::R_POS + k]; o[P_NORMAL + k] = r[orbr::R_NORMAL + k]; }
    o[P_MIN] = r[orbr::R_MIN]; o[P_MAX] = r[orbr::R_MAX];
    o[P_NOBS] = r[orbr::R_NOBS];
    o[P_STATUS] = (r[orbr::R_STATUS] >> 8) & 0xff;
}

// a record whose status is not DONE carries the pool's own normal and bounds: written back, they change nothing.  The flags
// word and the descriptors are never touched
__global__ __launch_bounds__(kThreads) void k_commit(orbu::StoreDev s, Dev d, const int32_t* __restrict__ slots, int n, int K)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < K) {
        const int slot = slots[i];
        if (slot >= 0 && slot < s.kfcap) {
#pragma unroll
            for (int k = 0; k < 3; k++) d.ctr[3 * (size_t)slot + k] = d.kf[i].Ow[k];
        }
    }
    if (i >= n) return;
    const uint32_t* o = d.out + (size_t)i * kPointWords;
    const int id = (int)o[P_ID];
    if (id < 0 || id >= d.pool.cap) return;
    d.pool.a[id] = make_float4(__uint_as_float(o[P_POS]), __uint_as_float(o[P_POS + 1]), __uint_as_float(o[P_POS + 2]), __uint_as_float(o[P_MIN]));
    d.pool.b[id] = make_float4(__uint_as_float(o[P_NORMAL]), __uint_as_float(o[P_NORMAL + 1]), __uint_as_float(o[P_NORMAL + 2]), __uint_as_float(o[P_MAX]));
}

}  // namespace orbe
