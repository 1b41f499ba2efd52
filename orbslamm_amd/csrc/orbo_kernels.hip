// orbo_kernels.hip -- device PoseOptimization (part of orbslamm_hip.hip; host side: orbo_host.inc, ABI:
// include/orbslamm_poseopt.h): Optimizer::PoseOptimization (src/Optimizer.cc:261-473), monocular, for a
// batch of frames in ONE launch.  One wave owns a frame from its first round to its last: the frame's edges are strided over
// the 64 lanes (edge e is lane e % 64's, always), every lane keeps its partial H (21), b (6) and chi2 in registers, and the
// sums are closed by the xor butterfly 32, 16, ..., 1 -- THE SUMMATION TREE of §8o, a function of the edge count alone.
// This file keeps what is PoseOptimization's own: the records, the gather, the SE3 pose with its oplus (SE3Quat::exp's V, the
// normalising product), the analytic Jacobian of EdgeSE3ProjectXYZOnlyPose with the `robust` switch, the four rounds, the
// classification and the result.  The Levenberg run, the 6 x 6 pivoted LDLT, the defined sin / cos, the quaternion and so(3)
// pieces and the edge record are orbg_kernels.hip's, shared with OptimizeSim3.
// Binary64 throughout, built with -ffp-contract=off, no atomics; every loop is bounded at compile time (4 rounds, 10
// iterations, 10 trials, kMaxEdgesPerLane edges), so no input can make the kernel spin.
// A lane reads back only per-edge words that the same lane wrote (the gathered edges, the outlier bytes): no fence is needed.
#pragma once

namespace orbo {

constexpr int kLanes = 64;
constexpr int kMaxEdges = 65535;                 // ORBO_MAX_EDGES
constexpr int kMaxFrames = 4096;                 // ORBO_MAX_FRAMES
constexpr int kMaxEdgesPerLane = (kMaxEdges + kLanes - 1) / kLanes;
constexpr int kRounds = 4;
constexpr double kDelta = (double)2.44765191f, kDelta2 = kDelta * kDelta;   // the Huber width: (float)sqrt(5.991), widened (:295)

struct FrameIn {
    float Tcw[16];
    float K[4];
    const orbm::KeyDev* keys;   // a device-resident frame's mvKeysUn, or null: the edge's observation is in Args::obs
    int32_t nKeys, e0, n, pad;
};
struct Obs { float u, v; int32_t octave; };
struct Args {
    const FrameIn* frames;
    const OrboEdge* edges;
    const Obs* obs;
    float4* pw;          // per edge: Xw, invSigma2 (written and read by the edge's lane)
    float2* uv;          // per edge: the observation
    OrboResult* out;
    uint8_t* outlier;
    float invSigma2[ORBX_MAX_LEVELS];
    int32_t nlevels;
};

using orbg::Cam;
using orbg::EdgeReg;
using orbg::edge_chi2;
using orbg::huber;
using orbg::load_edge;
using orbg::nan_canon;
using orbg::nan_canon_f;
using orbg::pinhole_error;
using orbg::wave_sum;

struct Pose { orbg::Quat q; double tx, ty, tz; };

// Converter::toSE3Quat
__host__ __device__ __forceinline__ Pose pose_of_tcw(const float* T)
{
    const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
    Pose P;
    P.q = orbg::quat_of_matrix(R);
    P.tx = (double)T[3]; P.ty = (double)T[7]; P.tz = (double)T[11];
    orbg::normalize_rotation(P.q);
    return P;
}

// exp(dx) * P: SE3Quat::exp, then SE3Quat::operator*
__host__ __device__ inline __noinline__ Pose oplus(const Pose& P, double w0, double w1, double w2, double u0, double u1, double u2)
{
    const orbg::So3Exp e = orbg::so3_exp(w0, w1, w2);
    const double Id[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    // V = I + b Omega + d Omega^2; below the threshold V = R = I + Omega + Omega^2 with no factor
    double d = 1.0;
    if (!e.small) d = (e.theta - e.sn) / (e.theta * e.theta * e.theta);
    double V[9];
#pragma unroll
    for (int k = 0; k < 9; k++) V[k] = e.small ? ((Id[k] + e.Om[k]) + e.Om2[k]) : ((Id[k] + e.b * e.Om[k]) + d * e.Om2[k]);
    Pose E;
    E.q = orbg::quat_of_matrix(e.R);
    E.tx = (V[0] * u0 + V[1] * u1) + V[2] * u2;
    E.ty = (V[3] * u0 + V[4] * u1) + V[5] * u2;
    E.tz = (V[6] * u0 + V[7] * u1) + V[8] * u2;
    orbg::normalize_rotation(E.q);
    Pose O;
    double rx, ry, rz;
    orbg::rotate(E.q, P.tx, P.ty, P.tz, rx, ry, rz);
    O.tx = E.tx + rx; O.ty = E.ty + ry; O.tz = E.tz + rz;
    O.q = orbg::quat_mul(E.q, P.q);
    orbg::normalize_rotation(O.q);
    return O;
}

// SE3Quat::map
__device__ __forceinline__ void camera_point(const Pose& P, const EdgeReg& E, double& x, double& y, double& z)
{
    double rx, ry, rz;
    orbg::rotate(P.q, E.X, E.Y, E.Z, rx, ry, rz);
    x = rx + P.tx; y = ry + P.ty; z = rz + P.tz;
}

// computeActiveErrors + activeRobustChi2 at pose P
__device__ __noinline__ double pass_chi2(const Args& a, int e0, int n, int lane, const Pose& P, const Cam& K, bool robust)
{
    double part = 0.0;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= n) break;
        if (a.outlier[e0 + e]) continue;
        const EdgeReg E = load_edge(a.pw[e0 + e], a.uv[e0 + e]);
        double x, y, z, r0, r1;
        camera_point(P, E, x, y, z);
        pinhole_error(K, E, x, y, z, r0, r1);
        const double c = edge_chi2(E, r0, r1);
        if (robust) {
            double cost, weight;
            huber(c, kDelta, kDelta2, cost, weight);
            part = part + cost;
        } else part = part + c;
    }
    return wave_sum(part);
}

// the same chi2 sum fused with buildSystem at the estimate: H's lower triangle (row by row), b, chi2
__device__ __noinline__ void pass_build(const Args& a, int e0, int n, int lane, const Pose& P, const Cam& K, bool robust,
                                        double (&H)[21], double (&b)[6], double& chiOut)
{
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 21; i++) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) b[i] = 0.0;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= n) break;
        if (a.outlier[e0 + e]) continue;
        const EdgeReg E = load_edge(a.pw[e0 + e], a.uv[e0 + e]);
        double x, y, z, r0, r1;
        camera_point(P, E, x, y, z);
        pinhole_error(K, E, x, y, z, r0, r1);
        const double c = edge_chi2(E, r0, r1);
        double cost = c, weight = 1.0;
        if (robust) huber(c, kDelta, kDelta2, cost, weight);
        chi = chi + cost;
        // the projection's derivative by the pose increment (rotation part first), row u then row v; the order of the operations
        // is the edge type's
        const double iz = 1.0 / z, iz2 = iz * iz, xy = x * y;
        double J0[6], J1[6];
        J0[0] = xy * iz2 * K.fx;
        J0[1] = -(1.0 + x * x * iz2) * K.fx;
        J0[2] = y * iz * K.fx;
        J0[3] = -iz * K.fx;
        J0[4] = 0.0;
        J0[5] = x * iz2 * K.fx;
        J1[0] = (1.0 + y * y * iz2) * K.fy;
        J1[1] = -xy * iz2 * K.fy;
        J1[2] = -x * iz * K.fy;
        J1[3] = 0.0;
        J1[4] = -iz * K.fy;
        J1[5] = y * iz2 * K.fy;
        // constructQuadraticForm: with a kernel b -= ((weight A^T) Omega) e and H += (A^T (weight Omega)) A, without b -= (A^T Omega) e
        // and H += (A^T Omega) A
        const double W00 = robust ? weight * E.w00 : E.w00, W01 = robust ? weight * E.w01 : E.w01, W10 = robust ? weight * E.w10 : E.w10,
                     W11 = robust ? weight * E.w11 : E.w11;
        double T0[6], T1[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double l0 = robust ? weight * J0[i] : J0[i], l1 = robust ? weight * J1[i] : J1[i];
            const double g0 = l0 * E.w00 + l1 * E.w10, g1 = l0 * E.w01 + l1 * E.w11;
            b[i] = b[i] - (g0 * r0 + g1 * r1);
            T0[i] = J0[i] * W00 + J1[i] * W10;
            T1[i] = J0[i] * W01 + J1[i] * W11;
        }
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++, q++) H[q] = H[q] + (T0[i] * J0[j] + T1[i] * J1[j]);
    }
#pragma unroll
    for (int i = 0; i < 21; i++) H[i] = wave_sum(H[i]);
#pragma unroll
    for (int i = 0; i < 6; i++) b[i] = wave_sum(b[i]);
    chiOut = wave_sum(chi);
}

// what orbg::levenberg runs on: the frame's edges at a pose, under the round's `robust`.  K and est are the kernel's objects,
// held by reference: the passes and oplus are calls that take them by address, and a field whose address leaves would keep this
// whole record in memory
struct Problem {
    const Args& a;
    int e0, n, lane;
    const Cam& K;
    bool robust;
    Pose& est;
    Pose err;   // where the active edges' _error was last computed
    __device__ __forceinline__ void build(double (&H)[21], double (&b)[6], double& chi) const { pass_build(a, e0, n, lane, est, K, robust, H, b, chi); }
    __device__ __forceinline__ void step(double (&)[6]) const {}
    __device__ __forceinline__ Pose oplus(const double (&x)[6]) const { return orbo::oplus(est, x[0], x[1], x[2], x[3], x[4], x[5]); }
    __device__ __forceinline__ double chi2(const Pose& cand) const { return pass_chi2(a, e0, n, lane, cand, K, robust); }
};

// PoseOptimization behind its gather (:343-473): the frame's n edges lie in a.pw / a.uv from e0 on with their outlier bytes 0,
// edge e written where lane e % 64 reads it (by that lane, or by another with a workgroup barrier in between).  Tcw and K4 are
// the caller's pose and fx fy cx cy in memory; anyBad: an edge's octave (or, for orbq's prologue, a point) was refused -- the
// record then says rounds = -1 and the host refuses the call.  Shared by k_pose_optimize and orbq::k_track_pose.
__device__ __forceinline__ void solve_frame(const Args& a, const float* Tcw, const float* K4, int e0, int n, bool anyBad, OrboResult* out,
                                            orbg::LmShared<6>& sLm, int lane)
{
    if (lane == 0) {
        for (int i = 0; i < 16; i++) out->Tcw[i] = Tcw[i];
        out->n_initial = n; out->n_good = 0; out->rounds = anyBad ? -1 : 0;   // (-1: an octave outside nlevels; the host refuses)
        for (int r = 0; r < kRounds; r++) { out->iterations[r] = 0; out->trials[r] = 0; out->lambda[r] = 0.0; out->chi2[r] = 0.0; }
    }
    if (anyBad || n < 3) return;   // :386

    const Cam K = {(double)K4[0], (double)K4[1], (double)K4[2], (double)K4[3]};
    Pose est = pose_of_tcw(Tcw);
    Problem p = {a, e0, n, lane, K, true, est, est};
    orbg::LmState<6> lm;   // lambda, growth, flatSteps and the solver's x: they live across the rounds
    int nBad = 0, rounds = 0;
    for (int it = 0; it < kRounds; it++) {
        // every round starts from the caller's pose: mTcw is written only at the end (:399, :470)
        est = pose_of_tcw(Tcw);
        p.err = est;
        int nActive = 0;
        for (int k = 0; k < kMaxEdgesPerLane; k++) {
            const int e = lane + k * kLanes;
            if (e >= n) break;
            nActive += a.outlier[e0 + e] == 0;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nActive += __shfl_xor(nActive, m, kLanes);
        orbg::LmRun run = {0, 0, 0.0};
        if (nActive > 0) run = orbg::levenberg<6>(p, sLm, lm, orbg::kIterations, lane);
        // the classification (:404-431): level-0 edges with the error of the last trial's pose, outliers with a fresh one
        nBad = 0;
        for (int k = 0; k < kMaxEdgesPerLane; k++) {
            const int e = lane + k * kLanes;
            if (e >= n) break;
            const EdgeReg E = load_edge(a.pw[e0 + e], a.uv[e0 + e]);
            const bool was = a.outlier[e0 + e] != 0;
            double x, y, z, r0, r1;
            camera_point(was ? est : p.err, E, x, y, z);
            pinhole_error(K, E, x, y, z, r0, r1);
            const float chi2 = (float)edge_chi2(E, r0, r1);
            const bool isOut = chi2 > 5.991f;
            a.outlier[e0 + e] = isOut ? 1 : 0;
            nBad += isOut;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nBad += __shfl_xor(nBad, m, kLanes);
        if (lane == 0) {
            out->iterations[it] = run.iterations; out->trials[it] = run.trials;
            out->lambda[it] = nActive > 0 ? nan_canon(lm.lambda) : 0.0; out->chi2[it] = nan_canon(run.chi2);
        }
        if (it == 2) p.robust = false;   // :429-430
        rounds = it + 1;
        if (n < 10) break;   // :462
    }
    if (lane == 0) {
        // Converter::toCvMat(SE3Quat): toRotationMatrix, narrowed
        const double tx = 2.0 * est.q.x, ty = 2.0 * est.q.y, tz = 2.0 * est.q.z;
        const double twx = tx * est.q.w, twy = ty * est.q.w, twz = tz * est.q.w;
        const double txx = tx * est.q.x, txy = ty * est.q.x, txz = tz * est.q.x;
        const double tyy = ty * est.q.y, tyz = tz * est.q.y, tzz = tz * est.q.z;
        float* T = out->Tcw;
        T[0] = nan_canon_f(1.0 - (tyy + tzz)); T[1] = nan_canon_f(txy - twz); T[2] = nan_canon_f(txz + twy); T[3] = nan_canon_f(est.tx);
        T[4] = nan_canon_f(txy + twz); T[5] = nan_canon_f(1.0 - (txx + tzz)); T[6] = nan_canon_f(tyz - twx); T[7] = nan_canon_f(est.ty);
        T[8] = nan_canon_f(txz - twy); T[9] = nan_canon_f(tyz + twx); T[10] = nan_canon_f(1.0 - (txx + tyy)); T[11] = nan_canon_f(est.tz);
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
        out->n_good = n - nBad;
        out->rounds = rounds;
    }
}

__global__ __launch_bounds__(kLanes) void k_pose_optimize(Args a, int nFrames)
{
    __shared__ orbg::LmShared<6> sLm;
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= nFrames) return;
    const FrameIn& F = a.frames[f];
    const int e0 = F.e0, n = F.n;
    // the gather (Optimizer.cc:302-341): observation, information, world position of the lane's edges; mvbOutlier = false
    bool bad = false;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= n) break;
        const OrboEdge ed = a.edges[e0 + e];
        float u, v;
        int oct;
        if (F.keys) { const orbm::KeyDev kp = F.keys[ed.feature]; u = kp.x; v = kp.y; oct = kp.octave; }
        else { const Obs o = a.obs[e0 + e]; u = o.u; v = o.v; oct = o.octave; }
        const bool okOct = oct >= 0 && oct < a.nlevels;
        bad |= !okOct;
        a.pw[e0 + e] = make_float4(ed.Xw[0], ed.Xw[1], ed.Xw[2], okOct ? a.invSigma2[oct] : 0.f);
        a.uv[e0 + e] = make_float2(u, v);
        a.outlier[e0 + e] = 0;
    }
    solve_frame(a, F.Tcw, F.K, e0, n, __any(bad), a.out + f, sLm, lane);
}

}  // namespace orbo
