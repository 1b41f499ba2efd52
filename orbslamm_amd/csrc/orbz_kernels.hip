// orbz_kernels.hip -- device OptimizeSim3 (part of orbslamm_hip.hip; host side: orbz_host.inc, ABI: include/orbslamm_sim3opt.h,
// DESIGN.md §8p): Optimizer::OptimizeSim3 (src/Optimizer.cc:1348-1543), monocular, for a batch of loop / merge candidates in ONE
// launch.  One wave owns a problem from its first pass to its last.  Correspondence c owns edge 2c (e12: S12 maps pKF2's point into
// camera 1) and edge 2c + 1 (e21: the inverse maps pKF1's point into camera 2); edge e is lane e % 64's, always, so even lanes hold
// e12 edges and odd lanes e21 edges and the difference between them is DATA (which record set, which K, which point), not control
// flow.  Every lane keeps its partial H (28), b (7) and chi2 in registers and the sums are closed by the xor butterfly 32 .. 1 --
// THE SUMMATION TREE of §8o over the edge index.
// g2o differentiates these edges NUMERICALLY (linearizeOplus is commented out in types_seven_dof_expmap.h): 14 perturbed
// estimates Sim3(+-1e-9 e_d) * S per linearisation.  They and their inverses depend on the problem, not on the edge: lanes 0 .. 13
// compute them once into LDS (with the base estimate 30 records of 8 doubles) and every edge evaluates its 15 errors from there.
// This file keeps what is OptimizeSim3's own: the records, the gather, the Sim3 with its oplus (the constructor's A / B / C
// branches, the product with no normalisation) and inverse, the numeric Jacobian from the LDS records, the two passes, the check
// and the result.  The Levenberg run, the 7 x 7 pivoted LDLT, the defined sin / cos and exp, the quaternion and so(3) pieces and
// the edge record are orbg_kernels.hip's, shared with PoseOptimization.
// Binary64 throughout, -ffp-contract=off, no atomics; every loop is bounded at compile time (2 passes, 5 / 10
// iterations, 10 trials, kMaxEdgesPerLane edges).  A lane reads back only per-edge words that the same lane wrote.
// The two passes, the checks and the result are a device function (solve_problem) so that k_compute_sim3 (orby_kernels.hip, DESIGN.md
// §8v) runs them behind its own gather: the same bytes for the same correspondence list.
#pragma once

namespace orbz {

constexpr int kLanes = 64;
constexpr int kMaxCorr = 32767;                  // ORBZ_MAX_CORR
constexpr int kMaxProblems = 4096;               // ORBZ_MAX_PROBLEMS
constexpr int kMaxEdgesPerLane = (2 * kMaxCorr + kLanes - 1) / kLanes;
constexpr int kPasses = 2;
constexpr int kRecords = 30;                     // (base + 14 perturbed) x (itself, its inverse)

struct ProblemIn {
    OrbzProblem p;
    double delta;        // (double)sqrtf(th2): the Huber width (:1398), taken on the host
    int32_t c0, n;
};
struct Args {
    const ProblemIn* problems;
    const OrbzCorr* corrs;
    float4* pw;          // per edge: the camera-frame point, invSigma2 (written and read by the edge's lane)
    float2* uv;          // per edge: the observation
    uint8_t* off;        // per edge: its pair was removed by the first check (written and read by the edge's lane)
    OrbzResult* out;
    uint8_t* removed;    // per correspondence: the output (written by the even lane, never read here)
    const float* invSigma2;   // the two keyframes' level tables, ORBX_MAX_LEVELS floats each
    int32_t nlevels;
};

using orbg::Cam;
using orbg::EdgeReg;
using orbg::edge_chi2;
using orbg::huber;
using orbg::load_edge;
using orbg::nan_canon;
using orbg::wave_sum;

struct S3 { orbg::Quat q; double tx, ty, tz, s; };

// Sim3::inverse: Sim3(conj, conj * ((-1. / s) * t), 1. / s)
__host__ __device__ __forceinline__ S3 inverse(const S3& S)
{
    S3 o;
    o.q.x = -S.q.x; o.q.y = -S.q.y; o.q.z = -S.q.z; o.q.w = S.q.w;
    const double f = -1. / S.s;
    orbg::rotate(o.q, f * S.tx, f * S.ty, f * S.tz, o.tx, o.ty, o.tz);
    o.s = 1. / S.s;
    return o;
}

// Sim3(update) * P: the constructor's four branches (types/sim3.h:70-142), then operator* with NO normalisation
__host__ __device__ inline __noinline__ S3 oplus(const S3 P, double w0, double w1, double w2, double u0, double u1, double u2, double sigma)
{
    const orbg::So3Exp e = orbg::so3_exp(w0, w1, w2);
    const double theta = e.theta, sn = e.sn, cs = e.cs;
    const bool smallTheta = e.small;
    const double Id[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    S3 E;
    E.s = orbg::exp_defined(sigma);
    double A, B, C;
    if (fabs(sigma) < 0.00001) {
        C = 1;
        if (smallTheta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cs) / (theta2);
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (E.s - 1) / sigma;
        if (smallTheta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * E.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * E.s) / (sigma2 * sigma);
        } else {
            const double a = E.s * sn, b = E.s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    E.q = orbg::quat_of_matrix(e.R);
    double W[9];
#pragma unroll
    for (int k = 0; k < 9; k++) W[k] = (A * e.Om[k] + B * e.Om2[k]) + C * Id[k];
    E.tx = (W[0] * u0 + W[1] * u1) + W[2] * u2;
    E.ty = (W[3] * u0 + W[4] * u1) + W[5] * u2;
    E.tz = (W[6] * u0 + W[7] * u1) + W[8] * u2;
    S3 O;
    O.q = orbg::quat_mul(E.q, P.q);
    double rx, ry, rz;
    orbg::rotate(E.q, P.tx, P.ty, P.tz, rx, ry, rz);
    O.tx = E.s * rx + E.tx; O.ty = E.s * ry + E.ty; O.tz = E.s * rz + E.tz;
    O.s = E.s * P.s;
    return O;
}

__device__ __forceinline__ void store_record(double* rec, const S3& S)
{
    rec[0] = S.q.x; rec[1] = S.q.y; rec[2] = S.q.z; rec[3] = S.q.w; rec[4] = S.tx; rec[5] = S.ty; rec[6] = S.tz; rec[7] = S.s;
}
__device__ __forceinline__ S3 load_record(const double* rec)
{
    S3 S;
    S.q.x = rec[0]; S.q.y = rec[1]; S.q.z = rec[2]; S.q.w = rec[3]; S.tx = rec[4]; S.ty = rec[5]; S.tz = rec[6]; S.s = rec[7];
    return S;
}

// computeError of either edge type: obs - cam_map(project(S.map(P))), S being the estimate or its inverse by the edge's side
__device__ __forceinline__ void edge_error(const S3& S, const Cam& K, const EdgeReg& E, double& e0, double& e1)
{
    double rx, ry, rz;
    orbg::rotate(S.q, E.X, E.Y, E.Z, rx, ry, rz);
    orbg::pinhole_error(K, E, S.s * rx + S.tx, S.s * ry + S.ty, S.s * rz + S.tz, e0, e1);
}

// computeActiveErrors + activeRobustChi2 at estimate S (Sinv its inverse; the lane's side picks)
__device__ __forceinline__ double pass_chi2(const Args& a, int e0, int nE, int lane, const S3& mine, const Cam& K, double delta, double delta2)
{
    double part = 0.0;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= nE) break;
        if (a.off[e0 + e]) continue;
        const EdgeReg E = load_edge(a.pw[e0 + e], a.uv[e0 + e]);
        double r0, r1, cost, weight;
        edge_error(mine, K, E, r0, r1);
        huber(edge_chi2(E, r0, r1), delta, delta2, cost, weight);
        part = part + cost;
    }
    return wave_sum(part);
}

// the same chi2 sum fused with buildSystem at the estimate: the numeric Jacobian from the records in LDS, H's lower triangle
// (row by row), b, chi2.  rec: the lane's side's record set, 15 records at a stride of 16 doubles
__device__ __forceinline__ void pass_build(const Args& a, int e0, int nE, int lane, const double* rec, const Cam& K, double delta, double delta2,
                                           double (&H)[28], double (&b)[7], double& chiOut)
{
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 28; i++) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) b[i] = 0.0;
    const double scalar = 1.0 / (2 * 1e-9);
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= nE) break;
        if (a.off[e0 + e]) continue;
        const EdgeReg E = load_edge(a.pw[e0 + e], a.uv[e0 + e]);
        double r0, r1;
        edge_error(load_record(rec), K, E, r0, r1);
        double B0[7], B1[7];
#pragma unroll
        for (int d = 0; d < 7; d++) {
            double p0, p1, m0, m1;
            edge_error(load_record(rec + (1 + 2 * d) * 16), K, E, p0, p1);
            edge_error(load_record(rec + (2 + 2 * d) * 16), K, E, m0, m1);
            B0[d] = scalar * (p0 - m0);
            B1[d] = scalar * (p1 - m1);
        }
        double cost, weight;
        huber(edge_chi2(E, r0, r1), delta, delta2, cost, weight);
        chi = chi + cost;
        // constructQuadraticForm, robust, the `to` vertex: omega_r = -(Omega e), *= weight; b += B^T omega_r; H += (B^T (weight Omega)) B
        double g0 = -(E.w00 * r0 + E.w01 * r1), g1 = -(E.w10 * r0 + E.w11 * r1);
        g0 = g0 * weight; g1 = g1 * weight;
        const double W00 = weight * E.w00, W01 = weight * E.w01, W10 = weight * E.w10, W11 = weight * E.w11;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 7; i++) {
            b[i] = b[i] + (B0[i] * g0 + B1[i] * g1);
            const double t0 = B0[i] * W00 + B1[i] * W10, t1 = B0[i] * W01 + B1[i] * W11;
#pragma unroll
            for (int j = 0; j <= i; j++, q++) H[q] = H[q] + (t0 * B0[j] + t1 * B1[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 28; i++) H[i] = wave_sum(H[i]);
#pragma unroll
    for (int i = 0; i < 7; i++) b[i] = wave_sum(b[i]);
    chiOut = wave_sum(chi);
}

// what orbg::levenberg runs on: the problem's edges at an estimate, the lane's side picking the Sim3 or its inverse
struct Problem {
    const Args& a;
    int e0, nE, lane, side;
    Cam K;
    bool fixScale;
    double delta, delta2;
    double* rec;   // the records in LDS, see the kernel
    S3 est, err;   // err: where the active edges' _error was last computed
    __device__ __forceinline__ void build(double (&H)[28], double (&b)[7], double& chi) const
    {
        __syncthreads();   // (the last linearisation's reads of the records are done)
        if (lane < 15) {
            // lane 14: the estimate; lanes 0 .. 13: the step +-delta along dimension lane / 2 (with its scale entry zeroed
            // under fix_scale, as oplusImpl zeroes it)
            const int d = lane >> 1;
            const double step = lane == 14 ? 0.0 : ((lane & 1) ? -1e-9 : 1e-9);
            const S3 Sp = lane == 14 ? est
                                     : orbz::oplus(est, d == 0 ? step : 0.0, d == 1 ? step : 0.0, d == 2 ? step : 0.0, d == 3 ? step : 0.0,
                                                   d == 4 ? step : 0.0, d == 5 ? step : 0.0, (d == 6 && !fixScale) ? step : 0.0);
            const int j = lane == 14 ? 0 : 1 + lane;
            store_record(rec + (2 * j) * 8, Sp);
            store_record(rec + (2 * j + 1) * 8, inverse(Sp));
        }
        __syncthreads();
        pass_build(a, e0, nE, lane, rec + side * 8, K, delta, delta2, H, b, chi);
    }
    __device__ __forceinline__ void step(double (&x)[7]) const { if (fixScale) x[6] = 0; }   // oplusImpl writes the zero into the solver's x
    __device__ __forceinline__ S3 oplus(const double (&x)[7]) const { return orbz::oplus(est, x[0], x[1], x[2], x[3], x[4], x[5], x[6]); }
    __device__ __forceinline__ double chi2(const S3& cand) const
    {
        const S3 candInv = inverse(cand);
        return pass_chi2(a, e0, nE, lane, side ? candInv : cand, K, delta, delta2);
    }
};

// One problem from its estimate to its result (Optimizer.cc:1484-1541): the two optimize() passes, the two checks, the early return
// of :1514 and the recovered Sim3.  The problem's n correspondences own the edges 2 c0 .. 2 (c0 + n) of a.pw / a.uv / a.off, filled
// by the caller's gather (edge 2c: e12, edge 2c + 1: e21; nothing removed yet, a.removed zero) and made visible to the wave before
// the call.  sRec: the records, [j][side] at (2 j + side) * 8, j = 0 the estimate, 1 + 2 d the +delta step of dimension d, 2 + 2 d
// the -delta step; side 0 the Sim3 itself (e12 edges), side 1 its inverse (e21 edges).  The body of k_sim3_optimize, which is its
// first caller; k_compute_sim3 (orby_kernels.hip) is the second.
__device__ __forceinline__ void solve_problem(const Args& a, const OrbzProblem& P, double delta, int c0, int n, OrbzResult* out, double* sRec,
                                              orbg::LmShared<7>& sLm, int lane)
{
    const int side = lane & 1, e0 = 2 * c0, nE = 2 * n;
    S3 est0;
    est0.q.x = P.q[0]; est0.q.y = P.q[1]; est0.q.z = P.q[2]; est0.q.w = P.q[3];
    est0.tx = P.t[0]; est0.ty = P.t[1]; est0.tz = P.t[2]; est0.s = P.s;
    if (lane == 0) {
        out->q[0] = est0.q.x; out->q[1] = est0.q.y; out->q[2] = est0.q.z; out->q[3] = est0.q.w;
        out->t[0] = est0.tx; out->t[1] = est0.ty; out->t[2] = est0.tz; out->s = est0.s;
        out->written = 0; out->n_corr = n; out->n_bad = 0; out->n_in = 0;
        for (int r = 0; r < kPasses; r++) { out->iterations[r] = 0; out->trials[r] = 0; out->lambda[r] = 0.0; out->chi2[r] = 0.0; }
    }
    if (n == 0) return;   // no edge: no vertex is found, no iteration runs, and 0 - 0 < 10 (:1514)

    const float* Kf = side ? P.K2 : P.K1;   // cam_map1 for e12, cam_map2 for e21
    const double th2 = (double)P.th2;
    Problem p = {a, e0, nE, lane, side, {(double)Kf[0], (double)Kf[1], (double)Kf[2], (double)Kf[3]}, P.fix_scale != 0, delta, delta * delta, sRec, est0, est0};
    orbg::LmState<7> lm;   // lambda, growth, flatSteps and the solver's x: they live across the passes
    int nBad = 0, nIn = 0;
    const int kEdgeRounds = (nE + kLanes - 1) / kLanes;
    for (int pass = 0; pass < kPasses; pass++) {
        const int maxIt = pass == 0 ? 5 : (nBad > 0 ? 10 : 5);   // :1485, :1508-1512
        p.err = p.est;
        const orbg::LmRun run = orbg::levenberg<7>(p, sLm, lm, maxIt, lane);
        // the check (:1489-1506, :1523-1537): both edges of a pair with the error of the last trial's estimate; the pair's two lanes
        // exchange their chi2.  The loop bound is wave-uniform so that both lanes of every pair reach the exchange
        const S3 errInv = inverse(p.err);
        const S3 mine = side ? errInv : p.err;
        int bad = 0, in = 0;
        for (int k = 0; k < kMaxEdgesPerLane; k++) {
            if (k >= kEdgeRounds) break;
            const int e = lane + k * kLanes;
            const bool live = e < nE && a.off[e0 + (e < nE ? e : 0)] == 0;
            double c = 0.0;
            if (live) {
                const EdgeReg E = load_edge(a.pw[e0 + e], a.uv[e0 + e]);
                double r0, r1;
                edge_error(mine, p.K, E, r0, r1);
                c = edge_chi2(E, r0, r1);
            }
            const double other = __shfl_xor(c, 1, kLanes);
            if (live) {
                const bool fails = c > th2 || other > th2;
                if (fails) {
                    if (pass == 0) a.off[e0 + e] = 1;
                    if (!side) a.removed[c0 + (e >> 1)] = (uint8_t)(pass + 1);
                }
                if (!side) { bad += fails; in += !fails; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { bad += __shfl_xor(bad, m, kLanes); in += __shfl_xor(in, m, kLanes); }
        if (pass == 0) nBad = bad;
        else nIn = in;
        if (lane == 0) {
            out->iterations[pass] = run.iterations; out->trials[pass] = run.trials;
            out->lambda[pass] = nan_canon(lm.lambda); out->chi2[pass] = nan_canon(run.chi2);
            out->n_bad = nBad;
        }
        if (pass == 0 && n - nBad < 10) return;   // :1514: before g2oS12 is written; the nulled matches stay nulled
    }
    if (lane == 0) {
        const S3& est = p.est;
        out->q[0] = nan_canon(est.q.x); out->q[1] = nan_canon(est.q.y); out->q[2] = nan_canon(est.q.z); out->q[3] = nan_canon(est.q.w);
        out->t[0] = nan_canon(est.tx); out->t[1] = nan_canon(est.ty); out->t[2] = nan_canon(est.tz); out->s = nan_canon(est.s);
        out->written = 1;
        out->n_in = nIn;
    }
}

__global__ __launch_bounds__(kLanes) void k_sim3_optimize(Args a, int nProblems)
{
    __shared__ double sRec[kRecords * 8];
    __shared__ orbg::LmShared<7> sLm;
    const int pIdx = blockIdx.x, lane = threadIdx.x, side = lane & 1;
    if (pIdx >= nProblems) return;
    const ProblemIn& P = a.problems[pIdx];
    const int c0 = P.c0, n = P.n, e0 = 2 * c0, nE = 2 * n;
    // the gather (Optimizer.cc:1401-1481): the observation, its level's information and the OTHER keyframe's point in ITS camera
    // frame (R * Xw + t through gemm's small branch, as orbs_create takes it); nothing removed yet
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= nE) break;
        const OrbzCorr c = a.corrs[c0 + (e >> 1)];
        const float* R = side ? P.p.R1w : P.p.R2w;
        const float* t = side ? P.p.t1w : P.p.t2w;
        const float* Xw = side ? c.X1w : c.X2w;
        const int oct = side ? c.oct2 : c.oct1;
        float X[3];
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = cvm::gemm3_elem(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], Xw[0], Xw[1], Xw[2], 1.0, t[r], 1.0);
        const bool okOct = oct >= 0 && oct < a.nlevels;   // (the host has refused anything else)
        a.pw[e0 + e] = make_float4(X[0], X[1], X[2], okOct ? a.invSigma2[side * ORBX_MAX_LEVELS + oct] : 0.f);
        a.uv[e0 + e] = side ? make_float2(c.obs2[0], c.obs2[1]) : make_float2(c.obs1[0], c.obs1[1]);
        a.off[e0 + e] = 0;
        if (!side) a.removed[c0 + (e >> 1)] = 0;
    }
    solve_problem(a, P.p, P.delta, c0, n, a.out + pIdx, sRec, sLm, lane);
}

}  // namespace orbz
