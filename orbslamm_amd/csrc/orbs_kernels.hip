// orbs_kernels.hip -- Sim3Solver (src/Sim3Solver.cc) on the device: Horn's closed form per RANSAC hypothesis and the
// two-way reprojection count of CheckInliers, for every hypothesis of every solver of a batch.
//
// One orbs_run is one chain on the handle's stream with the host in the middle once:
//   k_sim3_fit      one hypothesis per lane: centroids, M = Pr2 * Pr1^T (double sums), N, JacobiImpl_<float> on the 4x4
//                   (arrays in LDS, one column per lane); leaves the quaternion evec.row(0)
//   (host)          atan2, cos and sin in binary64 through libm, as the reference calls them: the quaternion becomes R12
//   k_sim3_pose     one hypothesis per lane: P3 = R*Pr2, the scale, t12, T12 and T21
//   k_sim3_score    the hot path: one wave per hypothesis over the solver's points (staged in LDS up to kLdsPoints, streamed
//                   beyond), two projections and two comparisons a point; the count is an integer, so the order of
//                   its sum is free: ballot + popcount per pass
//   k_sim3_mask     the inlier flags of ONE hypothesis (the one iterate returns)
//   k_sim3_points   the constructor: Rcw*Xw + tcw, FromCameraToImage and the size_t thresholds, one point per lane
// Arithmetic: one IEEE operation per source operation (the library is built with -ffp-contract=off), float and double
// division and sqrt correctly rounded.  OpenCV's pieces follow its 3.0 source and are unpinned.
#pragma once

#include <cfloat>

namespace orbs {

constexpr int kMaxPoints = 65535;
constexpr int kMaxIterations = 4096;
constexpr int kFitThreads = 64;
constexpr int kPoseThreads = 64;
constexpr int kScoreThreads = 256;
constexpr int kHypPerBlock = 8;        // hypotheses of one solver a score block takes (two per wave)
constexpr int kLdsPoints = 1024;       // points a score block stages in LDS (48 bytes each)
constexpr int kPointThreads = 256;
constexpr int kHypWords = 30;          // OrbsHypothesis: n_inliers, s12, T12[16], R12[9], t12[3]
constexpr int kPoseWords = 24;         // rows 0..2 of T12, then of T21

// a solver as the kernels see it.  pts: three planes of n float4: (X1c, maxError1), (X2c, maxError2), (p1im1, p2im2)
struct Desc {
    const float4* pts;
    float* pose;          // iters x kPoseWords, kept by the solver for k_sim3_mask
    int32_t n, iters, hypBase, fixScale;
    float K1[4], K2[4];
};

// the solver of global hypothesis g: the last c with desc[c].hypBase <= g
__device__ __forceinline__ int find_solver(const Desc* __restrict__ desc, int count, int g)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].hypBase <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// OpenCV 3.0 arithmetic: orbx_cvmath.hpp
using cvm::expr_scale; using cvm::gemm3_elem; using cvm::hypot_cv;
// gemm3_elem with a NaN product defined as x86 defines it.  In mt12i = gemm(R, O2, -s, O1, 1) a NaN t (from a NaN R) meets
// alpha = -s, a NaN of the OPPOSITE sign: IEEE leaves the sign of the product open, the host's multiply returns its
// first operand (t, as the restatement compiles), and the device compiler may move the negation.  Written out, so that
// the stored NaN's bits are the host's.
__device__ __forceinline__ float gemm3_elem_nan_first(float a0, float a1, float a2, float b0, float b1, float b2, double alpha, float c, double beta)
{
    const float t = a0 * b0 + a1 * b1 + a2 * b2;
    const double td = (double)t;
    double p = td * alpha;
    if (td != td) p = td;
    else if (alpha != alpha) p = alpha;
    return (float)(p + (double)c * beta);
}

// ComputeCentroid of both point sets of a hypothesis: P (3x3, one point per column), Pr = P - C, O = C
__device__ __forceinline__ void centered(const float4* __restrict__ plane, const int32_t* __restrict__ set, float Pr[9], float O[3])
{
    float P[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float4 x = plane[set[i]];
        P[0 * 3 + i] = x.x; P[1 * 3 + i] = x.y; P[2 * 3 + i] = x.z;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        // cv::reduce SUM over columns (reduceC_): (p0 + p2) + p1; then C/P.cols: convertTo with alpha = 1./3
        float a0 = P[r * 3 + 0];
        const float a1 = P[r * 3 + 1];
        a0 = a0 + P[r * 3 + 2];
        O[r] = expr_scale(a0 + a1, 1. / 3);
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) Pr[r * 3 + i] = P[r * 3 + i] - O[r];
}

// ------------------------------------------------------------------ constructor
// rec: host-packed (X1w, sigma2_1), (X2w, sigma2_2) as two planes of n float4; out: the three planes of Desc::pts
__global__ __launch_bounds__(kPointThreads) void k_sim3_points(const float4* __restrict__ in, int n, const float* __restrict__ cam, float4* __restrict__ out)
{
    const int i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= n) return;
    // cam: Rcw1 (9), tcw1 (3), Rcw2 (9), tcw2 (3), K1 (4), K2 (4)
    float4 p;
#pragma unroll
    for (int f = 0; f < 2; f++) {
        const float* R = cam + f * 12;
        const float* t = R + 9;
        const float* K = cam + 24 + f * 4;
        const float4 w = in[f * n + i];
        float X[3];
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = gemm3_elem(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], w.x, w.y, w.z, 1.0, t[r], 1.0);
        // mvnMaxError: (size_t)(9.210 * sigma2), compared as a float
        const float th = (float)(unsigned long long)(9.210 * (double)w.w);
        out[f * n + i] = make_float4(X[0], X[1], X[2], th);
        const float invz = 1 / X[2];
        const float x = X[0] * invz;
        const float y = X[1] * invz;
        if (f == 0) { p.x = K[0] * x + K[2]; p.y = K[1] * y + K[3]; }
        else { p.z = K[0] * x + K[2]; p.w = K[1] * y + K[3]; }
    }
    out[2 * n + i] = p;
}

// ------------------------------------------------------------------ fit
// quat[g*4 ..] = evec.row(0) of hypothesis g (global over the batch); sets: 3 indices per hypothesis, in the same order
__global__ __launch_bounds__(kFitThreads) void k_sim3_fit(const Desc* __restrict__ desc, int count, int total, const int32_t* __restrict__ sets,
                                                          float* __restrict__ quat)
{
    __shared__ float sA[16 * kFitThreads];
    __shared__ float sV[16 * kFitThreads];
    __shared__ float sW[4 * kFitThreads];
    __shared__ int sR[4 * kFitThreads];
    __shared__ int sC[4 * kFitThreads];
    const int t = threadIdx.x, g = blockIdx.x * kFitThreads + t;
    if (g >= total) return;   // (no barrier below)
    const Desc& d = desc[find_solver(desc, count, g)];
    float Pr1[9], Pr2[9], O1[3], O2[3];
    centered(d.pts, sets + (size_t)g * 3, Pr1, O1);
    centered(d.pts + d.n, sets + (size_t)g * 3, Pr2, O2);
    // M = Pr2*Pr1.t() (GEMM_2_T: the generic kernel, double sums).  cvm::mm3_t2 written out: through the call the compiler
    // swaps the operands of these multiplies and adds, and the operand order decides which NaN's payload survives (the
    // tests compare NaN results as bits)
    float M[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)Pr2[i * 3 + k] * (double)Pr1[j * 3 + k];
            M[i * 3 + j] = (float)(s * 1.0);
        }
#define SM(r, c) M[(r) * 3 + (c)]
    const float N11 = SM(0, 0) + SM(1, 1) + SM(2, 2), N12 = SM(1, 2) - SM(2, 1), N13 = SM(2, 0) - SM(0, 2), N14 = SM(0, 1) - SM(1, 0);
    const float N22 = SM(0, 0) - SM(1, 1) - SM(2, 2), N23 = SM(0, 1) + SM(1, 0), N24 = SM(2, 0) + SM(0, 2);
    const float N33 = -SM(0, 0) + SM(1, 1) - SM(2, 2), N34 = SM(1, 2) + SM(2, 1), N44 = -SM(0, 0) - SM(1, 1) + SM(2, 2);
#undef SM
    // cv::eigen: JacobiImpl_<float>, n = 4 (only the upper triangle of A is read)
#define A_(i) sA[(i) * kFitThreads + t]
#define V_(i) sV[(i) * kFitThreads + t]
#define W_(i) sW[(i) * kFitThreads + t]
#define IR_(i) sR[(i) * kFitThreads + t]
#define IC_(i) sC[(i) * kFitThreads + t]
    {
        const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
#pragma unroll
        for (int i = 0; i < 16; i++) { A_(i) = Nm[i]; V_(i) = (i % 5 == 0) ? 1.f : 0.f; }
    }
    constexpr int n = 4;
    const float eps = FLT_EPSILON;
    int i, k, m;
    float mv;
    for (k = 0; k < n; k++) {
        W_(k) = A_((n + 1) * k);
        if (k < n - 1) {
            for (m = k + 1, mv = fabsf(A_(n * k + m)), i = k + 2; i < n; i++) {
                const float val = fabsf(A_(n * k + i));
                if (mv < val) mv = val, m = i;
            }
            IR_(k) = m;
        }
        if (k > 0) {
            for (m = 0, mv = fabsf(A_(k)), i = 1; i < k; i++) {
                const float val = fabsf(A_(n * i + k));
                if (mv < val) mv = val, m = i;
            }
            IC_(k) = m;
        }
    }
    for (int iters = 0; iters < n * n * 30; iters++) {
        for (k = 0, mv = fabsf(A_(IR_(0))), i = 1; i < n - 1; i++) {
            const float val = fabsf(A_(n * i + IR_(i)));
            if (mv < val) mv = val, k = i;
        }
        int l = IR_(k);
        for (i = 1; i < n; i++) {
            const float val = fabsf(A_(n * IC_(i) + i));
            if (mv < val) mv = val, k = IC_(i), l = i;
        }
        const float p = A_(n * k + l);
        if (fabsf(p) <= eps) break;
        const float y = (float)((double)(W_(l) - W_(k)) * 0.5);
        float tt = fabsf(y) + hypot_cv(p, y);
        float s = hypot_cv(p, tt);
        const float c = tt / s;
        s = p / s; tt = (p / tt) * p;
        if (y < 0) s = -s, tt = -tt;
        A_(n * k + l) = 0;
        W_(k) = W_(k) - tt;
        W_(l) = W_(l) + tt;
        float a0, b0;
#define ROT(x0, x1) a0 = x0, b0 = x1, x0 = a0 * c - b0 * s, x1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) ROT(A_(n * i + k), A_(n * i + l));
        for (i = k + 1; i < l; i++) ROT(A_(n * k + i), A_(n * i + l));
        for (i = l + 1; i < n; i++) ROT(A_(n * k + i), A_(n * l + i));
        for (i = 0; i < n; i++) ROT(V_(n * k + i), V_(n * l + i));
#undef ROT
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = fabsf(A_(n * idx + m)), i = idx + 2; i < n; i++) {
                    const float val = fabsf(A_(n * idx + i));
                    if (mv < val) mv = val, m = i;
                }
                IR_(idx) = m;
            }
            if (idx > 0) {
                for (m = 0, mv = fabsf(A_(idx)), i = 1; i < idx; i++) {
                    const float val = fabsf(A_(n * i + idx));
                    if (mv < val) mv = val, m = i;
                }
                IC_(idx) = m;
            }
        }
    }
    // the descending sort moves whole rows of V; only row 0's final content is needed: the row of the largest W, the
    // first of equals (the selection's `W[m] < W[i]` at k = 0)
    m = 0;
    for (i = 1; i < n; i++) if (W_(m) < W_(i)) m = i;
#pragma unroll
    for (i = 0; i < 4; i++) quat[(size_t)g * 4 + i] = V_(n * m + i);
#undef A_
#undef V_
#undef W_
#undef IR_
#undef IC_
}

// ------------------------------------------------------------------ pose
// rot[g*9 ..]: mR12i from the host.  Writes OrbsHypothesis g (all but n_inliers) and the solver's pose rows.
__global__ __launch_bounds__(kPoseThreads) void k_sim3_pose(const Desc* __restrict__ desc, int count, int total, const int32_t* __restrict__ sets,
                                                            const float* __restrict__ rot, float* __restrict__ hyp)
{
    const int g = blockIdx.x * kPoseThreads + threadIdx.x;
    if (g >= total) return;
    const Desc& d = desc[find_solver(desc, count, g)];
    float Pr1[9], Pr2[9], O1[3], O2[3], R[9];
    centered(d.pts, sets + (size_t)g * 3, Pr1, O1);
    centered(d.pts + d.n, sets + (size_t)g * 3, Pr2, O2);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rot[(size_t)g * 9 + k];
    // P3 = mR12i*Pr2 (cvm::mm3 written out, for the operand order of its multiplies: see k_sim3_fit's M)
    float P3[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            P3[i * 3 + j] = gemm3_elem(R[i * 3], R[i * 3 + 1], R[i * 3 + 2], Pr2[j], Pr2[3 + j], Pr2[6 + j], 1.0, 0.f, 0.0);
    float s12;
    if (!d.fixScale) {
        double nom = 0, den = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) nom += (double)Pr1[k] * (double)P3[k];
#pragma unroll
        for (int k = 0; k < 9; k++) den += (double)(P3[k] * P3[k]);   // cv::pow(P3, 2): float squares, summed in double
        s12 = (float)(nom / den);
    } else
        s12 = 1.0f;
    // mt12i = O1 - ms12i*mR12i*O2: gemm(R, O2, -s, O1, 1)
    float t12[3], sR[9], sRinv[9], tinv[3];
#pragma unroll
    for (int r = 0; r < 3; r++) t12[r] = gemm3_elem_nan_first(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], O2[0], O2[1], O2[2], -(double)s12, O1[r], 1.0);
#pragma unroll
    for (int k = 0; k < 9; k++) sR[k] = expr_scale(R[k], (double)s12);
    const double ainv = 1.0 / s12;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) sRinv[r * 3 + c] = ainv != 1.0 ? (float)((double)R[c * 3 + r] * ainv) : R[c * 3 + r];
#pragma unroll
    for (int r = 0; r < 3; r++) tinv[r] = gemm3_elem(sRinv[r * 3], sRinv[r * 3 + 1], sRinv[r * 3 + 2], t12[0], t12[1], t12[2], -1.0, 0.f, 0.0);
    float* o = hyp + (size_t)g * kHypWords;
    o[1] = s12;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) o[2 + r * 4 + c] = sR[r * 3 + c];
        o[2 + r * 4 + 3] = t12[r];
    }
    o[2 + 12] = 0.f; o[2 + 13] = 0.f; o[2 + 14] = 0.f; o[2 + 15] = 1.f;
#pragma unroll
    for (int k = 0; k < 9; k++) o[18 + k] = R[k];
#pragma unroll
    for (int r = 0; r < 3; r++) o[27 + r] = t12[r];
    float* ps = d.pose + (size_t)(g - d.hypBase) * kPoseWords;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { ps[r * 4 + c] = sR[r * 3 + c]; ps[12 + r * 4 + c] = sRinv[r * 3 + c]; }
        ps[r * 4 + 3] = t12[r];
        ps[12 + r * 4 + 3] = tinv[r];
    }
}

// ------------------------------------------------------------------ score
// Project of one point and its squared distance to q: Rcw*X + tcw through gemm's small branch, then the pinhole in float
__device__ __forceinline__ float reproj_err(const float* __restrict__ T, float X, float Y, float Z, const float* __restrict__ K, float qx, float qy, bool projFirst)
{
    const float cx = gemm3_elem(T[0], T[1], T[2], X, Y, Z, 1.0, T[3], 1.0);
    const float cy = gemm3_elem(T[4], T[5], T[6], X, Y, Z, 1.0, T[7], 1.0);
    const float cz = gemm3_elem(T[8], T[9], T[10], X, Y, Z, 1.0, T[11], 1.0);
    const float invz = 1 / cz;
    const float x = cx * invz;
    const float y = cy * invz;
    const float u = K[0] * x + K[2], v = K[1] * y + K[3];
    // dist1 = mvP1im1 - vP2im1, dist2 = vP1im2 - mvP2im2; Mat::dot sums in double
    const float dx = projFirst ? u - qx : qx - u, dy = projFirst ? v - qy : qy - v;
    double s = 0;
    s += (double)dx * (double)dx;
    s += (double)dy * (double)dy;
    return (float)s;
}
// CheckInliers' test of one point: a = (X1c, maxError1), b = (X2c, maxError2), c = (p1im1, p2im2); T: rows of T12, then T21
__device__ __forceinline__ bool is_inlier(const float4 a, const float4 b, const float4 c, const float* __restrict__ T, const float* __restrict__ K1,
                                          const float* __restrict__ K2)
{
    const float err1 = reproj_err(T, b.x, b.y, b.z, K1, c.x, c.y, false);
    const float err2 = reproj_err(T + 12, a.x, a.y, a.z, K2, c.z, c.w, true);
    return err1 < a.w && err2 < b.w;
}

// grid (ceil(max iters / kHypPerBlock), solvers); counts land in word 0 of each OrbsHypothesis
__global__ __launch_bounds__(kScoreThreads) void k_sim3_score(const Desc* __restrict__ desc, int32_t* __restrict__ hyp)
{
    __shared__ float4 sPts[3 * kLdsPoints];
    __shared__ float sT[kHypPerBlock * kPoseWords];
    const Desc& d = desc[blockIdx.y];
    const int h0 = blockIdx.x * kHypPerBlock;
    if (h0 >= d.iters) return;   // (block-uniform)
    const int n = d.n, t = threadIdx.x;
    const int nh = min(kHypPerBlock, d.iters - h0);
    const bool staged = n <= kLdsPoints;
    if (staged)
        for (int i = t; i < 3 * n; i += kScoreThreads) sPts[i] = d.pts[i];
    for (int i = t; i < nh * kPoseWords; i += kScoreThreads) sT[i] = d.pose[(size_t)h0 * kPoseWords + i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const float* K1 = d.K1;
    const float* K2 = d.K2;
    for (int hl = wave; hl < nh; hl += kScoreThreads / 64) {
        const float* T = sT + hl * kPoseWords;
        int cnt = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            bool in = false;
            if (p < n) {
                const float4 a = staged ? sPts[p] : d.pts[p];
                const float4 b = staged ? sPts[n + p] : d.pts[n + p];
                const float4 c = staged ? sPts[2 * n + p] : d.pts[2 * (size_t)n + p];
                in = is_inlier(a, b, c, T, K1, K2);
            }
            cnt += __popcll(__ballot(in));
        }
        if (lane == 0) hyp[(size_t)(d.hypBase + h0 + hl) * kHypWords] = cnt;
    }
}

// the flags of one hypothesis (pose: its kPoseWords)
__global__ __launch_bounds__(kPointThreads) void k_sim3_mask(const float4* __restrict__ pts, int n, const float* __restrict__ pose, const float* __restrict__ cam,
                                                             uint8_t* __restrict__ out)
{
    const int p = blockIdx.x * kPointThreads + threadIdx.x;
    if (p >= n) return;
    out[p] = is_inlier(pts[p], pts[n + p], pts[2 * (size_t)n + p], pose, cam + 24, cam + 28) ? 1 : 0;
}

}  // namespace orbs
