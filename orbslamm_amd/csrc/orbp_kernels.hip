// orbp_kernels.hip -- PnPsolver (src/PnPsolver.cc) on the device: EPnP per RANSAC hypothesis, CheckInliers of every
// hypothesis over every correspondence, and Refine (EPnP on a best mask's inliers) for every hypothesis that becomes the
// running best, for all solvers of a frame's relocalisation in one chain.
//
// One orbp_run is one chain on the handle's stream, the host at its end only:
//   k_pnp_fit       one hypothesis per lane: compute_pose on its 4 correspondences, all binary64; the 12x12 MtM / Ut, the
//                   6x10 L and the small SVD / QR systems live in LDS (dynamic indexing), kLaneDoubles per lane
//   k_pnp_score     the hot path: one wave per hypothesis over the solver's points (staged in LDS up to kLdsPoints,
//                   streamed beyond); the count is an integer: ballot + popcount per pass, one store per hypothesis
//   k_pnp_records   one lane per solver: the prefix strict maxima among the qualifying hypotheses (the only hypotheses
//                   whose mask Refine ever sees)
//   k_pnp_refine    one record per lane: the record's mask is recomputed point by point (never stored), compute_pose on
//                   its inliers with every sum one sequential chain in inlier order, CheckInliers of the refined pose
//   k_pnp_mask      the inlier flags of ONE pose (the one iterate returns)
//   k_pnp_gather    the constructor from a device-resident frame: P2D and sigma2 gathered from its undistorted keys
// Arithmetic: one IEEE operation per source operation (-ffp-contract=off), division and sqrt correctly rounded.  OpenCV's
// pieces (cvMulTransposed, JacobiSVDImpl_<double>, SVBkSb) follow its 3.0 source and are unpinned.
#pragma once

#include <cfloat>
#include <cstddef>

namespace orbp {

constexpr int kMaxPoints = 65535;
constexpr int kMaxIterations = 4096;
constexpr int kMaxSets = 2 * kMaxIterations;    // the OR loop runs past mRansacMaxIts: sets a solver may be given
constexpr int kFitThreads = 32;        // 32 lanes x kLaneDoubles x 8 B = 69 KiB of LDS: two blocks a CU, on two SIMDs
constexpr int kScoreThreads = 256;
constexpr int kHypPerBlock = 8;        // hypotheses of one solver a score block takes (two per wave)
constexpr int kLdsPoints = 2048;       // points a score block stages in LDS (24 bytes each)
constexpr int kPointThreads = 256;
// a lane's LDS, in doubles: At (12x12), L (6x10), the small systems (At 5x6 + Vt 5x5 + x 5, or A 6x4 + b 6), W (12)
constexpr int kAtD = 144, kLD = 60, kSmD = 60, kWD = 12;
constexpr int kLaneDoubles = kAtD + kLD + kSmD + kWD;

struct Hyp {   // OrbpHypothesis
    int32_t n, rec, rn, rok;
    double R[9], t[3], rR[9], rt[3];
};

// a solver as the kernels see it
struct Desc {
    const float4* pts;    // (P3Dw, sigma2) per correspondence
    const float2* uv;     // P2D
    int32_t n, iters, hypBase, minInliers;
    int32_t best0;        // the largest record count of the table this run continues (0: a new table)
    float th2;
    double fu, fv, uc, vc;
};

static_assert(offsetof(Hyp, t) == offsetof(Hyp, R) + 72 && offsetof(Hyp, rt) == offsetof(Hyp, rR) + 72,
              "the kernels read and write a pose as 12 doubles from Hyp::R / Hyp::rR: t must follow R");

struct Pose { double v[12]; };   // R row-major, then t

__device__ __forceinline__ int find_solver(const Desc* __restrict__ desc, int count, int g)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].hypBase <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// A NaN of a returned pose leaves as ONE pattern, x86's default NaN.  Which of two NaN operands an operation hands on (and
// with it the sign: a NaN born on the device is 0x7FF8..., on x86 0xFFF8..., and fabs / negation flip it on the way) is
// the compiler's choice of operand order on both sides, not something the source fixes; the tests compare NaN results as
// bits, so compute_pose's R and t are written through this (a defined choice, the restatement's too: DESIGN.md §8j).
__device__ __forceinline__ double nan_canonical(const double v)
{
    return v != v ? __longlong_as_double((long long)0xFFF8000000000000ull) : v;
}

// CheckInliers' test of one point (PnPsolver.cc:314-329): Xc, Yc, invZc are floats rounded from binary64 expressions, ue / ve
// binary64, the differences floats, the comparison in float against sigma2*th2 (a float product).  No depth test.
__device__ __forceinline__ bool is_inlier(const float4 P, const float2 q, const double* __restrict__ Rt, const double fu, const double fv,
                                          const double uc, const double vc, const float th2)
{
    const double X = (double)P.x, Y = (double)P.y, Z = (double)P.z;
    const float Xc = (float)(Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9]);
    const float Yc = (float)(Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10]);
    const float invZc = (float)(1.0 / (Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11]));
    const double ue = uc + fu * (double)Xc * (double)invZc;
    const double ve = vc + fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)q.x - ue);
    const float distY = (float)((double)q.y - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < P.w * th2;
}

// JacobiSVDImpl_<double> (cvm::jacobi_svd) as cvSVD reaches it here: n1 = n, the random completion of zero singular values
// always runs; Vt == nullptr: its rotations are skipped (nothing else depends on them)
template <int S>
__device__ __forceinline__ void jacobi_svd_d(double* At, double* W, double* Vt, const int m, const int n)
{
    cvm::jacobi_svd<double, S>(At, W, Vt, m, n, n, Vt != nullptr, true);
}

// the correspondences of a hypothesis: its set of four (a repeated point goes through as it is)
struct SetSrc {
    const float4* pts;
    const float2* uv;
    const int32_t* set;
    template <class F>
    __device__ __forceinline__ void each(F&& f) const
    {
        for (int k = 0; k < 4; k++) { const int i = set[k]; f(pts[i], uv[i]); }
    }
    template <class F>
    __device__ __forceinline__ void first(F&& f) const { const int i = set[0]; f(pts[i], uv[i]); }
};
// the correspondences of Refine: the inliers of a record's pose, in index order, the mask recomputed as it is walked
struct MaskSrc {
    const float4* pts;
    const float2* uv;
    int n, firstIdx;
    const double* Rt;
    double fu, fv, uc, vc;
    float th2;
    template <class F>
    __device__ __forceinline__ void each(F&& f) const
    {
        for (int i = firstIdx; i < n; i++) {
            const float4 P = pts[i];
            const float2 q = uv[i];
            if (is_inlier(P, q, Rt, fu, fv, uc, vc, th2)) f(P, q);
        }
    }
    template <class F>
    __device__ __forceinline__ void first(F&& f) const { f(pts[firstIdx], uv[firstIdx]); }
};

// compute_pose (PnPsolver.cc:477-525) on the nc correspondences of src; lane: this lane's LDS (kLaneDoubles doubles, S
// lanes interleaved); out: R (9, row-major) then t (3).  Every sum over the correspondences is one chain in src's order.
template <int S, class Src>
__device__ void epnp(const Src& src, const int nc, const double fu, const double fv, const double uc, const double vc, double* lane,
                     double* __restrict__ out)
{
    double* At = lane;
    double* Lm = lane + kAtD * S;
    double* Sm = Lm + kLD * S;
    double* W = Sm + kSmD * S;
#define AT(e) At[(e) * S]
#define LM(e) Lm[(e) * S]
#define SM(e) Sm[(e) * S]
    // ---- choose_control_points (:375-409)
    double c0[3] = {0, 0, 0};
    src.each([&](const float4 P, const float2) { c0[0] += (double)P.x; c0[1] += (double)P.y; c0[2] += (double)P.z; });
#pragma unroll
    for (int j = 0; j < 3; j++) c0[j] /= nc;
    {
        // cvMulTransposed(PW0, PW0tPW0, 1): the upper triangle, each entry one sum over the rows; completeSymm mirrors it
        double s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
        src.each([&](const float4 P, const float2) {
            const double x = (double)P.x - c0[0], y = (double)P.y - c0[1], z = (double)P.z - c0[2];
            s00 += x * x; s01 += x * y; s02 += x * z; s11 += y * y; s12 += y * z; s22 += z * z;
        });
        // cvSVD(MODIFY_A | U_T): At = the transposed source (symmetric)
        AT(0) = s00; AT(1) = s01; AT(2) = s02; AT(3) = s01; AT(4) = s11; AT(5) = s12; AT(6) = s02; AT(7) = s12; AT(8) = s22;
    }
    jacobi_svd_d<S>(At, W, nullptr, 3, 3);
    double cw[9];   // cws[1..3]
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double k = sqrt(W[i * S] / nc);
#pragma unroll
        for (int j = 0; j < 3; j++) cw[3 * i + j] = c0[j] + k * AT(3 * i + j);
    }
    // ---- compute_barycentric_coordinates (:411-434): cvInvert(CC, CC_inv, CV_SVD) = SVD + SVBkSb on the identity
    double ci[9];
    {
        // cc[3*i + j-1] = cws[j][i] - cws[0][i]; At = cc transposed: At[j][i] = cc[i][j]
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) AT(3 * j + i) = cw[3 * j + i] - c0[i];
        double* Vt = Sm;
        jacobi_svd_d<S>(At, W, Vt, 3, 3);
#pragma unroll
        for (int k = 0; k < 9; k++) ci[k] = 0;
        double threshold = 0;
#pragma unroll
        for (int i = 0; i < 3; i++) threshold += W[i * S];
        threshold *= DBL_EPSILON * 2;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double wi = W[i * S];
            if (fabs(wi) <= threshold) continue;
            wi = 1 / wi;
            double buf[3];
#pragma unroll
            for (int j = 0; j < 3; j++) buf[j] = AT(3 * i + j) * wi;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double s = SM(3 * i + r);
#pragma unroll
                for (int j = 0; j < 3; j++) ci[3 * r + j] = ci[3 * r + j] + s * buf[j];
            }
        }
    }
    // the alphas of one point (recomputed wherever they are needed: the same operations give the same bits)
    auto alphas = [&](const float4 P, double a[4]) {
        const double dx = (double)P.x - c0[0], dy = (double)P.y - c0[1], dz = (double)P.z - c0[2];
#pragma unroll
        for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * dx + ci[3 * j + 1] * dy + ci[3 * j + 2] * dz;
        a[0] = 1.0 - a[1] - a[2] - a[3];
    };
    // ---- M (fill_M, :436-451) and cvMulTransposed(M, MtM, 1): 78 sums over the 2n rows in row order, zeros included
#pragma unroll 1
    for (int e = 0; e < 144; e++) AT(e) = 0.;
    src.each([&](const float4 P, const float2 q) {
        double a[4];
        alphas(P, a);
        const double du = uc - (double)q.x, dv = vc - (double)q.y;
        double r[12];
#pragma unroll
        for (int k = 0; k < 4; k++) { r[3 * k] = a[k] * fu; r[3 * k + 1] = 0.0; r[3 * k + 2] = a[k] * du; }
#pragma unroll
        for (int i = 0; i < 12; i++)
#pragma unroll
            for (int j = i; j < 12; j++) AT(i * 12 + j) += r[i] * r[j];
#pragma unroll
        for (int k = 0; k < 4; k++) { r[3 * k] = 0.0; r[3 * k + 1] = a[k] * fv; r[3 * k + 2] = a[k] * dv; }
#pragma unroll
        for (int i = 0; i < 12; i++)
#pragma unroll
            for (int j = i; j < 12; j++) AT(i * 12 + j) += r[i] * r[j];
    });
#pragma unroll 1
    for (int i = 1; i < 12; i++)
        for (int j = 0; j < i; j++) AT(i * 12 + j) = AT(j * 12 + i);
    jacobi_svd_d<S>(At, W, nullptr, 12, 12);   // ut = At
    // ---- compute_L_6x10 (:760-800) and compute_rho (:802-810)
    {
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double d[4][3];   // dv[v][i]: v = 0..3 are rows 11, 10, 9, 8 of ut
#pragma unroll
            for (int v = 0; v < 4; v++)
#pragma unroll
                for (int c = 0; c < 3; c++) d[v][c] = AT((11 - v) * 12 + 3 * pa[i] + c) - AT((11 - v) * 12 + 3 * pb[i] + c);
#define DOT(a, b) (d[a][0] * d[b][0] + d[a][1] * d[b][1] + d[a][2] * d[b][2])
            LM(10 * i + 0) = DOT(0, 0);
            LM(10 * i + 1) = 2.0 * DOT(0, 1);
            LM(10 * i + 2) = DOT(1, 1);
            LM(10 * i + 3) = 2.0 * DOT(0, 2);
            LM(10 * i + 4) = 2.0 * DOT(1, 2);
            LM(10 * i + 5) = DOT(2, 2);
            LM(10 * i + 6) = 2.0 * DOT(0, 3);
            LM(10 * i + 7) = 2.0 * DOT(1, 3);
            LM(10 * i + 8) = 2.0 * DOT(2, 3);
            LM(10 * i + 9) = DOT(3, 3);
#undef DOT
        }
    }
    double rho[6];
    {
#define D2(px, py, pz, qx, qy, qz) (((px) - (qx)) * ((px) - (qx)) + ((py) - (qy)) * ((py) - (qy)) + ((pz) - (qz)) * ((pz) - (qz)))
        rho[0] = D2(c0[0], c0[1], c0[2], cw[0], cw[1], cw[2]);
        rho[1] = D2(c0[0], c0[1], c0[2], cw[3], cw[4], cw[5]);
        rho[2] = D2(c0[0], c0[1], c0[2], cw[6], cw[7], cw[8]);
        rho[3] = D2(cw[0], cw[1], cw[2], cw[3], cw[4], cw[5]);
        rho[4] = D2(cw[0], cw[1], cw[2], cw[6], cw[7], cw[8]);
        rho[5] = D2(cw[3], cw[4], cw[5], cw[6], cw[7], cw[8]);
#undef D2
    }
    // pw0 of estimate_R_and_t: the same sum for each of the three candidates
    double pw0[3] = {0, 0, 0};
    src.each([&](const float4 P, const float2) { pw0[0] += (double)P.x; pw0[1] += (double)P.y; pw0[2] += (double)P.z; });
#pragma unroll
    for (int j = 0; j < 3; j++) pw0[j] /= nc;
    // ---- the three beta approximations, each refined and scored; the winner by two strict `<` is a running strict minimum
    double bestErr = 0;
#pragma unroll 1
    for (int which = 1; which <= 3; which++) {
        // find_betas_approx_N (:667-758): cvSolve(L_6xN, Rho, B, CV_SVD) = SVD of the kept columns + SVBkSb
        const int ncol = which == 1 ? 4 : which == 2 ? 3 : 5;
        double* sAt = Sm;                   // ncol x 6
        double* sVt = Sm + 30 * S;          // ncol x ncol
        double* sX = Sm + 55 * S;           // ncol
        for (int c = 0; c < ncol; c++) {
            const int col = which == 1 ? (c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 3 : 6) : c;
            for (int i = 0; i < 6; i++) sAt[(c * 6 + i) * S] = LM(10 * i + col);
        }
        jacobi_svd_d<S>(sAt, W, sVt, 6, ncol);
        {
            for (int j = 0; j < ncol; j++) sX[j * S] = 0.;
            double threshold = 0;
            for (int i = 0; i < ncol; i++) threshold += W[i * S];
            threshold *= DBL_EPSILON * 2;
            for (int i = 0; i < ncol; i++) {
                double wi = W[i * S];
                if (fabs(wi) <= threshold) continue;
                wi = 1 / wi;
                double s = 0;
#pragma unroll
                for (int j = 0; j < 6; j++) s += sAt[(i * 6 + j) * S] * rho[j];
                s *= wi;
                for (int j = 0; j < ncol; j++) sX[j * S] = sX[j * S] + s * sVt[(i * ncol + j) * S];
            }
        }
        double betas[4];
        {
            const double b0 = sX[0], b1 = sX[1 * S], b2 = sX[2 * S], b3 = sX[3 * S];   // (b3: read only where ncol > 3)
            if (which == 1) {
                if (b0 < 0) {
                    betas[0] = sqrt(-b0);
                    betas[1] = -b1 / betas[0]; betas[2] = -b2 / betas[0]; betas[3] = -b3 / betas[0];
                } else {
                    betas[0] = sqrt(b0);
                    betas[1] = b1 / betas[0]; betas[2] = b2 / betas[0]; betas[3] = b3 / betas[0];
                }
            } else {
                if (b0 < 0) {
                    betas[0] = sqrt(-b0);
                    betas[1] = (b2 < 0) ? sqrt(-b2) : 0.0;
                } else {
                    betas[0] = sqrt(b0);
                    betas[1] = (b2 > 0) ? sqrt(b2) : 0.0;
                }
                if (b1 < 0) betas[0] = -betas[0];
                betas[2] = which == 3 ? b3 / betas[0] : 0.0;
                betas[3] = 0.0;
            }
        }
        // gauss_newton (:840-858): five steps of qr_solve on A (6x4) and b (6), in place in LDS; x starts as zeros (defined)
        {
            double* qA = Sm;             // 24
            double* qb = Sm + 24 * S;    // 6
            double x[4] = {0, 0, 0, 0};
#pragma unroll 1
            for (int step = 0; step < 5; step++) {
                for (int i = 0; i < 6; i++) {
                    const double r0 = LM(10 * i), r1 = LM(10 * i + 1), r2 = LM(10 * i + 2), r3 = LM(10 * i + 3), r4 = LM(10 * i + 4),
                                 r5 = LM(10 * i + 5), r6 = LM(10 * i + 6), r7 = LM(10 * i + 7), r8 = LM(10 * i + 8), r9 = LM(10 * i + 9);
                    qA[(i * 4 + 0) * S] = 2 * r0 * betas[0] + r1 * betas[1] + r3 * betas[2] + r6 * betas[3];
                    qA[(i * 4 + 1) * S] = r1 * betas[0] + 2 * r2 * betas[1] + r4 * betas[2] + r7 * betas[3];
                    qA[(i * 4 + 2) * S] = r3 * betas[0] + r4 * betas[1] + 2 * r5 * betas[2] + r8 * betas[3];
                    qA[(i * 4 + 3) * S] = r6 * betas[0] + r7 * betas[1] + r8 * betas[2] + 2 * r9 * betas[3];
                    double rhoi = rho[0];
#pragma unroll
                    for (int k = 1; k < 6; k++) if (i == k) rhoi = rho[k];
                    qb[i * S] = rhoi - (r0 * betas[0] * betas[0] + r1 * betas[0] * betas[1] + r2 * betas[1] * betas[1] + r3 * betas[0] * betas[2] +
                                        r4 * betas[1] * betas[2] + r5 * betas[2] * betas[2] + r6 * betas[0] * betas[3] + r7 * betas[1] * betas[3] +
                                        r8 * betas[2] * betas[3] + r9 * betas[3] * betas[3]);
                }
                // qr_solve (:860-950), nr = 6, nc = 4; its singular branch leaves x as it was and prints nothing
#define QA(i, j) qA[((i) * 4 + (j)) * S]
                double A1[4], A2[4];
                bool singular = false;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (singular) continue;
                    // the scan's pointer starts at row k while its counter starts at k+1: it reads rows k .. 4
                    double eta = fabs(QA(k, k));
                    for (int i = k + 1; i < 6; i++) { const double elt = fabs(QA(i - 1, k)); if (eta < elt) eta = elt; }
                    if (eta == 0) { singular = true; continue; }
                    double sum = 0.0;
                    const double inv_eta = 1. / eta;
                    for (int i = k; i < 6; i++) { const double v = QA(i, k) * inv_eta; QA(i, k) = v; sum += v * v; }
                    double sigma = sqrt(sum);
                    if (QA(k, k) < 0) sigma = -sigma;
                    const double akk = QA(k, k) + sigma;
                    QA(k, k) = akk;
                    A1[k] = sigma * akk;
                    A2[k] = -eta * sigma;
                    for (int j = k + 1; j < 4; j++) {
                        double s = 0;
                        for (int i = k; i < 6; i++) s += QA(i, k) * QA(i, j);
                        const double tau = s / A1[k];
                        for (int i = k; i < 6; i++) QA(i, j) -= tau * QA(i, k);
                    }
                }
                if (!singular) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        double tau = 0;
                        for (int i = j; i < 6; i++) tau += QA(i, j) * qb[i * S];
                        tau /= A1[j];
                        for (int i = j; i < 6; i++) qb[i * S] -= tau * QA(i, j);
                    }
                    x[3] = qb[3 * S] / A2[3];
                    {
                        double s = 0;
                        s += QA(2, 3) * x[3];
                        x[2] = (qb[2 * S] - s) / A2[2];
                    }
                    {
                        double s = 0;
                        s += QA(1, 2) * x[2];
                        s += QA(1, 3) * x[3];
                        x[1] = (qb[1 * S] - s) / A2[1];
                    }
                    {
                        double s = 0;
                        s += QA(0, 1) * x[1];
                        s += QA(0, 2) * x[2];
                        s += QA(0, 3) * x[3];
                        x[0] = (qb[0] - s) / A2[0];
                    }
                }
#undef QA
#pragma unroll
                for (int i = 0; i < 4; i++) betas[i] += x[i];
            }
        }
        // ---- compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
        double ccs[12];
#pragma unroll
        for (int k = 0; k < 12; k++) ccs[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 12; k++) ccs[k] += betas[i] * AT((11 - i) * 12 + k);
        auto pcs = [&](const float4 P, double pc[3]) {
            double a[4];
            alphas(P, a);
#pragma unroll
            for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
        };
        bool flip = false;
        src.first([&](const float4 P, const float2) { double pc[3]; pcs(P, pc); flip = pc[2] < 0.0; });
        double pc0[3] = {0, 0, 0};
        src.each([&](const float4 P, const float2) {
            double pc[3];
            pcs(P, pc);
#pragma unroll
            for (int j = 0; j < 3; j++) pc0[j] += flip ? -pc[j] : pc[j];
        });
#pragma unroll
        for (int j = 0; j < 3; j++) pc0[j] /= nc;
        double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        src.each([&](const float4 P, const float2) {
            double pc[3];
            pcs(P, pc);
            const double wx = (double)P.x - pw0[0], wy = (double)P.y - pw0[1], wz = (double)P.z - pw0[2];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double c = (flip ? -pc[j] : pc[j]) - pc0[j];
                abt[3 * j] += c * wx;
                abt[3 * j + 1] += c * wy;
                abt[3 * j + 2] += c * wz;
            }
        });
        // cvSVD(ABt, D, U, V, MODIFY_A): sAt rows = columns of U, sVt rows = columns of V
        double* sU = Sm;
        double* sV = Sm + 9 * S;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) sU[(i * 3 + k) * S] = abt[3 * k + i];
        jacobi_svd_d<S>(sU, W, sV, 3, 3);
        double R[9], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = sU[i * S] * sV[j * S] + sU[(3 + i) * S] * sV[(3 + j) * S] + sU[(6 + i) * S] * sV[(6 + j) * S];
        const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
        if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
#pragma unroll
        for (int r = 0; r < 3; r++) t[r] = pc0[r] - (R[3 * r] * pw0[0] + R[3 * r + 1] * pw0[1] + R[3 * r + 2] * pw0[2]);
        double sum2 = 0.0;
        src.each([&](const float4 P, const float2 q) {
            const double X = (double)P.x, Y = (double)P.y, Z = (double)P.z;
            const double Xc = (R[0] * X + R[1] * Y + R[2] * Z) + t[0];
            const double Yc = (R[3] * X + R[4] * Y + R[5] * Z) + t[1];
            const double inv_Zc = 1.0 / ((R[6] * X + R[7] * Y + R[8] * Z) + t[2]);
            const double ue = uc + fu * Xc * inv_Zc;
            const double ve = vc + fv * Yc * inv_Zc;
            const double u = (double)q.x, v = (double)q.y;
            sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
        });
        const double err = sum2 / nc;
        if (which == 1 || err < bestErr) {
            bestErr = err;
#pragma unroll
            for (int k = 0; k < 9; k++) out[k] = nan_canonical(R[k]);
#pragma unroll
            for (int k = 0; k < 3; k++) out[9 + k] = nan_canonical(t[k]);
        }
    }
#undef AT
#undef LM
#undef SM
}

// ------------------------------------------------------------------ fit
// sets: 4 indices per hypothesis, global over the batch; hyp[g].R / .t receive compute_pose of hypothesis g
__global__ __launch_bounds__(kFitThreads) void k_pnp_fit(const Desc* __restrict__ desc, int count, int total, const int32_t* __restrict__ sets,
                                                         Hyp* __restrict__ hyp)
{
    extern __shared__ double sLane[];
    const int t = threadIdx.x, g = blockIdx.x * kFitThreads + t;
    if (g >= total) return;   // (no barrier below)
    const Desc& d = desc[find_solver(desc, count, g)];
    const SetSrc src{d.pts, d.uv, sets + (size_t)g * 4};
    epnp<kFitThreads>(src, 4, d.fu, d.fv, d.uc, d.vc, sLane + t, hyp[g].R);
}

// ------------------------------------------------------------------ score
// grid (ceil(max iters / kHypPerBlock), solvers); the count lands in Hyp::n
__global__ __launch_bounds__(kScoreThreads) void k_pnp_score(const Desc* __restrict__ desc, Hyp* __restrict__ hyp)
{
    __shared__ float4 sPts[kLdsPoints];
    __shared__ float2 sUv[kLdsPoints];
    __shared__ double sT[kHypPerBlock * 12];
    const Desc& d = desc[blockIdx.y];
    const int h0 = blockIdx.x * kHypPerBlock;
    if (h0 >= d.iters) return;   // (block-uniform)
    const int n = d.n, t = threadIdx.x;
    const int nh = min(kHypPerBlock, d.iters - h0);
    const bool staged = n <= kLdsPoints;
    if (staged)
        for (int i = t; i < n; i += kScoreThreads) { sPts[i] = d.pts[i]; sUv[i] = d.uv[i]; }
    for (int i = t; i < nh * 12; i += kScoreThreads) sT[i] = hyp[d.hypBase + h0 + i / 12].R[i % 12];   // (R[9] runs on into t[3])
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const double fu = d.fu, fv = d.fv, uc = d.uc, vc = d.vc;
    const float th2 = d.th2;
    for (int hl = wave; hl < nh; hl += kScoreThreads / 64) {
        const double* T = sT + hl * 12;
        int cnt = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            bool in = false;
            if (p < n) in = is_inlier(staged ? sPts[p] : d.pts[p], staged ? sUv[p] : d.uv[p], T, fu, fv, uc, vc, th2);
            cnt += __popcll(__ballot(in));
        }
        if (lane == 0) hyp[d.hypBase + h0 + hl].n = cnt;
    }
}

// ------------------------------------------------------------------ records
// one lane per solver: hypothesis k is a record when count >= mRansacMinInliers and count > every earlier record's
__global__ __launch_bounds__(64) void k_pnp_records(const Desc* __restrict__ desc, int count, Hyp* __restrict__ hyp)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= count) return;
    const Desc& d = desc[c];
    int best = d.best0;
    for (int k = 0; k < d.iters; k++) {
        const int n = hyp[d.hypBase + k].n;
        if (n >= d.minInliers && n > best) { best = n; hyp[d.hypBase + k].rec = 1; }
    }
}

// ------------------------------------------------------------------ Refine
// one record per lane (the other lanes leave at once): compute_pose on the record's inliers, CheckInliers of the result
__global__ __launch_bounds__(kFitThreads) void k_pnp_refine(const Desc* __restrict__ desc, int count, int total, Hyp* __restrict__ hyp)
{
    extern __shared__ double sLane[];
    const int t = threadIdx.x, g = blockIdx.x * kFitThreads + t;
    if (g >= total) return;   // (no barrier below)
    Hyp& h = hyp[g];
    if (!h.rec) return;
    const Desc& d = desc[find_solver(desc, count, g)];
    MaskSrc src{d.pts, d.uv, d.n, 0, h.R, d.fu, d.fv, d.uc, d.vc, d.th2};
    while (src.firstIdx < d.n && !is_inlier(d.pts[src.firstIdx], d.uv[src.firstIdx], h.R, d.fu, d.fv, d.uc, d.vc, d.th2)) src.firstIdx++;
    if (src.firstIdx >= d.n) return;   // (cannot happen: a record counted at least mRansacMinInliers inliers)
    epnp<kFitThreads>(src, h.n, d.fu, d.fv, d.uc, d.vc, sLane + t, h.rR);
    int cnt = 0;
    for (int i = 0; i < d.n; i++) cnt += is_inlier(d.pts[i], d.uv[i], h.rR, d.fu, d.fv, d.uc, d.vc, d.th2) ? 1 : 0;
    h.rn = cnt;
    h.rok = cnt > d.minInliers ? 1 : 0;
}

// ------------------------------------------------------------------ the constructor from a resident frame
// P2D = mvKeysUn[idx].pt and sigma2 = mvLevelSigma2[kp.octave] where the frame's undistorted keys lie (pts[i].w and uv[i]
// are written; P3Dw came from the host).  An octave outside the table (no extractor of this library makes one) reads its
// last entry rather than past it.
__global__ __launch_bounds__(kPointThreads) void k_pnp_gather(const orbm::KeyDev* __restrict__ keys, const int32_t* __restrict__ idx, int n,
                                                              const float* __restrict__ levelSigma2, int nLevels, float4* __restrict__ pts,
                                                              float2* __restrict__ uv)
{
    const int i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= n) return;
    const orbm::KeyDev k = keys[idx[i]];
    pts[i].w = levelSigma2[min(max(k.octave, 0), nLevels - 1)];
    uv[i] = make_float2(k.x, k.y);
}

// ------------------------------------------------------------------ the mask iterate hands back
__global__ __launch_bounds__(kPointThreads) void k_pnp_mask(const float4* __restrict__ pts, const float2* __restrict__ uv, int n, const Pose pose, double fu,
                                                            double fv, double uc, double vc, float th2, uint8_t* __restrict__ out)
{
    const int p = blockIdx.x * kPointThreads + threadIdx.x;
    if (p >= n) return;
    out[p] = is_inlier(pts[p], uv[p], pose.v, fu, fv, uc, vc, th2) ? 1 : 0;
}

}  // namespace orbp
