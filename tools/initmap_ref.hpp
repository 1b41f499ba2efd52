// initmap_ref.hpp -- an independent restatement of Tracking::CreateInitialMapMonocular from its bundle adjustment on
// (src/Tracking.cc:728-758; `trk:LINE`), monocular: Optimizer::BundleAdjustment (src/Optimizer.cc:68-260; `ref:LINE`) over
// two keyframes and the points they share, ComputeSceneMedianDepth(2) (src/KeyFrame.cc:682-712; `kf:LINE`), the verdict and
// the rescaling.  For the tests and for tools/initmap_bench.py; on the host, in plain C++11 with the standard library alone.
// It shares no header with the library it checks.  The g2o pieces are restated here (`g2o:FILE:LINE` cites
// Thirdparty/g2o/g2o/FILE; Eigen is cited by function, as of Eigen 3.2.0: no Eigen is installed, so parity against g2o itself
// is UNPINNED, as DESIGN.md §2 says of OpenCV); SE3Quat, the Huber kernel, the defined sin / cos and the two arithmetic modes
// are poseopt_ref.hpp's, OpenCV's float arithmetic is cv_ref.hpp's.  Build with -ffp-contract=off.
//
// THE PROBLEM.  Two VertexSE3Expmap (pose 0: the initial keyframe, pose 1: the current one), each free or fixed (ref:100: the
// first is fixed when mnId == 0; both fixed is refused by the caller of this file).  One marginalised VertexSBAPointXYZ per
// matched feature of the initial frame in ascending feature index (ascending mnId: g2o's landmark order).  Two
// EdgeSE3ProjectXYZ per point; GetObservations() is walked in heap-address order (ref:126) and the DEFINED CHOICE is pose 0's
// edge first.  Vertex 0 of an edge is the point, vertex 1 the pose (ref:144-145).
//
// Two modes:
//   Serial   every sum over edges or points runs in g2o's order with one accumulator; libm's sin, cos and pow.
//   Defined  what the device is held to bit for bit.  THE SUMMATION TREE of §8o over POINTS: point k of the
//     problem goes to partial k % 64; each of the 64 partials starts at +0.0 and takes its points in ascending order (a
//     point's two edges in the defined order, pose 0's first); then six exchange steps m = 32, 16, 8, 4, 2, 1 replace every
//     partial l by p[l] + p[l ^ m] (all 64 at once), and partial 0 is the sum.  A sum that g2o starts from a value S that is
//     not zero (Hschur from Hpp + lambda, computeScale's landmark part from its pose part) is S + tree, its terms entering
//     the partials by + or - as g2o applies them.  The maximum of computeLambdaInit is taken the same way with
//     max(a, b) = (a < b) ? b : a for +: a partial takes max(|h|, partial) per diagonal entry, an exchange step gives
//     max(p[l], p[l ^ m]), and the result is max(tree, the poses' maximum).  The sums in question: the free poses' blocks of
//     Hpp (the 21 entries (i, j), i <= j, each), the poses' part of b, the Schur updates (21 + 36 + 21), `coefficients`,
//     computeScale's landmark part, the diagonal maximum, the robust chi2.
//     x^3 is x * x * x; sin / cos are definedSinCos; a NaN among the outputs leaves as x86's default NaN.
//
// THE REDUCED SOLVE.  g2o factors Hschur with Eigen's SimplicialLDLT behind an ordering (g2o:solvers/linear_solver_eigen.h:
// 60-110), reading the UPPER triangle (fillSparseMatrix(.., true)).  There is no Eigen to pin either, so: DEFINED CHOICE, an
// unpivoted LDLt in the poses' natural order over the entries (r, c), r <= c, of Hschur (which is why only the 21 upper entries
// of a diagonal block are summed), row by row, every dot product left to right (ldltPlain below).  It fails on a pivot that is
// zero or not finite.  On failure x -- poses AND points -- keeps what the last successful solve wrote, ZERO before any solve
// (the reading poseopt_ref.hpp documents), and the trial's chi2 becomes DBL_MAX.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cv_ref.hpp"
#include "poseopt_ref.hpp"

namespace initmap_ref {

using poseopt_ref::Arith;
using poseopt_ref::Cam;
using poseopt_ref::Defined;
using poseopt_ref::SE3;
using poseopt_ref::Serial;
using poseopt_ref::nanCanonical;

enum { kOk = 0, kResetDepth = 1, kResetTracked = 2, kResetNonfinite = 3 };
enum { kStopIterations = 0, kStopTrials = 1, kStopRhoZero = 2, kStopFlat = 3 };
enum { kStDone = 1 };   // UpdateNormalAndDepth ran (the statuses of refresh_ref.hpp; no other can occur here)

inline double maxOf(double a, double b) { return (a < b) ? b : a; }   // std::max(a, b)

// K sums over the points of a problem by the mode's rule (THE SUMMATION TREE above); start: what g2o's accumulator holds before
// the first term, or null for zero
template <class Mode, int K> struct PointSums {
    enum { P = Arith<Mode>::kPartials };
    double p[P][K], from[K];
    bool has;
    explicit PointSums(const double* start = 0) : has(start != 0)
    {
        for (int l = 0; l < P; l++) for (int k = 0; k < K; k++) p[l][k] = 0.0;
        for (int k = 0; k < K; k++) from[k] = start ? start[k] : 0.0;
        if (has && P == 1) for (int k = 0; k < K; k++) p[0][k] = start[k];
    }
    void add(int pt, int k, double v) { p[pt % P][k] = p[pt % P][k] + v; }
    void sub(int pt, int k, double v) { p[pt % P][k] = p[pt % P][k] - v; }
    void total(double* out)
    {
        for (int m = P / 2; m >= 1; m /= 2) {
            std::vector<double> q((size_t)P * K);
            for (int l = 0; l < P; l++) for (int k = 0; k < K; k++) q[(size_t)l * K + k] = p[l][k] + p[l ^ m][k];
            for (int l = 0; l < P; l++) for (int k = 0; k < K; k++) p[l][k] = q[(size_t)l * K + k];
        }
        for (int k = 0; k < K; k++) out[k] = (has && P > 1) ? from[k] + p[0][k] : p[0][k];
    }
};
template <class Mode> struct PointMax {
    enum { P = Arith<Mode>::kPartials };
    double p[P], from;
    explicit PointMax(double start) : from(start)
    {
        for (int l = 0; l < P; l++) p[l] = 0.0;
        if (P == 1) p[0] = start;
    }
    void take(int pt, double h) { p[pt % P] = maxOf(std::fabs(h), p[pt % P]); }
    double total()
    {
        for (int m = P / 2; m >= 1; m /= 2) {
            double q[P];
            for (int l = 0; l < P; l++) q[l] = maxOf(p[l], p[l ^ m]);
            for (int l = 0; l < P; l++) p[l] = q[l];
        }
        return P > 1 ? maxOf(p[0], from) : p[0];
    }
};

// the index of entry (i, j), i <= j, among the 21 of a 6 x 6 upper triangle, row by row
inline int upperIndex(int i, int j) { return i * (13 - i) / 2 + (j - i); }

// Eigen's 3 x 3 inverse (compute_inverse_size3_helper): the cofactors, the determinant from the first column, one reciprocal.
// M and out row-major
inline double cofactor3(const double* M, int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return M[i1 * 3 + j1] * M[i2 * 3 + j2] - M[i1 * 3 + j2] * M[i2 * 3 + j1];
}
inline void inverse3(const double* M, double* out)
{
    const double c0 = cofactor3(M, 0, 0), c1 = cofactor3(M, 1, 0), c2 = cofactor3(M, 2, 0);
    const double det = (c0 * M[0] + c1 * M[3]) + c2 * M[6];
    const double invdet = 1.0 / det;
    out[0] = c0 * invdet; out[1] = c1 * invdet; out[2] = c2 * invdet;
    for (int r = 1; r < 3; r++) for (int c = 0; c < 3; c++) out[r * 3 + c] = cofactor3(M, c, r) * invdet;
}

// THE REDUCED SOLVE (the header comment).  M: N x N row-major, its LOWER triangle holds the matrix (entry (r, c), c <= r, is
// Hschur's (c, r)) and is overwritten by L (unit diagonal implied) with D on the diagonal.  Row r: w[c] = M(r, c) - sum_{k < c}
// w[k] L(c, k) for c = 0 .. r - 1 in order (w[c] is L(r, c) D(c)), then L(r, c) = w[c] / D(c), then D(r) = M(r, r) - sum_{c < r}
// w[c] L(r, c).  Forward y(r) = b(r) - sum_{k < r} L(r, k) y(k), z(r) = y(r) / D(r), backward x(r) = z(r) - sum_{k > r} L(k, r) x(k),
// k ascending.  Every sum starts with its first product.  x is written only on success.
inline bool ldltPlain(int N, double* M, const double* b, double* x)
{
    double w[12], y[12];
    for (int r = 0; r < N; r++) {
        for (int c = 0; c < r; c++) {
            double t = M[r * N + c];
            if (c > 0) {
                double dot = w[0] * M[c * N];
                for (int k = 1; k < c; k++) dot = dot + w[k] * M[c * N + k];
                t = t - dot;
            }
            w[c] = t;
        }
        for (int c = 0; c < r; c++) M[r * N + c] = w[c] / M[c * N + c];
        double d = M[r * N + r];
        if (r > 0) {
            double dot = w[0] * M[r * N];
            for (int c = 1; c < r; c++) dot = dot + w[c] * M[r * N + c];
            d = d - dot;
        }
        if (!(d - d == 0.0) || d == 0.0) return false;
        M[r * N + r] = d;
    }
    for (int r = 0; r < N; r++) {
        double t = b[r];
        if (r > 0) {
            double dot = M[r * N] * y[0];
            for (int k = 1; k < r; k++) dot = dot + M[r * N + k] * y[k];
            t = t - dot;
        }
        y[r] = t;
    }
    for (int r = 0; r < N; r++) y[r] = y[r] / M[r * N + r];
    for (int r = N - 2; r >= 0; r--) {
        double dot = M[(r + 1) * N + r] * y[r + 1];
        for (int k = r + 2; k < N; k++) dot = dot + M[k * N + r] * y[k];
        y[r] = y[r] - dot;
    }
    for (int r = 0; r < N; r++) x[r] = y[r];
    return true;
}

// ------------------------------------------------------------------ the records (the layouts of the C entry's)
struct Key { float u, v; int32_t octave; };
struct Problem {
    float Tcw1[12], Tcw2[12];     // 3 x 4 row-major
    float K[4];                   // fx fy cx cy
    int32_t fixedFirst, fixedSecond, iterations, robust, n1, n2;
};
struct Result {
    float Tcw1[12], Tcw2[12], Ow1[3], Ow2[3], Tcw2Scaled[12];
    float medianDepth, invMedianDepth;
    int32_t nPoints, verdict, iterations, trials, stop, pad;
    double chi2First, chi2Last, lambda;
};
struct Point {
    float pos[3], posScaled[3], normal[3];
    float minDistance, maxDistance;
    uint8_t status, matched, pad[2];
};
struct Diag {
    int32_t rejectedTrials;     // trials that ended in pop()
    int32_t failedSolves;       // trials whose reduced solve failed
    double huberGap;            // min over linearisations and edges of |chi2 - delta^2| / delta^2 (DBL_MAX: none)
};

// ------------------------------------------------------------------ the edge (g2o:types/types_six_dof_expmap.cpp:103-138)
struct Obs { double uv[2], Om[4]; };

inline void computeError(const SE3& T, const Cam& K, const double* X, const Obs& o, double err[2])
{
    double p[3];
    poseopt_ref::se3Map(T, X, p);
    const double px = p[0] / p[2], py = p[1] / p[2];   // project2d
    err[0] = o.uv[0] - (px * K.fx + K.cx);
    err[1] = o.uv[1] - (py * K.fy + K.cy);
}

// A = _jacobianOplusXi (2 x 3, by the point), B = _jacobianOplusXj (2 x 6, by the pose), row-major
inline void linearizeOplus(const SE3& T, const Cam& K, const double* X, double A[6], double B[12])
{
    double p[3], R[9];
    poseopt_ref::se3Map(T, X, p);
    const double x = p[0], y = p[1], z = p[2], z_2 = z * z;
    const double tmp[6] = {K.fx, 0.0, -x / z * K.fx, 0.0, K.fy, -y / z * K.fy};
    poseopt_ref::quatToMatrix(T.q, R);
    const double c = -1. / z;
    double S[6];
    for (int k = 0; k < 6; k++) S[k] = c * tmp[k];            // -1./z * tmp, evaluated before the product with R
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) A[i * 3 + j] = (S[i * 3] * R[j] + S[i * 3 + 1] * R[3 + j]) + S[i * 3 + 2] * R[6 + j];
    B[0] = x * y / z_2 * K.fx;
    B[1] = -(1 + (x * x / z_2)) * K.fx;
    B[2] = y / z * K.fx;
    B[3] = -1. / z * K.fx;
    B[4] = 0;
    B[5] = x / z_2 * K.fx;
    B[6] = (1 + y * y / z_2) * K.fy;
    B[7] = -x * y / z_2 * K.fy;
    B[8] = -x / z * K.fy;
    B[9] = 0;
    B[10] = -1. / z * K.fy;
    B[11] = y / z_2 * K.fy;
}

// ------------------------------------------------------------------ the per-point pieces of the linear system
// BaseBinaryEdge::constructQuadraticForm (g2o:core/base_binary_edge.hpp:55-120) of one edge: `from` is the point (never fixed),
// `to` the pose.  Adds the edge's terms to the point's D (3 x 3 row-major) and b3; when the pose is free, ADDS to Bp (the pose's
// 6 x 3 block of Hpl, row-major) and writes the pose's own terms: Hterm (the 21 entries (i, j), i <= j, of B^T W B) and bterm.
// _hessianRowMajor is true for this edge (block_solver.hpp:240-244: the point is vertex 0), so Hpl's block takes B^T W A
// (robust) or B^T (A^T Omega)^T.  Returns the edge's chi2 (meaningful with `robust` only: it is what the kernel is given)
inline double edgeQuadraticForm(const SE3& T, const Cam& K, const double* X, const Obs& o, bool robust, double delta, double dsqr, bool poseFixed,
                                double* D, double* b3, double* Bp, double* Hterm, double* bterm)
{
    double err[2], A[6], B[12];
    computeError(T, K, X, o, err);
    linearizeOplus(T, K, X, A, B);
    // omega_r = - omega * _error: the unary minus binds to omega
    double r[2] = {(-o.Om[0]) * err[0] + (-o.Om[1]) * err[1], (-o.Om[2]) * err[0] + (-o.Om[3]) * err[1]};
    double W[4] = {o.Om[0], o.Om[1], o.Om[2], o.Om[3]};
    double c = 0.0;
    if (robust) {
        double rho[3];
        c = poseopt_ref::chi2Of(err, o.Om);
        poseopt_ref::huber(c, delta, dsqr, rho);
        for (int i = 0; i < 4; i++) W[i] = rho[1] * o.Om[i];   // robustInformation: rho[1] * Omega
        r[0] = r[0] * rho[1]; r[1] = r[1] * rho[1];           // omega_r *= rho[1]
    }
    // from->b() += A^T omega_r; from->A() += (A^T W) A
    double AtW[6];
    for (int i = 0; i < 3; i++) { AtW[i * 2] = A[i] * W[0] + A[3 + i] * W[2]; AtW[i * 2 + 1] = A[i] * W[1] + A[3 + i] * W[3]; }
    for (int i = 0; i < 3; i++) b3[i] = b3[i] + (A[i] * r[0] + A[3 + i] * r[1]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) D[i * 3 + j] = D[i * 3 + j] + (AtW[i * 2] * A[j] + AtW[i * 2 + 1] * A[3 + j]);
    if (poseFixed) return c;
    double BtW[12];
    for (int i = 0; i < 6; i++) { BtW[i * 2] = B[i] * W[0] + B[6 + i] * W[2]; BtW[i * 2 + 1] = B[i] * W[1] + B[6 + i] * W[3]; }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 3; j++) {
            if (robust) Bp[i * 3 + j] = Bp[i * 3 + j] + (BtW[i * 2] * A[j] + BtW[i * 2 + 1] * A[3 + j]);
            else Bp[i * 3 + j] = Bp[i * 3 + j] + (B[i] * AtW[j * 2] + B[6 + i] * AtW[j * 2 + 1]);
        }
    for (int i = 0; i < 6; i++) bterm[i] = B[i] * r[0] + B[6 + i] * r[1];                      // to->b() += B^T omega_r
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) Hterm[upperIndex(i, j)] = BtW[i * 2] * B[j] + BtW[i * 2 + 1] * B[6 + j];   // to->A() += (B^T W) B
    return c;
}

// one landmark of BlockSolver::solve's marginalisation (g2o:core/block_solver.hpp:385-436) behind setLambda (:586-591): Dinv of
// the damped block, db = Dinv * db, and per free pose BDinv = Bi * Dinv, the term of Bb += Bi * db (Cterm, pose * 6 + i) and the
// terms of Hschur(i1, i2) -= BDinv * Bj^T for i2 >= i1 (Sterm: [0, 21) block (0, 0) upper, [21, 57) block (0, 1) full row-major,
// [57, 78) block (1, 1) upper).  Bp: the point's two 6 x 3 blocks.  Entries of a fixed pose are left untouched
inline void pointSchur(const double* D, const double* b3, const double* Bp, const bool* fixed, double lambda, double* Dinv, double* Cterm, double* Sterm)
{
    double Dl[9], db[3];
    for (int i = 0; i < 9; i++) Dl[i] = D[i];
    for (int i = 0; i < 3; i++) Dl[i * 4] = Dl[i * 4] + lambda;
    inverse3(Dl, Dinv);
    for (int i = 0; i < 3; i++) db[i] = (Dinv[i * 3] * b3[0] + Dinv[i * 3 + 1] * b3[1]) + Dinv[i * 3 + 2] * b3[2];
    for (int s1 = 0; s1 < 2; s1++) {
        if (fixed[s1]) continue;
        const double* Bi = Bp + 18 * s1;
        double BDinv[18];
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 3; j++) BDinv[i * 3 + j] = (Bi[i * 3] * Dinv[j] + Bi[i * 3 + 1] * Dinv[3 + j]) + Bi[i * 3 + 2] * Dinv[6 + j];
        for (int i = 0; i < 6; i++) Cterm[6 * s1 + i] = (Bi[i * 3] * db[0] + Bi[i * 3 + 1] * db[1]) + Bi[i * 3 + 2] * db[2];
        for (int s2 = s1; s2 < 2; s2++) {
            if (fixed[s2]) continue;
            const double* Bj = Bp + 18 * s2;
            for (int i = 0; i < 6; i++)
                for (int j = (s1 == s2 ? i : 0); j < 6; j++)
                    Sterm[s1 != s2 ? 21 + i * 6 + j : (s1 ? 57 : 0) + upperIndex(i, j)] =
                        (BDinv[i * 3] * Bj[j * 3] + BDinv[i * 3 + 1] * Bj[j * 3 + 1]) + BDinv[i * 3 + 2] * Bj[j * 3 + 2];
        }
    }
}

// one landmark of the back-substitution (:463-486): cl = bl - Bt * xp (rightMultiply with cp = -xp, pose by pose), xl = Dinv * cl
// into zeroed memory.  xp: the free poses' steps in their order
inline void pointBackSubstitute(const double* b3, const double* Bp, const int* freeOf, int nFree, const double* xp, const double* Dinv, double* xl)
{
    double cl[3];
    for (int j = 0; j < 3; j++) cl[j] = b3[j];
    for (int a = 0; a < nFree; a++) {
        const double* Bi = Bp + 18 * freeOf[a];
        for (int j = 0; j < 3; j++) {
            double dot = Bi[j] * -xp[6 * a];
            for (int i = 1; i < 6; i++) dot = dot + Bi[i * 3 + j] * -xp[6 * a + i];
            cl[j] = cl[j] + dot;
        }
    }
    for (int j = 0; j < 3; j++) xl[j] = 0.0 + ((Dinv[j * 3] * cl[0] + Dinv[j * 3 + 1] * cl[1]) + Dinv[j * 3 + 2] * cl[2]);
}

// the reduced system from the summed Schur blocks S (pointSchur's layout) and bschur = bp - coeff, into the LOWER triangle of M
// (N x N, N = 6 nFree) as ldltPlain reads it
inline void assembleReduced(const double* S, const double* bp, const double* coeff, const int* freeOf, int nFree, double* M, double* bs)
{
    const int N = 6 * nFree;
    for (int i = 0; i < N * N; i++) M[i] = 0.0;
    for (int a = 0; a < nFree; a++) {
        const int s = freeOf[a];
        for (int i = 0; i < 6; i++) {
            bs[6 * a + i] = bp[6 * s + i] - coeff[6 * s + i];   // _bschur = _b - _coefficients
            for (int j = i; j < 6; j++) M[(6 * a + j) * N + (6 * a + i)] = S[(s ? 57 : 0) + upperIndex(i, j)];
        }
    }
    if (nFree == 2)
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) M[(6 + j) * N + i] = S[21 + i * 6 + j];
}

// ------------------------------------------------------------------ the optimizer
template <class Mode> struct BundleAdjuster {
    Cam K;
    int n;                          // points
    SE3 pose[2];
    bool fixed[2], robust;
    double delta, dsqr;
    std::vector<Obs> obs[2];        // the point's observation in keyframe 0 and 1
    std::vector<double> X;          // the points' estimates, 3 each
    // the linear system as buildSystem leaves it
    double Hpp[42], bp[12];         // the free poses' upper triangles (pose * 21 + upperIndex) and b (pose * 6 + i)
    std::vector<double> Hll, bl, Hpl;   // per point: 9 (row-major), 3, 2 x 18 (pose, then 6 x 3 row-major)
    std::vector<double> Dinv;           // per point, as the last solve() left it
    // what lives across trials and iterations
    double lambda, growth, xp[12];
    std::vector<double> xl;
    int flatSteps;
    Diag diag;

    // computeActiveErrors + activeRobustChi2 (g2o:core/sparse_optimizer.cpp:61-76, 100-114): activeEdges() is sorted by edge id,
    // the order of addEdge (ref:162): point by point, pose 0's edge first
    double activeRobustChi2()
    {
        PointSums<Mode, 1> sum;
        for (int k = 0; k < n; k++)
            for (int s = 0; s < 2; s++) {
                double err[2], rho[3];
                computeError(pose[s], K, &X[3 * (size_t)k], obs[s][(size_t)k], err);
                const double c = poseopt_ref::chi2Of(err, obs[s][(size_t)k].Om);
                if (robust) { poseopt_ref::huber(c, delta, dsqr, rho); sum.add(k, 0, rho[0]); }
                else sum.add(k, 0, c);
            }
        double out[1];
        sum.total(out);
        return out[0];
    }

    // buildSystem (g2o:core/block_solver.hpp:506-565): every active edge's quadratic form, point by point, pose 0's edge first
    void buildSystem()
    {
        PointSums<Mode, 42> sH;
        PointSums<Mode, 12> sb;
        for (int k = 0; k < n; k++) {
            double* D = &Hll[9 * (size_t)k];
            double* b3 = &bl[3 * (size_t)k];
            for (int i = 0; i < 9; i++) D[i] = 0.0;
            for (int i = 0; i < 3; i++) b3[i] = 0.0;
            for (int s = 0; s < 2; s++) {
                double* Bp = &Hpl[36 * (size_t)k + 18 * s];
                for (int i = 0; i < 18; i++) Bp[i] = 0.0;
                double Hterm[21], bterm[6];
                const double c = edgeQuadraticForm(pose[s], K, &X[3 * (size_t)k], obs[s][(size_t)k], robust, delta, dsqr, fixed[s], D, b3, Bp, Hterm, bterm);
                if (robust) {
                    const double gap = std::fabs(c - dsqr) / dsqr;
                    if (gap < diag.huberGap) diag.huberGap = gap;
                }
                if (fixed[s]) continue;
                for (int i = 0; i < 6; i++) sb.add(k, 6 * s + i, bterm[i]);
                for (int i = 0; i < 21; i++) sH.add(k, 21 * s + i, Hterm[i]);
            }
        }
        sH.total(Hpp);
        sb.total(bp);
    }

    // BlockSolver::solve (g2o:core/block_solver.hpp:358-490) behind setLambda (:568-593); true: x is written
    bool solveSystem()
    {
        // _Hschur->clear(); _Hpp->add(_Hschur): zero plus the damped block
        double start[78];
        for (int i = 0; i < 78; i++) start[i] = 0.0;
        for (int s = 0; s < 2; s++)
            for (int i = 0; i < 6; i++)
                for (int j = i; j < 6; j++) {
                    const double h = Hpp[21 * s + upperIndex(i, j)];
                    start[(s ? 57 : 0) + upperIndex(i, j)] = 0.0 + (i == j ? h + lambda : h);
                }
        PointSums<Mode, 78> sS(start);
        PointSums<Mode, 12> sC;
        for (int k = 0; k < n; k++) {
            double Cterm[12], Sterm[78];
            for (int i = 0; i < 12; i++) Cterm[i] = 0.0;
            for (int i = 0; i < 78; i++) Sterm[i] = 0.0;
            pointSchur(&Hll[9 * (size_t)k], &bl[3 * (size_t)k], &Hpl[36 * (size_t)k], fixed, lambda, &Dinv[9 * (size_t)k], Cterm, Sterm);
            for (int s1 = 0; s1 < 2; s1++) {
                if (fixed[s1]) continue;
                for (int i = 0; i < 6; i++) sC.add(k, 6 * s1 + i, Cterm[6 * s1 + i]);
                for (int i = 0; i < 21; i++) sS.sub(k, (s1 ? 57 : 0) + i, Sterm[(s1 ? 57 : 0) + i]);
                if (s1 == 0 && !fixed[1]) for (int i = 0; i < 36; i++) sS.sub(k, 21 + i, Sterm[21 + i]);
            }
        }
        double S[78], coeff[12];
        sS.total(S);
        sC.total(coeff);
        int freeOf[2], nFree = 0;
        for (int s = 0; s < 2; s++) if (!fixed[s]) freeOf[nFree++] = s;
        const int N = 6 * nFree;
        double M[144], bs[12], sol[12];
        for (int i = 0; i < 12; i++) { bs[i] = 0.0; sol[i] = 0.0; }
        assembleReduced(S, bp, coeff, freeOf, nFree, M, bs);
        if (!ldltPlain(N, M, bs, sol)) return false;
        for (int i = 0; i < N; i++) xp[i] = sol[i];
        for (int k = 0; k < n; k++)
            pointBackSubstitute(&bl[3 * (size_t)k], &Hpl[36 * (size_t)k], freeOf, nFree, xp, &Dinv[9 * (size_t)k], &xl[3 * (size_t)k]);
        return true;
    }

    // OptimizationAlgorithmLevenberg::solve (g2o:core/optimization_algorithm_levenberg.cpp:61-164); the stop reason, or -1: OK
    int solve(int iteration, int& trials, double& chiFirst, double& chiOut)
    {
        double chiNow = activeRobustChi2();
        double chiTrial = chiNow;
        const double chiStart = chiNow;
        if (iteration == 0) chiFirst = chiNow;
        buildSystem();
        int freeOf[2], nFree = 0;
        for (int s = 0; s < 2; s++) if (!fixed[s]) freeOf[nFree++] = s;
        if (iteration == 0) {
            // computeLambdaInit (:166-180) over indexMapping(): the free poses, then the points
            double poseMax = 0.;
            for (int a = 0; a < nFree; a++)
                for (int j = 0; j < 6; j++) poseMax = maxOf(std::fabs(Hpp[21 * freeOf[a] + upperIndex(j, j)]), poseMax);
            PointMax<Mode> mx(poseMax);
            for (int k = 0; k < n; k++) for (int j = 0; j < 3; j++) mx.take(k, Hll[9 * (size_t)k + 4 * j]);
            lambda = 1e-5 * mx.total();
            growth = 2;
            flatSteps = 0;
        }
        double gain = 0;
        int nTried = 0;
        do {
            const SE3 backup[2] = {pose[0], pose[1]};   // push() of every vertex
            const std::vector<double> Xbackup = X;
            const bool solved = solveSystem();
            if (!solved) diag.failedSolves++;
            // update(): oplus of every vertex with the solver's x, whatever solve() said
            for (int a = 0; a < nFree; a++) pose[freeOf[a]] = poseopt_ref::se3Mul(poseopt_ref::se3Exp<Mode>(&xp[6 * a]), pose[freeOf[a]]);
            for (size_t i = 0; i < X.size(); i++) X[i] = X[i] + xl[i];
            chiTrial = activeRobustChi2();
            if (!solved) chiTrial = DBL_MAX;
            gain = (chiNow - chiTrial);
            // computeScale (:182-189) over the whole x and b: the poses' dimensions, then the points'
            double poseScale = 0.;
            for (int a = 0; a < nFree; a++)
                for (int j = 0; j < 6; j++) poseScale += xp[6 * a + j] * (lambda * xp[6 * a + j] + bp[6 * freeOf[a] + j]);
            PointSums<Mode, 1> sc(&poseScale);
            for (int k = 0; k < n; k++)
                for (int j = 0; j < 3; j++) sc.add(k, 0, xl[3 * (size_t)k + j] * (lambda * xl[3 * (size_t)k + j] + bl[3 * (size_t)k + j]));
            double scale;
            sc.total(&scale);
            scale += 1e-3;
            gain /= scale;
            if (gain > 0 && (chiTrial >= -DBL_MAX && chiTrial <= DBL_MAX)) {
                const double t = 2 * gain - 1;
                double keep = 1. - Arith<Mode>::cube(t);
                keep = ((2. / 3.) < keep) ? (2. / 3.) : keep;
                const double shrink = ((1. / 3.) < keep) ? keep : (1. / 3.);
                lambda *= shrink;
                growth = 2;
                chiNow = chiTrial;
            } else {
                lambda *= growth;
                growth *= 2;
                pose[0] = backup[0]; pose[1] = backup[1];   // pop() of every vertex
                X = Xbackup;
                diag.rejectedTrials++;
            }
            nTried++;
        } while (gain < 0 && nTried < 10);
        trials += nTried;
        chiOut = chiNow;
        if (nTried == 10) return kStopTrials;
        if (gain == 0) return kStopRhoZero;
        if ((chiStart - chiNow) * 1e3 < chiStart) flatSteps++;
        else flatSteps = 0;
        if (flatSteps >= 3) return kStopFlat;
        return -1;
    }
};

inline void tcw16(const float* T12, float* T16)
{
    for (int i = 0; i < 12; i++) T16[i] = T12[i];
    T16[12] = 0.f; T16[13] = 0.f; T16[14] = 0.f; T16[15] = 1.f;
}

// KeyFrame::SetPose's centre (src/KeyFrame.cc:99-106): Rwc = Rcw.t(), Ow = -Rwc*tcw (gemm, alpha = -1), T 3 x 4 row-major
inline void cameraCentre(const float* T, float* Ow)
{
    const float tcw[3] = {T[3], T[7], T[11]};
    for (int i = 0; i < 3; i++) {
        const float row[3] = {T[i], T[4 + i], T[8 + i]};
        Ow[i] = cv_ref::gemmElem(row, tcw, 1, -1.0, 0.f, 0.0);
    }
}

// trk:728-758.  keys1 / keys2: mvKeysUn of the initial and the current frame; matches12: mvIniMatches (n1); P3D: mvIniP3D (3 n1).
// The caller has refused what the C entry refuses.  points: n1 records
template <class Mode>
inline void initialMap(const Problem& pr, const Key* keys1, const Key* keys2, const int32_t* matches12, const float* P3D, const float* invLevelSigma2,
                       const float* scaleFactors, int nlevels, Result& res, Point* points, Diag* diagOut)
{
    std::memset(&res, 0, sizeof res);
    std::memset(points, 0, sizeof(Point) * (size_t)pr.n1);
    BundleAdjuster<Mode> o;
    o.K.fx = (double)pr.K[0]; o.K.fy = (double)pr.K[1]; o.K.cx = (double)pr.K[2]; o.K.cy = (double)pr.K[3];
    float T16[16];
    tcw16(pr.Tcw1, T16); o.pose[0] = poseopt_ref::toSE3Quat(T16);   // ref:98
    tcw16(pr.Tcw2, T16); o.pose[1] = poseopt_ref::toSE3Quat(T16);
    o.fixed[0] = pr.fixedFirst != 0; o.fixed[1] = pr.fixedSecond != 0;
    o.robust = pr.robust != 0;
    const float thHuber2D = std::sqrt(5.99);   // ref:106: a float
    o.delta = (double)thHuber2D;
    o.dsqr = o.delta * o.delta;
    std::vector<int32_t> feat;
    for (int i = 0; i < pr.n1; i++) if (matches12[i] >= 0) feat.push_back(i);   // trk:694-697
    const int n = (int)feat.size();
    o.n = n;
    o.obs[0].resize((size_t)n); o.obs[1].resize((size_t)n);
    o.X.resize(3 * (size_t)n);
    for (int k = 0; k < n; k++) {
        const Key* kp[2] = {&keys1[feat[(size_t)k]], &keys2[matches12[feat[(size_t)k]]]};
        for (int s = 0; s < 2; s++) {
            Obs& ob = o.obs[s][(size_t)k];
            ob.uv[0] = (double)kp[s]->u; ob.uv[1] = (double)kp[s]->v;
            const double w = (double)invLevelSigma2[kp[s]->octave];   // Matrix2d::Identity() * invSigma2 (ref:148): the zeros multiply
            ob.Om[0] = 1.0 * w; ob.Om[1] = 0.0 * w; ob.Om[2] = 0.0 * w; ob.Om[3] = 1.0 * w;
        }
        for (int c = 0; c < 3; c++) o.X[3 * (size_t)k + c] = (double)P3D[3 * (size_t)feat[(size_t)k] + c];   // toVector3d (ref:116)
    }
    o.Hll.assign(9 * (size_t)n, 0.0); o.bl.assign(3 * (size_t)n, 0.0); o.Hpl.assign(36 * (size_t)n, 0.0); o.Dinv.assign(9 * (size_t)n, 0.0);
    o.xl.assign(3 * (size_t)n, 0.0);
    for (int i = 0; i < 12; i++) o.xp[i] = 0.0;
    for (int i = 0; i < 42; i++) o.Hpp[i] = 0.0;
    for (int i = 0; i < 12; i++) o.bp[i] = 0.0;
    o.lambda = 0.; o.growth = 2.; o.flatSteps = 0;
    o.diag.rejectedTrials = 0; o.diag.failedSolves = 0; o.diag.huberGap = DBL_MAX;
    // optimize(nIterations) (g2o:core/sparse_optimizer.cpp:352-420).  With no point there is no edge, initializeOptimization()
    // finds no vertex and optimize() returns at once
    res.stop = kStopIterations;
    if (n > 0)
        for (int i = 0; i < pr.iterations; i++) {
            res.iterations++;
            const int stop = o.solve(i, res.trials, res.chi2First, res.chi2Last);
            if (stop >= 0) { res.stop = stop; break; }
        }
    res.lambda = o.lambda;
    res.nPoints = n;
    // ---- recovery (ref:214-258): the poses first
    poseopt_ref::toCvMat(o.pose[0], T16); for (int i = 0; i < 12; i++) res.Tcw1[i] = T16[i];
    poseopt_ref::toCvMat(o.pose[1], T16); for (int i = 0; i < 12; i++) res.Tcw2[i] = T16[i];
    cameraCentre(res.Tcw1, res.Ow1);
    cameraCentre(res.Tcw2, res.Ow2);
    // ---- then every point: SetWorldPos narrowed, UpdateNormalAndDepth (src/MapPoint.cc:330-371) over the observations in
    // the defined order with the NEW centres; pRefKF is the current keyframe (trk:702), the level its feature's octave
    std::vector<float> depths;
    bool finite = true;
    for (int k = 0; k < n; k++) {
        Point& pt = points[feat[(size_t)k]];
        pt.matched = 1;
        for (int c = 0; c < 3; c++) pt.pos[c] = (float)o.X[3 * (size_t)k + c];
        float normal[3] = {0.f, 0.f, 0.f};
        const float* Ow[2] = {res.Ow1, res.Ow2};
        for (int s = 0; s < 2; s++) {
            float normali[3];
            for (int c = 0; c < 3; c++) normali[c] = pt.pos[c] - Ow[s][c];
            const float a = (float)(1. / cv_ref::norm(normali, 3));
            for (int c = 0; c < 3; c++) { const float t = normali[c] * a; normal[c] = t + normal[c]; }
        }
        float PC[3];
        for (int c = 0; c < 3; c++) PC[c] = pt.pos[c] - res.Ow2[c];
        const float dist = (float)cv_ref::norm(PC, 3);
        const int level = keys2[matches12[feat[(size_t)k]]].octave;
        pt.maxDistance = dist * scaleFactors[level];
        pt.minDistance = pt.maxDistance / scaleFactors[nlevels - 1];
        for (int c = 0; c < 3; c++) pt.normal[c] = cv_ref::exprScale(normal[c], 1. / 2);
        pt.status = kStDone;
        // kf:695-705 with the adjusted pose of the initial keyframe: float z = Rcw2.dot(x3Dw) + zcw -- the dot is a double, zcw
        // widens, the sum narrows
        const float z = (float)(cv_ref::dot(res.Tcw1 + 8, pt.pos, 3) + (double)res.Tcw1[11]);
        if (!(z - z == 0.f)) finite = false;
        depths.push_back(z);
    }
    // ---- trk:731-734
    if (!finite) {
        res.verdict = kResetNonfinite;
        res.medianDepth = nanCanonical(std::nanf(""));
        res.invMedianDepth = res.medianDepth;
    } else {
        if (n > 0) {
            std::sort(depths.begin(), depths.end());
            res.medianDepth = depths[(depths.size() - 1) / 2] + 0.f;   // (a zero leaves as +0: sort does not order -0 and +0)
        } else res.medianDepth = 0.f;   // DEFINED: the reference indexes an empty vector
        res.invMedianDepth = 1.0f / res.medianDepth;
        res.verdict = res.medianDepth < 0 ? kResetDepth : n < 90 ? kResetTracked : kOk;
    }
    // ---- trk:745-757: cv::Mat * float is a MatExpr with alpha = the float widened
    const bool rescale = res.verdict == kOk;
    for (int i = 0; i < 12; i++) res.Tcw2Scaled[i] = (rescale && i % 4 == 3) ? cv_ref::exprScale(res.Tcw2[i], (double)res.invMedianDepth) : res.Tcw2[i];
    for (int k = 0; k < n; k++) {
        Point& pt = points[feat[(size_t)k]];
        for (int c = 0; c < 3; c++) pt.posScaled[c] = rescale ? cv_ref::exprScale(pt.pos[c], (double)res.invMedianDepth) : pt.pos[c];
    }
    // ---- a NaN leaves in one pattern
    float* rf = reinterpret_cast<float*>(&res);
    for (int i = 0; i < 44; i++) rf[i] = nanCanonical(rf[i]);   // Tcw1 .. invMedianDepth: 44 floats in a row
    res.chi2First = nanCanonical(res.chi2First); res.chi2Last = nanCanonical(res.chi2Last); res.lambda = nanCanonical(res.lambda);
    for (int k = 0; k < n; k++) {
        float* pf = reinterpret_cast<float*>(&points[feat[(size_t)k]]);
        for (int i = 0; i < 11; i++) pf[i] = nanCanonical(pf[i]);
    }
    if (diagOut) *diagOut = o.diag;
}

}  // namespace initmap_ref
