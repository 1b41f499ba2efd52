// sim3_ref.hpp -- a literal C++ restatement of Sim3Solver (src/Sim3Solver.cc, identical in both scenarios) and of the
// OpenCV 3.0 pieces it calls: cv::eigen on a symmetric 4x4 CV_32F (lapack.cpp's JacobiImpl_<float>), cv::Rodrigues vector
// to matrix (cvRodrigues2), cv::reduce SUM over columns, cv::pow(., 2), gemm's small-matrix and transposed branches,
// MatExpr scaling, norm and dot on CV_32F.  It is the checker of the device Sim3Solver (orbslamm_amd/csrc/
// orbs_kernels.hip): it shares no header with the library and is built with g++ -ffp-contract=off (every operation one
// IEEE operation).  The OpenCV pieces it has in common with the other restatements, and the set draw it has in common
// with pnp_ref, are cv_ref.hpp's (which says how far they can be trusted); cv::eigen, Rodrigues and reduce are here.
//
// Kept as the reference has them:
//   - mvnMaxError1/2 are vector<size_t>: the threshold is (size_t)(9.210 * (double)sigma2), compared as a float
//   - the set draw overwrites vAvailableIndices[idx] with idx the drawn VALUE (Sim3Solver.cc:175), so a set can repeat a
//     point; restated on a plain array of N with a live length (the reference's write past the live part lands inside
//     the vector's capacity and is never read back: the live length only shrinks)
//   - no special cases: three equal points or a quaternion of exactly (+-1, 0, 0, 0) give NaN through 0 * inf
//   - iterate's state (mnIterations, mnBestInliers and the best fields) persists across calls
// Defined choice: the double -> int conversion of SetRansacParameters' iteration count is x86's (cvttsd2si: NaN and
// out-of-range values give INT_MIN), which the reference leaves to the compiler.
#pragma once

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cv_ref.hpp"

namespace sim3_ref {

// ------------------------------------------------------------------------------------------------ OpenCV arithmetic
// gemm(A, B, alpha, C, beta) with flags == 0 and len == 3: cv_ref::gemmElem per element; C absent: c = 0, beta = 0.
// A is 3x3 row-major, B and C are 3 x cols row-major.
inline void gemm3(const float* A, const float* B, int cols, double alpha, const float* Cm, double beta, float* D)
{
    float o[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < cols; j++)
            o[i * cols + j] = cv_ref::gemmElem(A + i * 3, B + j, cols, alpha, Cm ? Cm[i * cols + j] : 0.f, Cm ? beta : 0.0);
    std::memcpy(D, o, sizeof(float) * 3 * cols);
}
// A*B.t() (GEMM_2_T takes the generic kernel, GEMMSingleMul<float, double>): double sums in k order, d = (float)(s*alpha)
inline void gemm3T2(const float* A, const float* B, float* D)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)A[i * 3 + k] * (double)B[j * 3 + k];
            D[i * 3 + j] = (float)(s * 1.0);
        }
}
using cv_ref::exprScale;
using cv_ref::norm;
using cv_ref::dot;

// cv::reduce(P, C, 1, CV_REDUCE_SUM) on a 3x3 CV_32F (reduceC_<float, float, OpAdd<float>>): per row a0 = p[0], a1 = p[1],
// the tail loop adds p[2] to a0, then a0 + a1
inline void reduceSumCols3(const float* P, float* C)
{
    for (int r = 0; r < 3; r++) {
        float a0 = P[r * 3 + 0];
        const float a1 = P[r * 3 + 1];
        a0 = a0 + P[r * 3 + 2];
        C[r] = a0 + a1;
    }
}

// cv::eigen(src, evals, evects) on an n x n symmetric CV_32F: JacobiImpl_<float> on a copy of src (only its upper
// triangle is read), eigenvalues descending, eigenvectors as ROWS of V
inline void eigenSym(const float* src, int n, float* W, float* V)
{
    const float eps = FLT_EPSILON;
    std::vector<float> Abuf(src, src + (size_t)n * n);
    float* A = Abuf.data();
    const int astep = n, vstep = n;
    int i, j, k, m;
    for (i = 0; i < n; i++) {
        for (j = 0; j < n; j++) V[i * vstep + j] = 0.f;
        V[i * vstep + i] = 1.f;
    }
    int iters;
    const int maxIters = n * n * 30;
    std::vector<int> indRv(n), indCv(n);
    int *indR = indRv.data(), *indC = indCv.data();
    float mv = 0.f;
    for (k = 0; k < n; k++) {
        W[k] = A[(astep + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = std::abs(A[astep * k + m]), i = k + 2; i < n; i++) {
                const float val = std::abs(A[astep * k + i]);
                if (mv < val) mv = val, m = i;
            }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = std::abs(A[k]), i = 1; i < k; i++) {
                const float val = std::abs(A[astep * i + k]);
                if (mv < val) mv = val, m = i;
            }
            indC[k] = m;
        }
    }
    if (n > 1) for (iters = 0; iters < maxIters; iters++) {
        // the pivot p = A(k, l)
        for (k = 0, mv = std::abs(A[indR[0]]), i = 1; i < n - 1; i++) {
            const float val = std::abs(A[astep * i + indR[i]]);
            if (mv < val) mv = val, k = i;
        }
        int l = indR[k];
        for (i = 1; i < n; i++) {
            const float val = std::abs(A[astep * indC[i] + i]);
            if (mv < val) mv = val, k = indC[i], l = i;
        }
        const float p = A[astep * k + l];
        if (std::abs(p) <= eps) break;
        const float y = (float)((W[l] - W[k]) * 0.5);
        float t = std::abs(y) + cv_ref::hypotCv(p, y);
        float s = cv_ref::hypotCv(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[astep * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        float a0, b0;
#define SIM3_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) SIM3_ROTATE(A[astep * i + k], A[astep * i + l]);
        for (i = k + 1; i < l; i++) SIM3_ROTATE(A[astep * k + i], A[astep * i + l]);
        for (i = l + 1; i < n; i++) SIM3_ROTATE(A[astep * k + i], A[astep * l + i]);
        for (i = 0; i < n; i++) SIM3_ROTATE(V[vstep * k + i], V[vstep * l + i]);
#undef SIM3_ROTATE
        for (j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = std::abs(A[astep * idx + m]), i = idx + 2; i < n; i++) {
                    const float val = std::abs(A[astep * idx + i]);
                    if (mv < val) mv = val, m = i;
                }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = std::abs(A[idx]), i = 1; i < idx; i++) {
                    const float val = std::abs(A[astep * i + idx]);
                    if (mv < val) mv = val, m = i;
                }
                indC[idx] = m;
            }
        }
    }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) {
            std::swap(W[m], W[k]);
            for (i = 0; i < n; i++) std::swap(V[vstep * m + i], V[vstep * k + i]);
        }
    }
}

// cv::Rodrigues(vec, R) for a 3-vector CV_32F and a 3x3 CV_32F R (cvRodrigues2's vector branch): binary64 from the float
// vector, theta < DBL_EPSILON gives the identity, the result rounded to float
inline void rodrigues(const float* v, float* Rout)
{
    double rx = v[0], ry = v[1], rz = v[2];
    const double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; k++) Rout[k] = (k % 4 == 0) ? 1.f : 0.f;
        return;
    }
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double c = std::cos(theta);
    const double s = std::sin(theta);
    const double c1 = 1. - c;
    const double itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) Rout[k] = (float)(c * I[k] + c1 * rrt[k] + s * r_x[k]);
}

// iterate's set draw (Sim3Solver.cc:163-177): `iterations` sets of 3
inline std::vector<int32_t> drawSets(int N, int iterations) { return cv_ref::drawSets(N, iterations, 3); }

// x86's double -> int (cvttsd2si)
inline int toInt(double v) { return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN; }

// ------------------------------------------------------------------------------------------------ Sim3Solver
// one hypothesis's fields (mT12i, mR12i, mt12i, ms12i, mnInliersi); the layout equals OrbsHypothesis of the C ABI
struct Hypothesis {
    int32_t nInliers = 0;
    float s12 = 0.f;
    float T12[16] = {0}, R12[9] = {0}, t12[3] = {0};
};
// iterate's outputs; the layout equals OrbsResult of the C ABI
struct Result {
    int32_t returned = 0;      // 1: a T12 was returned (else the empty cv::Mat)
    int32_t noMore = 0;        // bNoMore
    int32_t nInliers = 0;
    int32_t hypothesis = -1;   // the iteration that returned (0-based), -1: none
    int32_t iterations = 0;    // mnIterations after the call
    int32_t bestInliers = 0;   // mnBestInliers after the call
    int32_t hasBest = 0;       // 1: the best fields have been written (some hypothesis passed `>=`)
    float T12[16] = {0};       // the returned matrix (returned == 1)
    float bestR[9] = {0}, bestT[3] = {0}, bestS = 0.f;   // GetEstimatedRotation / Translation / Scale
};

class Sim3Solver {
public:
    // the constructor after its pointer chasing: idx1 = mvnIndices1 (N entries into [0, n1)), X1w / X2w the map points'
    // world positions, K = (fx, fy, cx, cy), sigma2_* = mvLevelSigma2[kp.octave]
    Sim3Solver(int n1, const int32_t* idx1, int n, const float* X1w, const float* X2w, const float* Rcw1, const float* tcw1,
               const float* Rcw2, const float* tcw2, const float K1[4], const float K2[4], const float* sigma2_1, const float* sigma2_2,
               bool fixScale)
        : mN1(n1), mnIterations(0), mnBestInliers(0), mbFixScale(fixScale)
    {
        for (int i = 0; i < n; i++) {
            mvnMaxError1.push_back(9.210 * sigma2_1[i]);   // (double product, then size_t: truncated)
            mvnMaxError2.push_back(9.210 * sigma2_2[i]);
            mvnIndices1.push_back((size_t)idx1[i]);
            float x[3];
            gemm3(Rcw1, X1w + 3 * i, 1, 1.0, tcw1, 1.0, x);
            mvX3Dc1.insert(mvX3Dc1.end(), x, x + 3);
            gemm3(Rcw2, X2w + 3 * i, 1, 1.0, tcw2, 1.0, x);
            mvX3Dc2.insert(mvX3Dc2.end(), x, x + 3);
        }
        for (int k = 0; k < 4; k++) { mK1[k] = K1[k]; mK2[k] = K2[k]; }
        FromCameraToImage(mvX3Dc1, mvP1im1, mK1);
        FromCameraToImage(mvX3Dc2, mvP2im2, mK2);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();
        mvbInliersi.resize(N);
        float epsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N)
            nIterations = 1;
        else
            nIterations = toInt(std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3.0))));
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
    }

    int maxIterations() const { return mRansacMaxIts; }
    int size() const { return N; }

    // iterate with the sets given (mRansacMaxIts x 3; set k belongs to iteration k).  inliers: mN1 bytes.  hyp (may be
    // null): every hypothesis evaluated is stored at its iteration.
    void iterate(int nIterations, const int32_t* sets, Result& res, uint8_t* vbInliers, Hypothesis* hyp)
    {
        res.returned = 0; res.noMore = 0; res.nInliers = 0; res.hypothesis = -1;
        for (int i = 0; i < mN1; i++) vbInliers[i] = 0;
        if (N < mRansacMinInliers) {
            res.noMore = 1;
            finish(res);
            return;
        }
        float P3Dc1i[9], P3Dc2i[9];
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            mnIterations++;
            const int32_t* set = sets + (size_t)(mnIterations - 1) * 3;
            for (short i = 0; i < 3; ++i) {
                const int idx = set[i];
                for (int r = 0; r < 3; r++) { P3Dc1i[r * 3 + i] = mvX3Dc1[(size_t)idx * 3 + r]; P3Dc2i[r * 3 + i] = mvX3Dc2[(size_t)idx * 3 + r]; }
            }
            ComputeSim3(P3Dc1i, P3Dc2i);
            CheckInliers();
            if (hyp) {
                Hypothesis& h = hyp[mnIterations - 1];
                h.nInliers = mnInliersi; h.s12 = ms12i;
                std::memcpy(h.T12, mT12i, sizeof mT12i); std::memcpy(h.R12, mR12i, sizeof mR12i); std::memcpy(h.t12, mt12i, sizeof mt12i);
            }
            if (mnInliersi >= mnBestInliers) {
                mvbBestInliers = mvbInliersi;
                mnBestInliers = mnInliersi;
                std::memcpy(mBestT12, mT12i, sizeof mT12i);
                std::memcpy(mBestRotation, mR12i, sizeof mR12i);
                std::memcpy(mBestTranslation, mt12i, sizeof mt12i);
                mBestScale = ms12i;
                mHasBest = true;
                if (mnInliersi > mRansacMinInliers) {
                    res.nInliers = mnInliersi;
                    for (int i = 0; i < N; i++)
                        if (mvbInliersi[i]) vbInliers[mvnIndices1[i]] = 1;
                    res.returned = 1;
                    res.hypothesis = mnIterations - 1;
                    std::memcpy(res.T12, mBestT12, sizeof mBestT12);
                    finish(res);
                    return;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) res.noMore = 1;
        finish(res);
    }

    void find(const int32_t* sets, Result& res, uint8_t* vbInliers, Hypothesis* hyp) { iterate(mRansacMaxIts, sets, res, vbInliers, hyp); }

    // thresholds as the comparison sees them
    float maxError1(int i) const { return (float)mvnMaxError1[i]; }
    float maxError2(int i) const { return (float)mvnMaxError2[i]; }

    static void FromCameraToImage(const std::vector<float>& vP3Dc, std::vector<float>& vP2D, const float K[4])
    {
        const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
        vP2D.clear();
        for (size_t i = 0, iend = vP3Dc.size() / 3; i < iend; i++) {
            const float invz = 1 / (vP3Dc[i * 3 + 2]);
            const float x = vP3Dc[i * 3 + 0] * invz;
            const float y = vP3Dc[i * 3 + 1] * invz;
            vP2D.push_back(fx * x + cx);
            vP2D.push_back(fy * y + cy);
        }
    }

    // ComputeSim3 on P1, P2 (3x3, one point per COLUMN); public for the tests
    void ComputeSim3(const float* P1, const float* P2)
    {
        float Pr1[9], Pr2[9], O1[3], O2[3];
        ComputeCentroid(P1, Pr1, O1);
        ComputeCentroid(P2, Pr2, O2);
        float M[9];
        gemm3T2(Pr2, Pr1, M);
#define SM(r, c) M[(r) * 3 + (c)]
        // the reference's doubles hold float expressions
        const double N11 = SM(0, 0) + SM(1, 1) + SM(2, 2);
        const double N12 = SM(1, 2) - SM(2, 1);
        const double N13 = SM(2, 0) - SM(0, 2);
        const double N14 = SM(0, 1) - SM(1, 0);
        const double N22 = SM(0, 0) - SM(1, 1) - SM(2, 2);
        const double N23 = SM(0, 1) + SM(1, 0);
        const double N24 = SM(2, 0) + SM(0, 2);
        const double N33 = -SM(0, 0) + SM(1, 1) - SM(2, 2);
        const double N34 = SM(1, 2) + SM(2, 1);
        const double N44 = -SM(0, 0) - SM(1, 1) + SM(2, 2);
#undef SM
        const float Nm[16] = {(float)N11, (float)N12, (float)N13, (float)N14, (float)N12, (float)N22, (float)N23, (float)N24,
                              (float)N13, (float)N23, (float)N33, (float)N34, (float)N14, (float)N24, (float)N34, (float)N44};
        float eval[4], evec[16];
        eigenSym(Nm, 4, eval, evec);
        for (int k = 0; k < 4; k++) mQuat[k] = evec[k];
        float vec[3] = {evec[1], evec[2], evec[3]};
        const double ang = std::atan2(norm(vec, 3), (double)evec[0]);
        // vec = 2*ang*vec/norm(vec): one MatExpr with alpha = (2*ang) * (1./norm)
        const double alpha = (2 * ang) * (1. / norm(vec, 3));
        for (int k = 0; k < 3; k++) vec[k] = exprScale(vec[k], alpha);
        rodrigues(vec, mR12i);
        float P3[9];
        gemm3(mR12i, Pr2, 3, 1.0, nullptr, 0.0, P3);
        if (!mbFixScale) {
            const double nom = dot(Pr1, P3, 9);
            float aux[9];
            for (int k = 0; k < 9; k++) aux[k] = P3[k] * P3[k];   // cv::pow(P3, 2, .): multiply(src, src)
            double den = 0;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) den += aux[i * 3 + j];
            ms12i = nom / den;
        } else
            ms12i = 1.0f;
        // mt12i = O1 - ms12i*mR12i*O2: one gemm(R, O2, -s, O1, 1)
        gemm3(mR12i, O2, 1, -(double)ms12i, O1, 1.0, mt12i);
        float sR[9];
        for (int k = 0; k < 9; k++) sR[k] = exprScale(mR12i[k], (double)ms12i);
        setT(mT12i, sR, mt12i);
        // sRinv = (1.0/ms12i)*mR12i.t(): transpose, then convertTo unless alpha is 1
        const double ainv = 1.0 / ms12i;
        float sRinv[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) sRinv[r * 3 + c] = ainv != 1.0 ? (float)((double)mR12i[c * 3 + r] * ainv) : mR12i[c * 3 + r];
        float tinv[3];
        gemm3(sRinv, mt12i, 1, -1.0, nullptr, 0.0, tinv);
        setT(mT21i, sRinv, tinv);
    }

    const float* T12i() const { return mT12i; }
    const float* T21i() const { return mT21i; }
    const float* R12i() const { return mR12i; }
    const float* t12i() const { return mt12i; }
    float s12i() const { return ms12i; }
    const float* quat() const { return mQuat; }

private:
    void finish(Result& res) const
    {
        res.iterations = mnIterations;
        res.bestInliers = mnBestInliers;
        res.hasBest = mHasBest ? 1 : 0;
        std::memcpy(res.bestR, mBestRotation, sizeof mBestRotation);
        std::memcpy(res.bestT, mBestTranslation, sizeof mBestTranslation);
        res.bestS = mBestScale;
    }
    static void setT(float* T, const float* R, const float* t)
    {
        for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.f : 0.f;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[r * 4 + c] = R[r * 3 + c]; T[r * 4 + 3] = t[r]; }
    }
    static void ComputeCentroid(const float* P, float* Pr, float* Cn)
    {
        reduceSumCols3(P, Cn);
        for (int r = 0; r < 3; r++) Cn[r] = exprScale(Cn[r], 1. / 3);   // C = C/P.cols
        for (int i = 0; i < 3; i++)
            for (int r = 0; r < 3; r++) Pr[r * 3 + i] = P[r * 3 + i] - Cn[r];
    }
    static void Project(const std::vector<float>& vP3Dw, std::vector<float>& vP2D, const float* Tcw, const float K[4])
    {
        const float Rcw[9] = {Tcw[0], Tcw[1], Tcw[2], Tcw[4], Tcw[5], Tcw[6], Tcw[8], Tcw[9], Tcw[10]};
        const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
        const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
        vP2D.clear();
        for (size_t i = 0, iend = vP3Dw.size() / 3; i < iend; i++) {
            float P3Dc[3];
            gemm3(Rcw, &vP3Dw[i * 3], 1, 1.0, tcw, 1.0, P3Dc);
            const float invz = 1 / (P3Dc[2]);
            const float x = P3Dc[0] * invz;
            const float y = P3Dc[1] * invz;
            vP2D.push_back(fx * x + cx);
            vP2D.push_back(fy * y + cy);
        }
    }
    void CheckInliers()
    {
        std::vector<float> vP1im2, vP2im1;
        Project(mvX3Dc2, vP2im1, mT12i, mK1);
        Project(mvX3Dc1, vP1im2, mT21i, mK2);
        mnInliersi = 0;
        for (size_t i = 0; i < mvP1im1.size() / 2; i++) {
            const float dist1[2] = {mvP1im1[i * 2] - vP2im1[i * 2], mvP1im1[i * 2 + 1] - vP2im1[i * 2 + 1]};
            const float dist2[2] = {vP1im2[i * 2] - mvP2im2[i * 2], vP1im2[i * 2 + 1] - mvP2im2[i * 2 + 1]};
            const float err1 = dot(dist1, dist1, 2);
            const float err2 = dot(dist2, dist2, 2);
            if (err1 < mvnMaxError1[i] && err2 < mvnMaxError2[i]) {   // float < size_t: the integer is converted to float
                mvbInliersi[i] = 1;
                mnInliersi++;
            } else
                mvbInliersi[i] = 0;
        }
    }

    std::vector<float> mvX3Dc1, mvX3Dc2;
    std::vector<size_t> mvnIndices1, mvnMaxError1, mvnMaxError2;
    int N = 0, mN1;
    float mR12i[9] = {0}, mt12i[3] = {0}, ms12i = 0.f, mT12i[16] = {0}, mT21i[16] = {0}, mQuat[4] = {0};
    std::vector<uint8_t> mvbInliersi;
    int mnInliersi = 0;
    int mnIterations;
    std::vector<uint8_t> mvbBestInliers;
    int mnBestInliers;
    float mBestT12[16] = {0}, mBestRotation[9] = {0}, mBestTranslation[3] = {0}, mBestScale = 0.f;
    bool mHasBest = false;
    bool mbFixScale;
    std::vector<float> mvP1im1, mvP2im2;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    float mK1[4], mK2[4];
};

}  // namespace sim3_ref
