// newpoints_ref.hpp -- a literal C++ restatement of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452 of both
// scenarios, monocular), of ComputeF12 (:536-553), of SearchForTriangulation's epipole (ORBmatcher.cc:666-672), of
// MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371) for a point with two observations, and of the OpenCV 3.0 pieces they
// call: gemm's small-matrix and transposed branches, the 3x3 invert, MatExpr scaling, addWeighted, norm and dot on CV_32F,
// and JacobiSVDImpl_<float> behind cv::SVD::compute.  It is the checker of the device CreateNewMapPoints
// (orbslamm_amd/csrc/orbl_kernels.hip): it includes no header of the library and is built with g++ -ffp-contract=off
// (every operation one IEEE op).  The OpenCV pieces it has in common with the other restatements are cv_ref.hpp's (which
// says how far they can be trusted); the 4x4 Jacobi SVD and the transposed gemm are here.
//
// The neighbour loop here is SERIAL, as the reference's: neighbour() handles one neighbour given the match list that
// SearchForTriangulation returned under the skip flags as they stand, and folds its successes into the flags before the
// caller searches the next neighbour.
//
// Defined choices, the same on the device:
//   - hypot inside the Jacobi rotation: lapack.cpp's written-out binary64 formula, not libm's
//   - UpdateNormalAndDepth's sum over the std::map runs in pointer order in the reference; here the current keyframe comes
//     first.  `normal + normali/norm` is taken as one MatOp_AddEx that assigns through cv::scaleAdd (float scale, float product,
//     float sum: from the published 3.0 source as remembered, unpinned like the rest); each term is then a float before the
//     sum, the first is added to zero, and the sum of two floats does not depend on the order
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "cv_ref.hpp"

namespace newpoints_ref {

struct KeyPt { float x, y, size, angle, response; int32_t octave, class_id; };   // cv::KeyPoint's layout
struct KeyFrame { float Rcw[9], tcw[3], Ow[3], K[4]; float medianDepth; };        // GetRotation, GetTranslation, GetCameraCenter, (fx, fy, cx, cy)
struct NewPoint { int32_t neighbour, idx1, idx2; float pos[3], normal[3], minDistance, maxDistance; };

enum Status : uint8_t { NEIGHBOUR_SKIPPED = 0, FEATURE_SKIPPED, NO_MATCH, PARALLAX, X3D_ZERO, Z1, Z2, REPROJ1, REPROJ2, DIST_ZERO, SCALE, ACCEPTED };

// ------------------------------------------------------------------------------------------------ OpenCV arithmetic
using cv_ref::gemmElem;   // gemm with flags == 0 and len == 3, one element
inline void mul33(const float* A, const float* B, float* D)
{
    float o[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[3 * i + j] = gemmElem(A + 3 * i, B + j, 3, 1.0, 0.f, 0.0);
    std::memcpy(D, o, sizeof o);
}
// A*B.t() (GEMM_2_T): the generic kernel, double sums in k order, d = (float)(s*alpha)
inline void mulT2(const float* A, const float* B, double alpha, float* D)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)A[3 * i + k] * (double)B[3 * j + k];
            D[3 * i + j] = (float)(s * alpha);
        }
}
using cv_ref::exprScale;
using cv_ref::scaleAdd;
using cv_ref::inv33;
inline double norm3(const float* v) { return cv_ref::norm(v, 3); }
inline double dot3(const float* a, const float* b) { return cv_ref::dot(a, b, 3); }
// JacobiSVDImpl_<float> on a 4x4: At (rows = columns of the source), Vt; the rotations and the sort (the random
// completion of a zero singular value touches only At, which CreateNewMapPoints does not read)
inline void jacobi4(float At[16], float Vt[16])
{
    const int n = 4;
    const float eps = FLT_EPSILON * 2;
    double W[4];
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < n; k++) { const float t = At[i * n + k]; sd += (double)t * t; }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                float *Ai = At + i * n, *Aj = At + j * n;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < n; k++) p += (double)Ai[k] * Aj[k];
                if (std::fabs(p) <= eps * std::sqrt((double)a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = cv_ref::hypotCv(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < n; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                float *Vi = Vt + i * n, *Vj = Vt + j * n;
                for (int k = 0; k < n; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < n; k++) { const float t = At[i * n + k]; sd += (double)t * t; }
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (int k = 0; k < n; k++) { float t = At[i * n + k]; At[i * n + k] = At[j * n + k]; At[j * n + k] = t; }
            for (int k = 0; k < n; k++) { float t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
}

// ------------------------------------------------------------------------------------------------ LocalMapping
// cv::Mat ComputeF12(pKF1, pKF2) and the epipole of SearchForTriangulation(pKF1, pKF2, ...)
inline void computeF12(const KeyFrame& k1, const KeyFrame& k2, float F12[9], float epipole[2])
{
    float R12[9], nR12[9], t12[3];
    mulT2(k1.Rcw, k2.Rcw, 1.0, R12);          // R1w*R2w.t()
    mulT2(k1.Rcw, k2.Rcw, -1.0, nR12);        // -R1w*R2w.t(): the scale rides in the gemm
    for (int i = 0; i < 3; i++) t12[i] = gemmElem(nR12 + 3 * i, k2.tcw, 1, 1.0, k1.tcw[i], 1.0);   // ...*t2w + t1w: gemm with C
    const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};      // SkewSymmetricMatrix
    const float K1t[9] = {k1.K[0], 0.f, 0.f, 0.f, k1.K[1], 0.f, k1.K[2], k1.K[3], 1.f};
    const float K2[9] = {k2.K[0], 0.f, k2.K[2], 0.f, k2.K[1], k2.K[3], 0.f, 0.f, 1.f};
    float iK1t[9], iK2[9], P[9], Q[9];
    inv33(K1t, iK1t);
    inv33(K2, iK2);
    mul33(iK1t, t12x, P);
    mul33(P, R12, Q);
    mul33(Q, iK2, F12);
    float C2[3];
    for (int i = 0; i < 3; i++) C2[i] = gemmElem(k2.Rcw + 3 * i, k1.Ow, 1, 1.0, k2.tcw[i], 1.0);   // R2w*Cw + t2w
    const float invz = 1.0f / C2[2];
    epipole[0] = k2.K[0] * C2[0] * invz + k2.K[2];
    epipole[1] = k2.K[1] * C2[1] * invz + k2.K[3];
}

// :244-260, monocular: true when the neighbour is skipped
inline bool baselineTooShort(const KeyFrame& k1, const KeyFrame& k2)
{
    float vBaseline[3];
    for (int i = 0; i < 3; i++) vBaseline[i] = k2.Ow[i] - k1.Ow[i];
    const float baseline = (float)norm3(vBaseline);
    const float ratioBaselineDepth = baseline / k2.medianDepth;
    return ratioBaselineDepth < 0.01;
}

inline float rowDotPlus(const float* R, int r, const float* X, float t) { return (float)(dot3(R + 3 * r, X) + t); }

// the body of the loop over vMatchedIndices (:286-450) for one pair, monocular; on ACCEPTED `out` holds the point and what
// UpdateNormalAndDepth leaves (neighbour, idx1, idx2 are the caller's).  dbg (optional, 9 floats, untouched where a gate
// returned earlier): cosParallaxRays, vt(3,3), z1, z2, the two squared reprojection errors, dist1, dist2, ratioDist -- the
// gates' float quantities, for the float64 check of the tests.
inline Status pair(const KeyFrame& k1, const KeyFrame& k2, const KeyPt& kp1, const KeyPt& kp2, const float* scaleFactors,
                   const float* levelSigma2, int nlevels, float ratioFactor, NewPoint& out, float* dbg = nullptr)
{
    float sink[9];
    if (!dbg) dbg = sink;
    const float fx1 = k1.K[0], fy1 = k1.K[1], cx1 = k1.K[2], cy1 = k1.K[3], invfx1 = 1.0f / fx1, invfy1 = 1.0f / fy1;
    const float fx2 = k2.K[0], fy2 = k2.K[1], cx2 = k2.K[2], cy2 = k2.K[3], invfx2 = 1.0f / fx2, invfy2 = 1.0f / fy2;
    const float xn1[3] = {(kp1.x - cx1) * invfx1, (kp1.y - cy1) * invfy1, 1.0f};
    const float xn2[3] = {(kp2.x - cx2) * invfx2, (kp2.y - cy2) * invfy2, 1.0f};
    float Rwc1[9], Rwc2[9], ray1[3], ray2[3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { Rwc1[3 * r + c] = k1.Rcw[3 * c + r]; Rwc2[3 * r + c] = k2.Rcw[3 * c + r]; }
    for (int r = 0; r < 3; r++) { ray1[r] = gemmElem(Rwc1 + 3 * r, xn1, 1, 1.0, 0.f, 0.0); ray2[r] = gemmElem(Rwc2 + 3 * r, xn2, 1, 1.0, 0.f, 0.0); }
    const float cosParallaxRays = dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2));
    const float cosParallaxStereo = cosParallaxRays + 1;
    dbg[0] = cosParallaxRays;
    if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < 0.9998)) return PARALLAX;
    // A.row(r) = xn(r)*Tcw.row(2) - Tcw.row(r): MatOp_AddEx(alpha = x, beta = -1) -> addWeighted_<float, double>; x == 1: subtract
    float Tcw1[12], Tcw2[12], A[16];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { Tcw1[4 * r + c] = k1.Rcw[3 * r + c]; Tcw2[4 * r + c] = k2.Rcw[3 * r + c]; }
        Tcw1[4 * r + 3] = k1.tcw[r]; Tcw2[4 * r + 3] = k2.tcw[r];
    }
    const float xs[4] = {xn1[0], xn1[1], xn2[0], xn2[1]};
    for (int r = 0; r < 4; r++) {
        const float* T = r < 2 ? Tcw1 : Tcw2;
        const int pr = r & 1;
        for (int c = 0; c < 4; c++)
            A[4 * r + c] = xs[r] == 1.f ? T[8 + c] - T[4 * pr + c] : (float)((double)T[8 + c] * (double)xs[r] + (double)T[4 * pr + c] * -1.0 + 0.0);
    }
    // cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV): temp_a = A.t(), vt from the rotations
    float At[16], Vt[16];
    for (int i = 0; i < 4; i++) for (int k = 0; k < 4; k++) At[4 * i + k] = A[4 * k + i];
    jacobi4(At, Vt);
    dbg[1] = Vt[15];
    if (Vt[15] == 0) return X3D_ZERO;
    float x3D[3];
    for (int c = 0; c < 3; c++) x3D[c] = exprScale(Vt[12 + c], 1. / (double)Vt[15]);   // x3D.rowRange(0,3)/x3D(3)
    const float z1 = rowDotPlus(k1.Rcw, 2, x3D, k1.tcw[2]);
    dbg[2] = z1;
    if (z1 <= 0) return Z1;
    const float z2 = rowDotPlus(k2.Rcw, 2, x3D, k2.tcw[2]);
    dbg[3] = z2;
    if (z2 <= 0) return Z2;
    const float sigmaSquare1 = levelSigma2[kp1.octave & 15];
    const float x1 = rowDotPlus(k1.Rcw, 0, x3D, k1.tcw[0]), y1 = rowDotPlus(k1.Rcw, 1, x3D, k1.tcw[1]);
    const float invz1 = 1.0 / z1;
    {
        const float u1 = fx1 * x1 * invz1 + cx1, v1 = fy1 * y1 * invz1 + cy1;
        const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y;
        dbg[4] = errX1 * errX1 + errY1 * errY1;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) return REPROJ1;
    }
    const float sigmaSquare2 = levelSigma2[kp2.octave & 15];
    const float x2 = rowDotPlus(k2.Rcw, 0, x3D, k2.tcw[0]), y2 = rowDotPlus(k2.Rcw, 1, x3D, k2.tcw[1]);
    const float invz2 = 1.0 / z2;
    {
        const float u2 = fx2 * x2 * invz2 + cx2, v2 = fy2 * y2 * invz2 + cy2;
        const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y;
        dbg[5] = errX2 * errX2 + errY2 * errY2;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) return REPROJ2;
    }
    float normal1[3], normal2[3];
    for (int c = 0; c < 3; c++) { normal1[c] = x3D[c] - k1.Ow[c]; normal2[c] = x3D[c] - k2.Ow[c]; }
    const double nrm1 = norm3(normal1), nrm2 = norm3(normal2);
    const float dist1 = nrm1, dist2 = nrm2;
    dbg[6] = dist1; dbg[7] = dist2;
    if (dist1 == 0 || dist2 == 0) return DIST_ZERO;
    const float ratioDist = dist2 / dist1;
    dbg[8] = ratioDist;
    const float ratioOctave = scaleFactors[kp1.octave & 15] / scaleFactors[kp2.octave & 15];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return SCALE;
    // new MapPoint(x3D, mpCurrentKeyFrame, mpMap); UpdateNormalAndDepth with the two observations
    for (int c = 0; c < 3; c++) {
        out.pos[c] = x3D[c];
        // normal = normal + normali/cv::norm(normali): MatOp_AddEx(alpha = 1/norm, beta = 1) -> cv::scaleAdd on CV_32F
        const float first = scaleAdd(normal1[c], 1. / nrm1, 0.f);
        const float sum = scaleAdd(normal2[c], 1. / nrm2, first);
        out.normal[c] = exprScale(sum, 1. / 2);                                                    // normal/n
    }
    out.maxDistance = dist1 * scaleFactors[kp1.octave & 15];
    out.minDistance = out.maxDistance / scaleFactors[(nlevels - 1) & 15];
    return ACCEPTED;
}

// One pass of the loop over vpNeighKFs (:237-451) for neighbour k.  m12 (n1 entries, -1: none) is what
// SearchForTriangulation returned under skip1 AS IT STANDS (null when the baseline gate skips the neighbour: the reference
// does not search then).  Successes are appended to out (walking vMatches12 in idx1 order, ORBmatcher.cc:817-822) and folded
// into skip1 (mpCurrentKeyFrame->AddMapPoint).  statusRow (n1) receives the code of every feature.  Returns the number of
// points appended.
inline int neighbour(int k, const KeyFrame& k1, const KeyFrame& k2, const KeyPt* keys1, int n1, const KeyPt* keys2, const int32_t* m12,
                     uint8_t* skip1, const float* scaleFactors, const float* levelSigma2, int nlevels, float scaleFactor, NewPoint* out,
                     uint8_t* statusRow)
{
    if (baselineTooShort(k1, k2)) {
        for (int q = 0; q < n1; q++) statusRow[q] = NEIGHBOUR_SKIPPED;
        return 0;
    }
    const float ratioFactor = 1.5f * scaleFactor;
    int nnew = 0;
    for (int q = 0; q < n1; q++) {
        if (skip1[q]) { statusRow[q] = FEATURE_SKIPPED; continue; }
        if (!m12 || m12[q] < 0) { statusRow[q] = NO_MATCH; continue; }
        NewPoint p;
        std::memset(&p, 0, sizeof p);
        const Status s = pair(k1, k2, keys1[q], keys2[m12[q]], scaleFactors, levelSigma2, nlevels, ratioFactor, p);
        statusRow[q] = s;
        if (s != ACCEPTED) continue;
        p.neighbour = k; p.idx1 = q; p.idx2 = m12[q];
        out[nnew++] = p;
    }
    // (the flags change after the walk: a feature appears once in vMatchedIndices, so the order inside a neighbour is moot)
    for (int i = 0; i < nnew; i++) skip1[out[i].idx1] = 1;
    return nnew;
}

}  // namespace newpoints_ref
