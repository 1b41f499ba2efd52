// frustum_ref.hpp -- a literal C++ restatement of the projections that feed Tracking's two searches, monocular:
//   Frame::isInFrustum (src/Frame.cc:269-325) with the head of ORBmatcher::SearchByProjection(F, vpMapPoints, th)
//   (src/ORBmatcher.cc:45-69) and RadiusByViewingCos (:131-137), and
//   the projection loop of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) (:1353-1392),
// and of the OpenCV 3.0 pieces they call on CV_32F (gemm's small-matrix branch with a C, norm, dot, the matrix subtraction).
// It is the checker of the device k_view_project (orbslamm_amd/csrc/orbw_kernels.hip): plain C++11, no
// header of the library, built with g++ -ffp-contract=off (every operation one IEEE operation).  The OpenCV pieces are
// restated from the published 3.0 source and are UNPINNED.
//
// PredictScale is the DIRECT formula here, ceil(log(ratio)/logScaleFactor) in float (MapPoint.cc:385-394), not a break table.
// Defined choices (the same on the device):
//   - a level that is NaN or outside [0, nlevels) ends the point at LEVEL_RANGE (the reference reads mvScaleFactors out of
//     bounds there), reported as -1 (below, or NaN) or nlevels (above); no float is converted to int out of range
//   - a u or v that is NaN ends at OUT_OF_IMAGE (in the reference `u<mnMinX || u>mnMaxX` is false for a NaN and
//     GetFeaturesInArea converts it to int)
// What a point that is not IN_VIEW reports: u, v are 0 until the depth gate is passed, viewCos 0 until it is formed, r 0 unless
// IN_VIEW, lvl = (level - 1, level) with level -1 until PredictScale has run.  Frame/frame: lvl = (octave - 1, octave + 1) for
// every id >= 0, all zero for NO_POINT.
#pragma once

#include <cmath>
#include <cstdint>

namespace frustum_ref {

struct View { float Rcw[9], tcw[3], Ow[3], K[4]; float minX, maxX, minY, maxY; float viewingCosLimit; };   // OrbwView's layout
struct Point { float pos[3], normal[3], minDistance, maxDistance; uint8_t desc[32]; uint8_t flags, pad[3]; };   // OrbwPoint's layout
struct Query { float u, v, r, viewCos; int8_t lvl[2]; uint8_t valid, obs, status; };

enum Status : uint8_t { BAD = 0, DEPTH, OUT_OF_IMAGE, DISTANCE, VIEW_ANGLE, LEVEL_RANGE, IN_VIEW, NO_POINT };
enum { FLAG_BAD = 1, FLAG_OBSERVED = 2 };

// ORBmatcher.cc:131-137: the float against the double literal
inline float radiusByViewingCos(const float& viewCos)
{
    if (viewCos > 0.998)
        return 2.5;
    else
        return 4.0;
}

// mRcw*P+mtcw (Frame.cc:277, ORBmatcher.cc:1363): MatExpr folds it into one gemm(Rcw, P, 1, tcw, 1); matmul.cpp's branch
// for flags == 0, len == 3, d_size.width == 1: float products summed left to right, d = (float)(t*alpha + c*beta) in double
inline void gemmRt(const float* R, const float* t, const float* X, float* pc)
{
    for (int i = 0; i < 3; i++) {
        const float s = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2];
        pc[i] = (float)((double)s * 1.0 + (double)t[i] * 1.0);
    }
}

// Frame.cc:269-325 for one MapPoint, then ORBmatcher.cc:57-69
inline Query localPoint(const View& F, const Point& P, float th, const float* scaleFactors, int nlevels, float logScaleFactor)
{
    Query q;
    q.u = q.v = q.r = q.viewCos = 0.f; q.lvl[0] = -2; q.lvl[1] = -1; q.valid = 0;
    q.obs = (P.flags & FLAG_OBSERVED) ? 1 : 0;
    q.status = BAD;
    if (P.flags & FLAG_BAD) return q;   // Tracking.cc:1235, ORBmatcher.cc:57
    float Pc[3];
    gemmRt(F.Rcw, F.tcw, P.pos, Pc);
    const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
    q.status = DEPTH;
    if (PcZ < 0.0f) return q;   // :283
    const float invz = 1.0f / PcZ;   // :287
    const float u = F.K[0] * PcX * invz + F.K[2];   // :288
    const float v = F.K[1] * PcY * invz + F.K[3];   // :289
    q.u = u; q.v = v;
    q.status = OUT_OF_IMAGE;
    if (u != u || v != v) return q;   // defined choice
    if (u < F.minX || u > F.maxX) return q;   // :291
    if (v < F.minY || v > F.maxY) return q;   // :293
    const float maxDistance = 1.2f * P.maxDistance;   // MapPoint.cc:379-383
    const float minDistance = 0.8f * P.minDistance;   // MapPoint.cc:373-377
    float PO[3];
    for (int i = 0; i < 3; i++) PO[i] = P.pos[i] - F.Ow[i];   // :299, cv::subtract on CV_32F
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)PO[i] * (double)PO[i];   // cv::norm: normL2_<float, double>
    const float dist = (float)std::sqrt(s);   // :300
    q.status = DISTANCE;
    if (dist < minDistance || dist > maxDistance) return q;   // :302
    double dt = 0;
    for (int i = 0; i < 3; i++) dt += (double)PO[i] * (double)P.normal[i];   // Mat::dot: dotProd_<float>, a double sum
    const float viewCos = (float)(dt / dist);   // :308
    q.viewCos = viewCos;
    q.status = VIEW_ANGLE;
    if (viewCos < F.viewingCosLimit) return q;   // :310
    const float ratio = P.maxDistance / dist;   // MapPoint.cc:390
    const float lv = std::ceil(std::log(ratio) / logScaleFactor);   // MapPoint.cc:393
    q.status = LEVEL_RANGE;
    if (!(lv >= 0.f)) return q;
    if (!(lv < (float)nlevels)) { q.lvl[0] = (int8_t)(nlevels - 1); q.lvl[1] = (int8_t)nlevels; return q; }
    const int nPredictedLevel = (int)lv;
    q.lvl[0] = (int8_t)(nPredictedLevel - 1); q.lvl[1] = (int8_t)nPredictedLevel;   // ORBmatcher.cc:69
    const bool bFactor = th != 1.0;   // ORBmatcher.cc:49
    float r = radiusByViewingCos(viewCos);   // :63
    if (bFactor) r *= th;   // :65-66
    q.r = r * scaleFactors[nPredictedLevel];   // :69
    q.valid = 1;
    q.status = IN_VIEW;
    return q;
}

// ORBmatcher.cc:1353-1392 for one LastFrame feature that holds MapPoint P (null: no MapPoint, or mvbOutlier[i])
inline Query framePoint(const View& F, const Point* P, int nLastOctave, float th, const float* scaleFactors)
{
    Query q;
    q.u = q.v = q.r = q.viewCos = 0.f; q.lvl[0] = q.lvl[1] = 0; q.valid = 0; q.obs = 0;
    q.status = NO_POINT;
    if (!P) return q;   // :1357-1359
    q.obs = (P->flags & FLAG_OBSERVED) ? 1 : 0;
    q.lvl[0] = (int8_t)(nLastOctave - 1); q.lvl[1] = (int8_t)(nLastOctave + 1);   // :1392
    float x3Dc[3];
    gemmRt(F.Rcw, F.tcw, P->pos, x3Dc);   // :1363
    const float xc = x3Dc[0];
    const float yc = x3Dc[1];
    const float invzc = 1.0 / x3Dc[2];   // :1367: a double division
    q.status = DEPTH;
    if (invzc < 0) return q;   // :1369
    float u = F.K[0] * xc * invzc + F.K[2];   // :1372
    float v = F.K[1] * yc * invzc + F.K[3];   // :1373
    q.u = u; q.v = v;
    q.status = OUT_OF_IMAGE;
    if (u != u || v != v) return q;   // defined choice
    if (u < F.minX || u > F.maxX) return q;   // :1375
    if (v < F.minY || v > F.maxY) return q;   // :1377
    q.r = th * scaleFactors[nLastOctave];   // :1383
    q.valid = 1;
    q.status = IN_VIEW;
    return q;
}

}  // namespace frustum_ref
