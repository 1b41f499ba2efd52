// orbslamm_dropin.hpp -- what the solver drop-ins (Initializer_hip.hpp, Sim3Solver_hip.hpp, PnPsolver_hip.hpp,
// LocalMapping_hip.hpp, LoopClosing_hip.hpp) share; below the solvers' part, what the keyframe drop-ins share: a keyframe
// flattened for the C ABI and the pieces of the two batched Fuse calls (CreateNewMapPointsT, SearchInNeighborsT,
// SearchAndFuseT).  Header-only, C++11; installed next to them and included by relative name.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_hip.h"

namespace iORB_SLAM {
namespace detail {

const int kCV_32F = 5;

// an error of the C ABI as the drop-ins throw it: who ("Sim3Solver(HIP): ") and the library's text
inline void check(int rc, const char* who)
{
    if (rc != ORBX_OK) throw std::runtime_error(std::string(who) + orbx_last_error());
}

// `count` more RANSAC sets of k behind `sets`, drawn as the Sim3Solver's and the PnPsolver's iterate draw them
// (Sim3Solver.cc:163-177, PnPsolver.cc:191-201): Random::RandomInt over the process's rand(), one call per index;
// vAvailableIndices[idx] is indexed by the drawn VALUE as in the reference (its write can land past the live part: here
// the vector keeps its N slots)
template <class Random>
void draw_sets(int N, int k, int count, std::vector<int32_t>& sets)
{
    std::vector<size_t> vAvailableIndices((size_t)N);
    size_t at = sets.size();
    sets.resize(at + (size_t)count * k, 0);
    for (int it = 0; it < count; it++) {
        for (int i = 0; i < N; i++) vAvailableIndices[i] = (size_t)i;
        int live = N;
        for (short i = 0; i < k; ++i) {
            const int randi = Random::RandomInt(0, live - 1);
            const int idx = (int)vAvailableIndices[randi];
            sets[at++] = idx;
            vAvailableIndices[idx] = vAvailableIndices[live - 1];
            live--;
        }
    }
}

// the first n flags of a mask as the reference's vector<bool>
inline std::vector<bool> mask_bools(const std::vector<uint8_t>& mask, int n)
{
    std::vector<bool> out((size_t)n, false);
    for (int i = 0; i < n; i++) if (mask[i]) out[i] = true;
    return out;
}

// a row-major float array as Mat(rows, cols, CV_32F)
template <class Mat>
Mat mat32f(const float* a, int rows, int cols)
{
    Mat m(rows, cols, kCV_32F);
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) m.template at<float>(r, c) = a[cols * r + c];
    return m;
}

// ------------------------------------------------------------------ keyframes and map points as the C ABI takes them
// mvKeysUn and the descriptors of a keyframe
struct FlatFeatures { std::vector<OrbxKeyPoint> keys; std::vector<uint8_t> desc; };

template <class KeyFrame>
void flatten_features(KeyFrame* pKF, FlatFeatures& f)
{
    f.keys.resize((size_t)pKF->N); f.desc.resize((size_t)pKF->N * 32);
    for (int i = 0; i < pKF->N; i++) {
        const auto& kp = pKF->mvKeysUn[i];
        OrbxKeyPoint& o = f.keys[i];
        o.x = kp.pt.x; o.y = kp.pt.y; o.size = kp.size; o.angle = kp.angle; o.response = kp.response; o.octave = kp.octave; o.class_id = kp.class_id;
        const unsigned char* d = pKF->mDescriptors.template ptr<unsigned char>(i);
        for (int b = 0; b < 32; b++) f.desc[(size_t)i * 32 + b] = d[b];
    }
}

// GetRotation, GetTranslation, GetCameraCenter as row-major floats
template <class KeyFrame>
void keyframe_pose(KeyFrame* pKF, float Rcw[9], float tcw[3], float Ow[3])
{
    const auto R = pKF->GetRotation();
    const auto t = pKF->GetTranslation();
    const auto O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rcw[3 * r + c] = R.template at<float>(r, c);
        tcw[r] = t.template at<float>(r, 0);
        Ow[r] = O.template at<float>(r, 0);
    }
}

// a Fuse target: the keyframe's intrinsics, image bounds and grid under the pose the caller names (its own, or a corrected one)
template <class KeyFrame>
void fuse_target(KeyFrame* k, const float Rcw[9], const float tcw[3], const float Ow[3], OrblFuseTarget& r)
{
    for (int i = 0; i < 9; i++) r.Rcw[i] = Rcw[i];
    for (int i = 0; i < 3; i++) { r.tcw[i] = tcw[i]; r.Ow[i] = Ow[i]; }
    r.K[0] = k->fx; r.K[1] = k->fy; r.K[2] = k->cx; r.K[3] = k->cy;
    r.min_x = (float)k->mnMinX; r.max_x = (float)k->mnMaxX; r.min_y = (float)k->mnMinY; r.max_y = (float)k->mnMaxY;
    r.grid.minX = (float)k->mnMinX; r.grid.minY = (float)k->mnMinY;
    r.grid.invW = k->mfGridElementWidthInv; r.grid.invH = k->mfGridElementHeightInv;
    r.grid.cols = k->mnGridCols; r.grid.rows = k->mnGridRows;
}

// a map point of a Fuse pool: GetWorldPos, GetNormal, the RAW mfMinDistance / mfMaxDistance, GetDescriptor
template <class Mat, class MapPoint>
OrblFusePoint fuse_point(MapPoint* pMP)
{
    OrblFusePoint p;
    const Mat X = pMP->GetWorldPos(), n = pMP->GetNormal(), d = pMP->GetDescriptor();
    for (int r = 0; r < 3; r++) { p.pos[r] = X.template at<float>(r, 0); p.normal[r] = n.template at<float>(r, 0); }
    p.min_distance = pMP->mfMinDistance; p.max_distance = pMP->mfMaxDistance;
    const unsigned char* b = d.template ptr<unsigned char>(0);
    for (int i = 0; i < 32; i++) p.desc[i] = b[i];
    return p;
}

// The window search of ONE (keyframe, point) pair on the host, with the descriptor the point holds NOW, through the
// reference's own pKF->GetFeaturesInArea: ORBmatcher.cc:894-951 (Chi2: with the 5.99 test) or :1053-1081 (without).
// bestIdx = -1, bestDist = 256 when the window holds no candidate
template <bool Chi2, class Mat, class KeyFrame, class MapPoint>
void fuse_rescore(KeyFrame* pKF, MapPoint* pMP, float u, float v, int nPredictedLevel, float th, int& bestDist, int& bestIdx)
{
    const float radius = th * pKF->mvScaleFactors[nPredictedLevel];
    const std::vector<size_t> vIndices = pKF->GetFeaturesInArea(u, v, radius);
    const Mat dMP = pMP->GetDescriptor();
    const unsigned char* a = dMP.template ptr<unsigned char>(0);
    bestDist = 256; bestIdx = -1;
    for (size_t k = 0; k < vIndices.size(); k++) {
        const size_t idx = vIndices[k];
        const auto& kp = pKF->mvKeysUn[idx];
        const int kpLevel = kp.octave;
        if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
        if (Chi2) {
            const float ex = u - kp.pt.x, ey = v - kp.pt.y;
            const float e2 = ex * ex + ey * ey;
            if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 5.99) continue;
        }
        const unsigned char* b = pKF->mDescriptors.template ptr<unsigned char>((int)idx);
        int dist = 0;
        for (int w = 0; w < 32; w++) dist += __builtin_popcount((unsigned)(a[w] ^ b[w]));
        if (dist < bestDist) { bestDist = dist; bestIdx = (int)idx; }
    }
}

}  // namespace detail
}  // namespace iORB_SLAM
