// Test infrastructure for ComputeSim3T (include/LoopClosing_hip.hpp): two mock keyframes (tests/cpp/mock_slam.hpp) of two maps that
// see one synthetic scene under a known similarity, each feature holding a MapPoint of its own map with a pool id, and the mock
// g2o::Sim3 of tests/cpp/mock_sim3opt.hpp.  Plain data holders and a scene generator: nothing here computes what the product computes.
#pragma once

#include <cmath>
#include <memory>
#include <vector>

#include "dropin_test.hpp"
#include "mock_sim3opt.hpp"

namespace cmock {

const int W = 640, H = 480, NLEVELS = 8;
const float SCALE = 1.2f;

struct MapPoint : mock::MapPoint { int poolId = -1; };

struct Pair {
    mock::KeyFrame K1, K2;
    std::vector<std::unique_ptr<MapPoint> > pts;
    std::vector<int> true2;          // pKF2's feature of pKF1's feature i
    float R12[9], t12[3], s12;       // the Sim3 a solver would hand over: the truth a little off
};

inline void initKeyFrame(mock::KeyFrame& K, int n, const double R[9], const double t[3])
{
    K.N = n;
    K.mvKeysUn.resize((size_t)n);
    K.mvuRight.assign((size_t)n, -1.f);
    K.mvpMapPoints.assign((size_t)n, nullptr);
    K.mDescriptors = mock::Mat::u8(n, 32);
    K.fx = 517.3f; K.fy = 516.5f; K.cx = 318.6f; K.cy = 255.3f;
    float sf = 1.f;
    for (int l = 0; l < NLEVELS; l++) { K.mvScaleFactors.push_back(sf); K.mvLevelSigma2.push_back(sf * sf); K.mvInvLevelSigma2.push_back(1.f / (sf * sf)); sf *= SCALE; }
    K.mfLogScaleFactor = std::log(SCALE);
    K.mnMinX = 0; K.mnMinY = 0; K.mnMaxX = W; K.mnMaxY = H;
    K.mfGridElementWidthInv = 64.f / W; K.mfGridElementHeightInv = 48.f / H;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) K.Tcw.at<float>(r, c) = (float)R[3 * r + c];
        K.Tcw.at<float>(r, 3) = (float)t[r];
    }
    K.Tcw.at<float>(3, 3) = 1.f;
}

// n features a keyframe on a jittered lattice; `holds` of pKF1's features (the first ones) hold a point, every feature of pKF2 does;
// pool ids from id0 on: pKF1's point of feature i at id0 + i, pKF2's point of feature j at id0 + n + j
inline void makePair(Pair& S, unsigned seed, int n, int holds, int id0)
{
    unsigned s = seed;
    double R1[9], R2[9], Rt[9], Rs[9];
    const double t1[3] = {0.3, -0.1, 0.4}, t2[3] = {-0.2, 0.15, 0.1}, tt[3] = {0.05, -0.03, 0.02}, st = 1.04;
    eulerR(0.05 + 0.1 * urand(s), -0.2, 0.03, R1);
    eulerR(-0.1, 0.15 + 0.1 * urand(s), 0.2, R2);
    eulerR(0.02, -0.03, 0.015, Rt);   // the truth: P1c = st Rt P2c + tt
    eulerR(0.022, -0.028, 0.016, Rs);
    initKeyFrame(S.K1, n, R1, t1);
    initKeyFrame(S.K2, n, R2, t2);
    for (int k = 0; k < 9; k++) S.R12[k] = (float)Rs[k];
    for (int k = 0; k < 3; k++) S.t12[k] = (float)(tt[k] + 0.004 * (k - 1));
    S.s12 = (float)(st * 1.004);
    S.true2.assign((size_t)n, -1);
    S.pts.clear();
    const int cols = 24;
    for (int i = 0; i < n; i++) {
        const int j = (int)(((long)i * 7 + 3) % n);   // (n is not a multiple of 7: a permutation)
        S.true2[(size_t)i] = j;
        const int oct = (int)(urand(s) * 4) % 4;
        const double u = 30 + 25.0 * (i % cols) + 4 * (urand(s) - 0.5), v = 30 + 30.0 * (i / cols) + 4 * (urand(s) - 0.5);
        const double z = 2 + 10 * urand(s), P1[3] = {(u - 318.6) / 517.3 * z, (v - 255.3) / 516.5 * z, z};
        double P2[3];
        for (int r = 0; r < 3; r++) { P2[r] = 0; for (int c = 0; c < 3; c++) P2[r] += Rt[3 * c + r] * (P1[c] - tt[c]); P2[r] /= st; }
        mock::KeyPoint& k1 = S.K1.mvKeysUn[(size_t)i];
        mock::KeyPoint& k2 = S.K2.mvKeysUn[(size_t)j];
        k1.pt.x = (float)(u + 0.6 * (urand(s) - 0.5)); k1.pt.y = (float)(v + 0.6 * (urand(s) - 0.5)); k1.octave = oct; k1.size = 31.f; k1.angle = 0.f; k1.response = 50.f; k1.class_id = -1;
        k2 = k1;
        k2.pt.x = (float)(517.3 * P2[0] / P2[2] + 318.6 + 0.6 * (urand(s) - 0.5)); k2.pt.y = (float)(516.5 * P2[1] / P2[2] + 255.3 + 0.6 * (urand(s) - 0.5));
        unsigned char* d1 = S.K1.mDescriptors.ptr<unsigned char>(i);
        unsigned char* d2 = S.K2.mDescriptors.ptr<unsigned char>(j);
        for (int b = 0; b < 32; b++) { d1[b] = (unsigned char)(urand(s) * 256); d2[b] = d1[b]; }
        for (int f = 0; f < 6; f++) { const int bit = (int)(urand(s) * 256) % 256; d2[bit / 8] ^= (unsigned char)(1 << (bit % 8)); }
        const double n1 = sqrt(P1[0] * P1[0] + P1[1] * P1[1] + P1[2] * P1[2]), n2 = sqrt(P2[0] * P2[0] + P2[1] * P2[1] + P2[2] * P2[2]);
        for (int side = 0; side < 2; side++) {
            if (side == 0 && i >= holds) continue;
            S.pts.emplace_back(new MapPoint());
            MapPoint* m = S.pts.back().get();
            const double* P = side ? P2 : P1;
            const double* R = side ? R2 : R1;
            const double* t = side ? t2 : t1;
            for (int r = 0; r < 3; r++) { double w = 0; for (int c = 0; c < 3; c++) w += R[3 * c + r] * (P[c] - t[c]); m->mWorldPos.at<float>(r, 0) = (float)w; }
            m->mfMaxDistance = (float)(0.95 * (side ? n2 : n1) * S.K1.mvScaleFactors[(size_t)oct]);
            m->mfMinDistance = m->mfMaxDistance / S.K1.mvScaleFactors[NLEVELS - 1];
            const unsigned char* d = side ? d2 : d1;
            for (int b = 0; b < 32; b++) m->mDescriptor.ptr<unsigned char>(0)[b] = d[b];
            mock::KeyFrame& K = side ? S.K2 : S.K1;
            const int f = side ? j : i;
            K.mvpMapPoints[(size_t)f] = m;
            m->AddObservation(&K, (size_t)f);
            m->poolId = id0 + (side ? n + j : i);
            m->id = m->poolId;
        }
    }
}

}  // namespace cmock
