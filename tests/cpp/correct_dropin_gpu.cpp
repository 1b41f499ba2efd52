// iORB_SLAM::CorrectLoopPosesT (include/LoopClosing_hip.hpp) over the mocks of mock_correct.hpp against LoopClosing.cc:455-524
// (round 0: the current keyframe's neighbourhood) and MultiMapper.cc:523-595 (round 1: every keyframe of the map, the same
// current keyframe, so the points of round 0 are the already corrected ones) written serially on the same mocks, their maps
// ordered by mnId: the DEFINED order of include/orbslamm_correct.h.  The Sim3 and pose arithmetic of the serial side is
// tools/correct_ref.hpp's.  Build with -ffp-contract=off.  Prints "correct drop-in: ok" and returns 0 when every member of every
// keyframe and point and both maps agree byte for byte after each round, and the pool holds what the host points hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <vector>

#include "LoopClosing_hip.hpp"
#include "mock_correct.hpp"
#include "dropin_test.hpp"
#include "correct_ref.hpp"

using cmock::KeyFrame;
using cmock::MapPoint;
typedef s3mock::Sim3 MSim3;
typedef correct_ref::Sim3 RSim3;

static uint32_t g_rng;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 10000) / 10000.f; }

const int NKF = 30, NF = 64, NPT = 300, NLEVELS = 8;

struct World {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> pts;
};

static void build(World& W)
{
    g_rng = 4242u;
    std::vector<float> sf(NLEVELS);
    sf[0] = 1.f;
    for (int l = 1; l < NLEVELS; l++) sf[(size_t)l] = sf[(size_t)l - 1] * 1.2f;
    W.kfs.assign((size_t)NKF, KeyFrame());
    W.pts.assign((size_t)NPT, MapPoint());
    for (int k = 0; k < NKF; k++) {
        KeyFrame& K = W.kfs[(size_t)k];
        K.mnId = (unsigned long)k;
        K.mvpMapPoints.assign((size_t)NF, nullptr); K.mvOctaves.resize((size_t)NF);
        for (int i = 0; i < NF; i++) K.mvOctaves[(size_t)i] = (int)(rnd() % NLEVELS);
        K.mvScaleFactors = sf; K.mnScaleLevels = NLEVELS;
        const double ax = rndf(-1.f, 1.f), ay = rndf(-1.f, 1.f), az = rndf(0.2f, 1.f), an = std::sqrt(ax * ax + ay * ay + az * az), th = rndf(-3.f, 3.f);
        const double x = ax / an, y = ay / an, z = az / an, c = std::cos(th), s = std::sin(th), C = 1 - c;
        const double R[9] = {c + x * x * C, x * y * C - z * s, x * z * C + y * s, y * x * C + z * s, c + y * y * C, y * z * C - x * s, z * x * C - y * s, z * y * C + x * s, c + z * z * C};
        for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) K.Tcw[4 * r + q] = (float)R[3 * r + q]; K.Tcw[4 * r + 3] = rndf(-3.f, 3.f); }
        correct_ref::setPose(K.Tcw, 0, K.Ow);
    }
    W.kfs[3].mvOctaves.assign((size_t)NF, NLEVELS);            // a reference keyframe whose octaves are out of range
    for (int p = 0; p < NPT; p++) {
        MapPoint& P = W.pts[(size_t)p];
        P.mnId = (unsigned long)p; P.mbBad = p % 23 == 5;
        P.mnCorrectedByKF = 1000000; P.mnCorrectedReference = 1000000;
        for (int c = 0; c < 3; c++) { P.mWorldPos[c] = rndf(-6.f, 6.f); P.mNormalVector[c] = rndf(-1.f, 1.f); }
        P.mfMinDistance = rndf(0.1f, 1.f); P.mfMaxDistance = rndf(4.f, 9.f);
        const int nobs = 1 + (int)(rnd() % 6);
        for (int o = 0; o < nobs; o++) {
            KeyFrame& K = W.kfs[rnd() % NKF];
            size_t i = rnd() % NF, tries = 0;
            while (K.mvpMapPoints[i] && tries++ < (size_t)NF) i = (i + 1) % NF;
            if (K.mvpMapPoints[i]) continue;
            K.mvpMapPoints[i] = &P;
            if (rnd() % 10 && !P.mObservations.count(&K)) P.mObservations[&K] = i;   // else: in the match slot, not in the observations
        }
        if (!P.mObservations.empty()) {
            std::map<KeyFrame*, size_t, cmock::ById>::iterator mit = P.mObservations.begin();
            std::advance(mit, (long)(rnd() % P.mObservations.size()));
            P.mpRefKF = mit->first;
        }
        if (p % 29 == 3) P.mpRefKF = nullptr;
        if (p % 31 == 4) P.mpRefKF = &W.kfs[(size_t)((p / 31) % NKF)];
    }
}

static double norm3(const float* v) { return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

// MapPoint.cc:330-371 on the mocks; false where the reference is undefined
static bool UpdateNormalAndDepth(MapPoint* p)
{
    if (p->mbBad) return true;
    if (p->mObservations.empty()) return true;
    float normal[3] = {0.f, 0.f, 0.f};
    int n = 0;
    for (std::map<KeyFrame*, size_t, cmock::ById>::iterator mit = p->mObservations.begin(); mit != p->mObservations.end(); mit++) {
        float normali[3];
        for (int c = 0; c < 3; c++) normali[c] = p->mWorldPos[c] - mit->first->Ow[c];
        const float a = (float)(1. / norm3(normali));
        for (int c = 0; c < 3; c++) { const float t = normali[c] * a; normal[c] = t + normal[c]; }
        n++;
    }
    KeyFrame* pRefKF = p->mpRefKF;
    if (!pRefKF || !p->mObservations.count(pRefKF)) return false;
    const int level = pRefKF->mvOctaves[p->mObservations[pRefKF]];
    if (level < 0 || level >= pRefKF->mnScaleLevels) return false;
    float PC[3];
    for (int c = 0; c < 3; c++) PC[c] = p->mWorldPos[c] - pRefKF->Ow[c];
    const float dist = (float)norm3(PC);
    p->mfMaxDistance = dist * pRefKF->mvScaleFactors[(size_t)level];
    p->mfMinDistance = p->mfMaxDistance / pRefKF->mvScaleFactors[(size_t)pRefKF->mnScaleLevels - 1];
    const double alpha = 1. / n;
    for (int c = 0; c < 3; c++) p->mNormalVector[c] = alpha == 1. ? normal[c] + 0.f : (float)((double)normal[c] * alpha);
    return true;
}

typedef std::map<KeyFrame*, RSim3, cmock::ById> RefPoses;

// LoopClosing.cc:444-524 (merge: MultiMapper.cc:512-595, whose :567 joins the two skips in one condition) on the mocks
static void CorrectSerial(const std::vector<KeyFrame*>& list, KeyFrame* cur, const RSim3& Scw, bool merge, RefPoses& CorrectedSim3, RefPoses& NonCorrectedSim3,
                          int& nMoved, int& nUndefined)
{
    CorrectedSim3[cur] = Scw;                                                 // :445
    float Twc[16], unused[3];
    correct_ref::setPose(cur->Tcw, Twc, unused);                              // :446
    for (size_t v = 0; v < list.size(); v++) {                                // :455
        KeyFrame* pKFi = list[v];
        const float* Tiw = pKFi->Tcw;                                         // :459
        if (pKFi != cur) {                                                    // :461
            float Tic[12];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) Tic[4 * r + c] = correct_ref::gemmElem4(Tiw + 4 * r, Twc + c, 4);   // :463
            CorrectedSim3[pKFi] = sim3opt_ref::sim3Mul(correct_ref::sim3OfPose(Tic), Scw);   // :466-469
        }
        NonCorrectedSim3[pKFi] = correct_ref::sim3OfPose(Tiw);                // :472-476
    }
    for (RefPoses::iterator mit = CorrectedSim3.begin(); mit != CorrectedSim3.end(); mit++) {   // :480
        KeyFrame* pKFi = mit->first;
        const RSim3 g2oCorrectedSiw = mit->second;
        const RSim3 g2oCorrectedSwi = sim3opt_ref::sim3Inverse(g2oCorrectedSiw);   // :484
        const RSim3 g2oSiw = NonCorrectedSim3[pKFi];
        std::vector<MapPoint*> vpMPsi = pKFi->GetMapPointMatches();           // :488
        for (size_t iMP = 0; iMP < vpMPsi.size(); iMP++) {
            MapPoint* pMPi = vpMPsi[iMP];
            if (!pMPi) continue;                                              // :492
            if (merge) { if (pMPi->isBad() || pMPi->mnCorrectedByKF == cur->mnId) continue; }   // MultiMapper.cc:567
            else { if (pMPi->isBad()) continue; if (pMPi->mnCorrectedByKF == cur->mnId) continue; }   // :494-497
            const double P[3] = {(double)pMPi->mWorldPos[0], (double)pMPi->mWorldPos[1], (double)pMPi->mWorldPos[2]};
            double m[3], c[3];
            sim3opt_ref::sim3Map(g2oSiw, P, m);                               // :502
            sim3opt_ref::sim3Map(g2oCorrectedSwi, m, c);
            for (int k = 0; k < 3; k++) pMPi->mWorldPos[k] = (float)c[k];     // :504-505
            pMPi->mnCorrectedByKF = cur->mnId;                                // :506
            pMPi->mnCorrectedReference = pKFi->mnId;                          // :507
            if (!UpdateNormalAndDepth(pMPi)) nUndefined++;                    // :508
            nMoved++;
        }
        double eigR[9];
        poseopt_ref::quatToMatrix(g2oCorrectedSiw.q, eigR);                   // :512
        const double f = 1. / g2oCorrectedSiw.s;                              // :514-516
        float T[12];
        for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) T[4 * r + q] = (float)eigR[3 * r + q]; T[4 * r + 3] = (float)(g2oCorrectedSiw.t[r] * f); }   // :518
        std::memcpy(pKFi->Tcw, T, sizeof T);                                  // :520 SetPose
        correct_ref::setPose(T, 0, pKFi->Ow);
        pKFi->setPoseCalls++;
    }
}

struct Hooks {
    World* W;
    int32_t SlotOfKF(KeyFrame* k) { return (int32_t)k->mnId; }
    int32_t IdOfPoint(MapPoint* p) { return (int32_t)p->mnId; }
    MapPoint* PointOfId(int32_t id) { return &W->pts[(size_t)id]; }
    void Pose(KeyFrame* k, float* T) { std::memcpy(T, k->Tcw, 48); }
    void SetPose(KeyFrame* k, const float* T) { std::memcpy(k->Tcw, T, 48); correct_ref::setPose(T, 0, k->Ow); k->setPoseCalls++; }
    void SetWorldPos(MapPoint* p, const float* x) { for (int c = 0; c < 3; c++) p->mWorldPos[c] = x[c]; }
    void SetNormalAndDepth(MapPoint* p, const float* nrm, float mn, float mx) { for (int c = 0; c < 3; c++) p->mNormalVector[c] = nrm[c]; p->mfMinDistance = mn; p->mfMaxDistance = mx; }
};

static bool same_sim3(const MSim3& a, const RSim3& b)
{
    double v[8];
    for (int c = 0; c < 4; c++) v[c] = a.rotation().coeffs()[c];
    for (int c = 0; c < 3; c++) v[4 + c] = a.translation()[c];
    v[7] = a.scale();
    return !std::memcmp(v, b.q, 32) && !std::memcmp(v + 4, b.t, 24) && !std::memcmp(v + 7, &b.s, 8);
}

int main()
{
    World dev, host;   // the world the drop-in corrects, the world the serial loops correct
    build(dev);
    build(host);
    orbm_t* h = nullptr;
    orbw_pool_t* pool = nullptr;
    orbu_store_t* store = nullptr;
    REQUIRE(orbm_create(0, &h) == ORBX_OK);
    REQUIRE(orbw_pool_create(h, NPT, &pool) == ORBX_OK);
    REQUIRE(orbu_store_create(pool, NKF, NF, 4, NKF * NF, &store) == ORBX_OK);
    std::vector<int32_t> ids((size_t)NPT), refs((size_t)NPT);
    std::vector<OrbwPoint> recs((size_t)NPT);
    for (int p = 0; p < NPT; p++) {
        const MapPoint& P = dev.pts[(size_t)p];
        OrbwPoint& r = recs[(size_t)p];
        std::memset(&r, 0, sizeof r);
        ids[(size_t)p] = p; refs[(size_t)p] = P.mpRefKF ? (int32_t)P.mpRefKF->mnId : -1;
        for (int c = 0; c < 3; c++) { r.pos[c] = P.mWorldPos[c]; r.normal[c] = P.mNormalVector[c]; }
        r.min_distance = P.mfMinDistance; r.max_distance = P.mfMaxDistance;
        r.flags = (uint8_t)((P.mbBad ? ORBW_FLAG_BAD : 0) | (P.mObservations.empty() ? 0 : ORBW_FLAG_OBSERVED));
    }
    REQUIRE(orbw_pool_set(pool, ids.data(), recs.data(), NPT) == ORBX_OK);
    std::vector<int32_t> slots((size_t)NKF), nent((size_t)NKF, NF), entries, neigh((size_t)NKF * ORBU_MAX_NEIGHBOURS, -1), parent((size_t)NKF, -1), nch((size_t)NKF, 0);
    std::vector<uint8_t> flags((size_t)NKF, 0);
    std::vector<float> centres;
    for (int k = 0; k < NKF; k++) {
        KeyFrame& K = dev.kfs[(size_t)k];
        slots[(size_t)k] = k;
        for (int i = 0; i < NF; i++) {
            MapPoint* P = K.mvpMapPoints[(size_t)i];
            const bool observes = P && P->mObservations.count(&K) && P->mObservations[&K] == (size_t)i;
            entries.push_back(!P ? -1 : (int32_t)P->mnId | (observes ? 0 : ORBU_ENTRY_NO_VOTE));
        }
        for (int c = 0; c < 3; c++) centres.push_back(K.Ow[c]);
    }
    OrbuKeyFrames rec;
    rec.nkf = NKF; rec.slot = slots.data(); rec.flags = flags.data(); rec.n = nent.data(); rec.entries = entries.data(); rec.neigh = neigh.data();
    rec.parent = parent.data(); rec.nchildren = nch.data(); rec.children = nullptr;
    REQUIRE(orbu_kf_set(store, &rec) == ORBX_OK);
    for (int k = 0; k < NKF; k++) {
        std::vector<uint8_t> oct((size_t)NF);
        for (int i = 0; i < NF; i++) oct[(size_t)i] = (uint8_t)dev.kfs[(size_t)k].mvOctaves[(size_t)i];
        REQUIRE(orbu_kf_set_octaves(store, k, oct.data(), NF) == ORBX_OK);
    }
    REQUIRE(orbu_kf_set_centres(store, slots.data(), centres.data(), NKF) == ORBX_OK);
    REQUIRE(orbu_point_set_ref_kf(store, ids.data(), refs.data(), NPT) == ORBX_OK);

    const int CUR = 11;
    RSim3 Scw;
    {
        const double q[4] = {0.18, -0.31, 0.22, 0.9};
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int c = 0; c < 4; c++) Scw.q[c] = q[c] / n;
        Scw.t[0] = 0.4; Scw.t[1] = -1.1; Scw.t[2] = 0.7; Scw.s = 1.23;
    }
    s3mock::Quaterniond Q;
    s3mock::Vector3d T;
    for (int c = 0; c < 4; c++) Q.coeffs()[c] = Scw.q[c];
    for (int c = 0; c < 3; c++) T[c] = Scw.t[c];
    const MSim3 mScw(Q, T, Scw.s);
    std::vector<float> sf = dev.kfs[0].mvScaleFactors;
    Hooks hooks; hooks.W = &dev;
    for (int round = 0; round < 2; round++) {
        std::vector<KeyFrame*> listDev, listHost;
        const int order[9] = {14, 2, 27, CUR, 8, 21, 5, 17, 9};     // round 0: the neighbourhood, the current keyframe among it, out of order
        for (int k = 0; k < (round == 0 ? 9 : NKF); k++) {
            const int slot = round == 0 ? order[k] : (k * 7) % NKF;
            listDev.push_back(&dev.kfs[(size_t)slot]); listHost.push_back(&host.kfs[(size_t)slot]);
        }
        std::vector<MapPoint*> already;
        for (int p = 0; p < NPT; p++) if (dev.pts[(size_t)p].mnCorrectedByKF == (unsigned long)CUR) already.push_back(&dev.pts[(size_t)p]);
        REQUIRE(round == 0 ? already.empty() : !already.empty());
        RefPoses wantC, wantN;
        int movedHost = 0, undefinedHost = 0;
        CorrectSerial(listHost, &host.kfs[(size_t)CUR], Scw, round == 1, wantC, wantN, movedHost, undefinedHost);
        cmock::KeyFrameAndPose gotC, gotN;
        typedef iORB_SLAM::CorrectLoopPosesT<KeyFrame, MapPoint, MSim3> Correct;
        const Correct::Result res = Correct::Run(store, listDev, &dev.kfs[(size_t)CUR], mScw, already, sf, gotC, gotN, hooks);
        REQUIRE(res.nMoved == movedHost && movedHost > 20 && res.nUndefined == undefinedHost && undefinedHost > 0 && res.nNormals > 10);
        REQUIRE(gotC.size() == wantC.size() && gotN.size() == wantN.size() && gotC.size() == listDev.size());
        for (size_t k = 0; k < listDev.size(); k++) {
            if (!same_sim3(gotC[listDev[k]], wantC[listHost[k]]) || !same_sim3(gotN[listDev[k]], wantN[listHost[k]])) {
                std::printf("round %d: the Sim3 of keyframe %lu differ\n", round, listDev[k]->mnId);
                return 1;
            }
        }
        for (int k = 0; k < NKF; k++) {
            const KeyFrame &a = dev.kfs[(size_t)k], &b = host.kfs[(size_t)k];
            if (std::memcmp(a.Tcw, b.Tcw, 48) || std::memcmp(a.Ow, b.Ow, 12) || a.setPoseCalls != b.setPoseCalls) { std::printf("round %d: keyframe %d differs\n", round, k); return 1; }
        }
        std::vector<OrbwPoint> now((size_t)NPT);
        REQUIRE(orbw_debug_pool_get(pool, ids.data(), NPT, now.data()) == ORBX_OK);
        for (int p = 0; p < NPT; p++) {
            const MapPoint &a = dev.pts[(size_t)p], &b = host.pts[(size_t)p];
            if (std::memcmp(a.mWorldPos, b.mWorldPos, 12) || std::memcmp(a.mNormalVector, b.mNormalVector, 12) || std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) ||
                std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) || a.mnCorrectedByKF != b.mnCorrectedByKF || a.mnCorrectedReference != b.mnCorrectedReference) {
                std::printf("round %d: point %d differs from the serial loop\n", round, p);
                return 1;
            }
            const OrbwPoint& r = now[(size_t)p];
            if (std::memcmp(r.pos, a.mWorldPos, 12) || std::memcmp(r.normal, a.mNormalVector, 12) || std::memcmp(&r.min_distance, &a.mfMinDistance, 4) ||
                std::memcmp(&r.max_distance, &a.mfMaxDistance, 4) || r.flags != recs[(size_t)p].flags) {
                std::printf("round %d: the pool's record of point %d differs from the host point\n", round, p);
                return 1;
            }
        }
    }
    REQUIRE(orbu_store_destroy(store) == ORBX_OK);
    REQUIRE(orbw_pool_destroy(pool) == ORBX_OK);
    orbm_destroy(h);
    std::printf("correct drop-in: ok\n");
    return 0;
}
