// iORB_SLAM::RefreshMapPointsT (include/MapPoint_hip.hpp) over the mocks of mock_refresh.hpp against
// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371) written serially on
// the same mocks, their maps ordered by mnId: the DEFINED order of include/orbslamm_refresh.h.  Build with -ffp-contract=off.
// Prints "refresh drop-in: ok" and returns 0 when every member of every point agrees byte for byte, after a plain refresh and
// after one with moved positions, and the pool holds what the host points hold.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <vector>

#include "MapPoint_hip.hpp"
#include "mock_refresh.hpp"
#include "dropin_test.hpp"

using rmock::KeyFrame;
using rmock::MapPoint;

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 10000) / 10000.f; }

// ---- the two members, serially, on the mocks
static void ComputeDistinctiveDescriptors(MapPoint* p)
{
    if (p->mbBad) return;                                                     // :251
    if (p->mObservations.empty()) return;                                     // :256
    std::vector<const uint8_t*> vDescriptors;
    for (std::map<KeyFrame*, size_t, rmock::ById>::iterator mit = p->mObservations.begin(); mit != p->mObservations.end(); mit++)
        if (!mit->first->isBad()) vDescriptors.push_back(&mit->first->mDescriptors[mit->second * 32]);   // :265-266
    if (vDescriptors.empty()) return;                                         // :269
    const size_t N = vDescriptors.size();
    std::vector<float> Distances(N * N, 0.f);
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) Distances[i * N + j] = Distances[j * N + i] = (float)descriptorDistance(vDescriptors[i], vDescriptors[j]);
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances.begin() + (long)(i * N), Distances.begin() + (long)(i * N + N));
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (double)(N - 1))];           // :294
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    std::memcpy(p->mDescriptor, vDescriptors[(size_t)BestIdx], 32);           // :305
}

static double norm3(const float* v) { return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

// returns false where the reference is undefined (no reference keyframe among the observations, its octave out of range)
static bool UpdateNormalAndDepth(MapPoint* p)
{
    if (p->mbBad) return true;                                                // :338
    if (p->mObservations.empty()) return true;                                // :345
    float normal[3] = {0.f, 0.f, 0.f};
    int n = 0;
    for (std::map<KeyFrame*, size_t, rmock::ById>::iterator mit = p->mObservations.begin(); mit != p->mObservations.end(); mit++) {
        float normali[3];
        for (int c = 0; c < 3; c++) normali[c] = p->mWorldPos[c] - mit->first->mOw[c];   // :354
        const float a = (float)(1. / norm3(normali));
        for (int c = 0; c < 3; c++) { const float t = normali[c] * a; normal[c] = t + normal[c]; }   // :355
        n++;
    }
    KeyFrame* pRefKF = p->mpRefKF;
    if (!pRefKF || !p->mObservations.count(pRefKF)) return false;
    const int level = pRefKF->mvOctaves[p->mObservations[pRefKF]];            // :361
    if (level < 0 || level >= pRefKF->mnScaleLevels) return false;
    float PC[3];
    for (int c = 0; c < 3; c++) PC[c] = p->mWorldPos[c] - pRefKF->mOw[c];     // :359
    const float dist = (float)norm3(PC);                                      // :360
    p->mfMaxDistance = dist * pRefKF->mvScaleFactors[(size_t)level];          // :367
    p->mfMinDistance = p->mfMaxDistance / pRefKF->mvScaleFactors[(size_t)pRefKF->mnScaleLevels - 1];   // :368
    const double alpha = 1. / n;
    for (int c = 0; c < 3; c++) p->mNormalVector[c] = alpha == 1. ? normal[c] + 0.f : (float)((double)normal[c] * alpha);   // :369
    return true;
}

struct Hooks {
    int32_t IdOfPoint(MapPoint* p) { return (int32_t)p->mnId; }
    int32_t SlotOfKF(KeyFrame* k) { return (int32_t)k->mnId; }
    void WorldPos(MapPoint* p, float* o) { for (int c = 0; c < 3; c++) o[c] = p->mWorldPos[c]; }
    void SetDescriptor(MapPoint* p, const uint8_t* d) { std::memcpy(p->mDescriptor, d, 32); }
    void SetNormalAndDepth(MapPoint* p, const float* nrm, float mn, float mx) { for (int c = 0; c < 3; c++) p->mNormalVector[c] = nrm[c]; p->mfMinDistance = mn; p->mfMaxDistance = mx; }
};

static bool same_members(const MapPoint& a, const MapPoint& b)
{
    return !std::memcmp(a.mDescriptor, b.mDescriptor, 32) && !std::memcmp(a.mNormalVector, b.mNormalVector, 12) && !std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) &&
           !std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) && !std::memcmp(a.mWorldPos, b.mWorldPos, 12);
}

int main()
{
    const int NKF = 30, NF = 96, NPT = 200, NLEVELS = 8;
    std::vector<float> sf(NLEVELS);
    sf[0] = 1.f;
    for (int l = 1; l < NLEVELS; l++) sf[(size_t)l] = sf[(size_t)l - 1] * 1.2f;
    std::vector<KeyFrame> kfs((size_t)NKF);
    std::vector<MapPoint> dev((size_t)NPT), host((size_t)NPT);   // the points the drop-in refreshes, the points the members refresh
    for (int k = 0; k < NKF; k++) {
        KeyFrame& K = kfs[(size_t)k];
        K.mnId = (unsigned long)k; K.N = NF; K.mbBad = k == 7 || k == 19;
        K.mDescriptors.resize((size_t)NF * 32); K.mvOctaves.resize((size_t)NF); K.mvpMapPoints.assign((size_t)NF, nullptr);
        for (size_t b = 0; b < K.mDescriptors.size(); b++) K.mDescriptors[b] = (uint8_t)rnd();
        for (int i = 0; i < NF; i++) K.mvOctaves[(size_t)i] = (int)(rnd() % NLEVELS);
        K.mvScaleFactors = sf; K.mnScaleLevels = NLEVELS;
        for (int c = 0; c < 3; c++) K.mOw[c] = rndf(-3.f, 3.f);
    }
    kfs[3].mvOctaves.assign((size_t)NF, NLEVELS);              // a reference keyframe whose octaves are out of range
    for (int p = 0; p < NPT; p++) {
        MapPoint& P = dev[(size_t)p];
        P.mnId = (unsigned long)p; P.mbBad = p % 23 == 5;
        for (int c = 0; c < 3; c++) { P.mWorldPos[c] = rndf(-6.f, 6.f); P.mNormalVector[c] = rndf(-1.f, 1.f); }
        P.mfMinDistance = rndf(0.1f, 1.f); P.mfMaxDistance = rndf(4.f, 9.f);
        for (int b = 0; b < 32; b++) P.mDescriptor[b] = (uint8_t)rnd();
        const int nobs = p % 17 == 0 ? 0 : 1 + (int)(rnd() % 9);
        for (int o = 0; o < nobs; o++) {
            KeyFrame& K = kfs[rnd() % NKF];
            if (P.mObservations.count(&K)) continue;
            size_t i = rnd() % NF;
            while (K.mvpMapPoints[i]) i = (i + 1) % NF;
            K.mvpMapPoints[i] = &P;
            P.AddObservation(&K, i);
        }
        if (!P.mObservations.empty()) {
            std::map<KeyFrame*, size_t, rmock::ById>::iterator mit = P.mObservations.begin();
            std::advance(mit, (long)(rnd() % P.mObservations.size()));
            P.mpRefKF = mit->first;
        }
        if (p % 29 == 3) P.mpRefKF = nullptr;                  // no reference keyframe
        if (p % 31 == 4) P.mpRefKF = &kfs[(size_t)((p / 31) % NKF)];   // perhaps one that does not observe the point
        host[(size_t)p] = P;
    }
    // ---- the pool and the store as the caller keeps them
    orbm_t* h = nullptr;
    orbw_pool_t* pool = nullptr;
    orbu_store_t* store = nullptr;
    REQUIRE(orbm_create(0, &h) == ORBX_OK);
    REQUIRE(orbw_pool_create(h, NPT, &pool) == ORBX_OK);
    REQUIRE(orbu_store_create(pool, NKF, NF, 4, NKF * NF, &store) == ORBX_OK);
    std::vector<int32_t> ids((size_t)NPT);
    std::vector<OrbwPoint> recs((size_t)NPT);
    for (int p = 0; p < NPT; p++) {
        const MapPoint& P = dev[(size_t)p];
        OrbwPoint& r = recs[(size_t)p];
        std::memset(&r, 0, sizeof r);
        ids[(size_t)p] = p;
        for (int c = 0; c < 3; c++) { r.pos[c] = P.mWorldPos[c]; r.normal[c] = P.mNormalVector[c]; }
        r.min_distance = P.mfMinDistance; r.max_distance = P.mfMaxDistance;
        std::memcpy(r.desc, P.mDescriptor, 32);
        r.flags = (uint8_t)((P.mbBad ? ORBW_FLAG_BAD : 0) | (P.mObservations.empty() ? 0 : ORBW_FLAG_OBSERVED));
    }
    REQUIRE(orbw_pool_set(pool, ids.data(), recs.data(), NPT) == ORBX_OK);
    std::vector<int32_t> slots((size_t)NKF), nent((size_t)NKF, NF), entries, neigh((size_t)NKF * ORBU_MAX_NEIGHBOURS, -1), parent((size_t)NKF, -1), nch((size_t)NKF, 0);
    std::vector<uint8_t> flags((size_t)NKF);
    std::vector<float> centres;
    for (int k = 0; k < NKF; k++) {
        slots[(size_t)k] = k; flags[(size_t)k] = kfs[(size_t)k].mbBad ? ORBU_KF_BAD : 0;
        for (int i = 0; i < NF; i++) entries.push_back(kfs[(size_t)k].mvpMapPoints[(size_t)i] ? (int32_t)kfs[(size_t)k].mvpMapPoints[(size_t)i]->mnId : -1);
        for (int c = 0; c < 3; c++) centres.push_back(kfs[(size_t)k].mOw[c]);
    }
    OrbuKeyFrames rec;
    rec.nkf = NKF; rec.slot = slots.data(); rec.flags = flags.data(); rec.n = nent.data(); rec.entries = entries.data(); rec.neigh = neigh.data();
    rec.parent = parent.data(); rec.nchildren = nch.data(); rec.children = nullptr;
    REQUIRE(orbu_kf_set(store, &rec) == ORBX_OK);
    for (int k = 0; k < NKF; k++) {
        std::vector<uint8_t> oct((size_t)NF);
        for (int i = 0; i < NF; i++) oct[(size_t)i] = (uint8_t)kfs[(size_t)k].mvOctaves[(size_t)i];
        REQUIRE(orbu_kf_set_octaves(store, k, oct.data(), NF) == ORBX_OK);
        REQUIRE(orbu_kf_set_descriptors(store, k, kfs[(size_t)k].mDescriptors.data(), NF) == ORBX_OK);
    }
    REQUIRE(orbu_kf_set_centres(store, slots.data(), centres.data(), NKF) == ORBX_OK);
    // ---- round 0: both halves as they stand; round 1: every point moved, normal and depth alone
    Hooks hooks;
    std::vector<MapPoint*> list;
    for (int p = 0; p < NPT; p++) list.push_back(&dev[(size_t)((p * 7) % NPT)]);   // (7 and 200 are coprime: every point once, out of order)
    for (int round = 0; round < 2; round++) {
        if (round == 1)
            for (int p = 0; p < NPT; p++)
                for (int c = 0; c < 3; c++) host[(size_t)p].mWorldPos[c] = dev[(size_t)p].mWorldPos[c] = dev[(size_t)p].mWorldPos[c] + rndf(-0.3f, 0.3f);
        int undefinedHost = 0;
        for (int p = 0; p < NPT; p++) {
            if (round == 0) ComputeDistinctiveDescriptors(&host[(size_t)p]);
            if (!UpdateNormalAndDepth(&host[(size_t)p])) undefinedHost++;
        }
        const iORB_SLAM::RefreshMapPointsT<KeyFrame, MapPoint>::Result res =
            iORB_SLAM::RefreshMapPointsT<KeyFrame, MapPoint>::Run(store, list, round == 0 ? ORBR_DESCRIPTOR | ORBR_NORMAL_DEPTH : ORBR_NORMAL_DEPTH, round == 1, sf, hooks);
        REQUIRE(res.nUndefined == undefinedHost && undefinedHost > 0);
        REQUIRE(res.nNormals > NPT / 2 && (round == 1 || res.nDescriptors > NPT / 2));
        for (int p = 0; p < NPT; p++)
            if (!same_members(dev[(size_t)p], host[(size_t)p])) { std::printf("round %d: point %d differs from the members\n", round, p); return 1; }
        std::vector<OrbwPoint> now((size_t)NPT);
        REQUIRE(orbw_debug_pool_get(pool, ids.data(), NPT, now.data()) == ORBX_OK);
        for (int p = 0; p < NPT; p++) {
            const MapPoint& P = dev[(size_t)p];
            const OrbwPoint& r = now[(size_t)p];
            if (std::memcmp(r.pos, P.mWorldPos, 12) || std::memcmp(r.normal, P.mNormalVector, 12) || std::memcmp(&r.min_distance, &P.mfMinDistance, 4) ||
                std::memcmp(&r.max_distance, &P.mfMaxDistance, 4) || std::memcmp(r.desc, P.mDescriptor, 32) || r.flags != recs[(size_t)p].flags) {
                std::printf("round %d: the pool's record of point %d differs from the host point\n", round, p);
                return 1;
            }
        }
    }
    REQUIRE(orbu_store_destroy(store) == ORBX_OK);
    REQUIRE(orbw_pool_destroy(pool) == ORBX_OK);
    orbm_destroy(h);
    std::printf("refresh drop-in: ok\n");
    return 0;
}
