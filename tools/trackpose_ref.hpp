// trackpose_ref.hpp -- the line behind the search in Tracking::TrackWithMotionModel and Tracking::TrackLocalMap, restated over
// flat arrays (include/orbslamm_trackpose.h): the merge of the search's matches into mvpMapPoints
// (src/ORBmatcher.cc:123, :1430), the edge list of Optimizer::PoseOptimization (src/Optimizer.cc:302-341, monocular), the solve
// (tools/poseopt_ref.hpp, the Defined arithmetic the device is held to), and the loops of src/Tracking.cc:950-969 and :993-1013.
// Plain C++11, no project header but poseopt_ref.hpp: the side orbq_track_pose is held to, byte for byte.
//
// The arrays: the frame's mvKeysUn as keys[n] (pt.x, pt.y, octave); the search as assign[t] (the query matched to feature t,
// or -1) over ids[nq] (the pool id of query q); baseIds[t], the pool id of mvpMapPoints[t] before the search (-1 = NULL; a null
// array = all NULL); the pool as pos[3 * id] and flags[id] (bit 0 isBad, bit 1 Observations() > 0).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "poseopt_ref.hpp"

namespace trackpose_ref {

struct Key { float u, v; int32_t octave; };
struct Pool { const float* pos; const uint8_t* flags; int cap; };
struct Job {
    const Key* keys;
    const int32_t* assign; const int32_t* ids; int nq;   // assign null: no search is merged
    const int32_t* baseIds;
    int n;                                              // mCurrentFrame.N
    int discard;                                        // 1: TrackWithMotionModel's loop, 0: TrackLocalMap's (monocular)
    poseopt_ref::Frame frame;                           // mTcw, fx fy cx cy
};
struct Result { poseopt_ref::Result opt; int32_t nMatches, nMatchesMap; };
// which branches ran, for the tests that must see each one
struct Branches {
    int nFromBase, nFromSearch, nOverwritten, nNull, nRepeatedId, nBadFlagEdge, nEdges, nOutlierDiscarded, nOutlierKept, nInlierObserved,
        nInlierUnobserved;
};

// 0, or -1: an input the device refuses with ORBX_E_INVALID behind its kernel (nothing is written then)
inline int trackPose(const Pool& pool, const Job& J, const float* invLevelSigma2, int nlevels, Result& res, int32_t* idsOut, uint8_t* outlierOut,
                     Branches* br)
{
    Branches b = Branches();
    // mvpMapPoints after the search: a match overwrites what the slot held (ORBmatcher.cc:123: F.mvpMapPoints[bestIdx]=pMP;
    // :1430: CurrentFrame.mvpMapPoints[bestIdx2]=pMP)
    std::vector<int32_t> merged((size_t)J.n, -1);
    for (int t = 0; t < J.n; t++) {
        const int32_t base = J.baseIds ? J.baseIds[t] : -1;   // Tracking.cc:940: fill(..., NULL) before the motion-model search
        const int32_t q = J.assign ? J.assign[t] : -1;
        if (q >= 0) {
            if (q >= J.nq || J.ids[q] < 0) return -1;           // (a match names a query that holds a point)
            merged[(size_t)t] = J.ids[q];
            b.nFromSearch++;
            if (base >= 0) b.nOverwritten++;
        } else if (base >= 0) {
            merged[(size_t)t] = base;
            b.nFromBase++;
        } else
            b.nNull++;
        if (merged[(size_t)t] >= pool.cap) return -1;
    }
    // Optimizer.cc:302-341: for(int i=0; i<N; i++) if(pMP) { nInitialCorrespondences++; mvbOutlier[i] = false; obs = mvKeysUn[i].pt;
    // invSigma2 = mvInvLevelSigma2[kpUn.octave]; Xw = pMP->GetWorldPos(); vpEdgesMono.push_back(e); vnIndexEdgeMono.push_back(i); }
    // isBad() is not asked
    std::vector<poseopt_ref::Edge> edges;
    std::vector<int32_t> indexEdge;
    std::vector<uint8_t> seen((size_t)(pool.cap > 0 ? pool.cap : 0), 0);
    for (int t = 0; t < J.n; t++) {                             // :302
        const int32_t id = merged[(size_t)t];
        if (id < 0) continue;                                   // :305 if(pMP)
        const Key& kp = J.keys[t];                              // :316 kpUn = pFrame->mvKeysUn[i]
        if (kp.octave < 0 || kp.octave >= nlevels) return -1;
        poseopt_ref::Edge e;
        e.u = kp.u; e.v = kp.v;                                 // :317 obs << kpUn.pt.x, kpUn.pt.y
        e.invSigma2 = invLevelSigma2[kp.octave];                // :322 invSigma2 = pFrame->mvInvLevelSigma2[kpUn.octave]
        e.Xw[0] = pool.pos[3 * (size_t)id]; e.Xw[1] = pool.pos[3 * (size_t)id + 1]; e.Xw[2] = pool.pos[3 * (size_t)id + 2];   // :333-336
        edges.push_back(e);                                     // :339
        indexEdge.push_back(t);                                 // :340
        if (seen[(size_t)id]) b.nRepeatedId++;
        seen[(size_t)id] = 1;
        if (pool.flags[id] & 1) b.nBadFlagEdge++;
    }
    b.nEdges = (int)edges.size();
    std::vector<uint8_t> edgeOutlier(edges.size() + 1, 0);
    std::memset(&res, 0, sizeof res);
    poseopt_ref::Diag diag;
    diag.classChi2 = nullptr;
    poseopt_ref::poseOptimization<poseopt_ref::Defined>(J.frame, edges.data(), (int)edges.size(), res.opt, edgeOutlier.data(), &diag);
    for (int t = 0; t < J.n; t++) outlierOut[t] = 0;            // (a feature without an edge keeps the false of Frame's constructor)
    for (size_t e = 0; e < edges.size(); e++) outlierOut[indexEdge[e]] = edgeOutlier[e];   // :410 / :416 mvbOutlier[idx]
    int nMatches = 0, nMatchesMap = 0;
    for (int i = 0; i < J.n; i++) {                             // Tracking.cc:952 / :994
        idsOut[i] = merged[(size_t)i];
        if (merged[(size_t)i] < 0) continue;                    // :954 / :996 if(mCurrentFrame.mvpMapPoints[i])
        if (outlierOut[i]) {                                    // :956 if(mvbOutlier[i]) / the else of :998
            if (J.discard) {
                idsOut[i] = -1;                                 // :960 mvpMapPoints[i] = NULL  (:961 clears the flag: the byte returned keeps
                b.nOutlierDiscarded++;                          //  it, for :962-963 mbTrackInView / mnLastFrameSeen on the caller's side)
            } else
                b.nOutlierKept++;                               // :1009-1010: only STEREO nulls the slot
        } else {
            nMatches++;                                         // :964 nmatches-- per outlier; :1007 under mbOnlyTracking
            if (pool.flags[merged[(size_t)i]] & 2) { nMatchesMap++; b.nInlierObserved++; }   // :966-967 / :1003-1004 Observations()>0
            else b.nInlierUnobserved++;
        }
    }
    res.nMatches = nMatches; res.nMatchesMap = nMatchesMap;
    if (br) *br = b;
    return 0;
}

// Tracking.cc:971-977: TrackWithMotionModel's verdict
inline bool motionModelVerdict(int nMatches, int nMatchesMap, bool onlyTracking, bool* vo)
{
    if (onlyTracking) { if (vo) *vo = nMatchesMap < 10; return nMatches > 20; }   // :973-974
    return nMatchesMap >= 10;                                                      // :977
}

// Tracking.cc:1017-1023: TrackLocalMap's verdict
inline bool localMapVerdict(int nMatches, int nMatchesMap, bool onlyTracking, long frameId, long lastRelocFrameId, long maxFrames)
{
    const int inliers = onlyTracking ? nMatches : nMatchesMap;                     // :1001-1007
    if (frameId < lastRelocFrameId + maxFrames && inliers < 50) return false;      // :1017
    return !(inliers < 20);                                                        // :1020
}

}  // namespace trackpose_ref
