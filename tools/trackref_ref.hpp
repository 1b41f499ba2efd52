// trackref_ref.hpp -- Tracking::TrackReferenceKeyFrame (src/Tracking.cc:802-844) around its search, restated over flat arrays
// (include/orbslamm_trackpose.h): which keyframe features SearchByBoW asks (src/ORBmatcher.cc:191-197), the merge
// of its match table into mvpMapPoints through the keyframe's match list (:236, Tracking.cc:817), the gate (Tracking.cc:814,
// :1436), the solve and the loop of :818-841 (tools/trackpose_ref.hpp: the same merge, edge list, solve and discard loop as
// TrackWithMotionModel's), and the verdict (:843).  Plain C++11, no project header but trackpose_ref.hpp: the side
// orbq_track_reference is held to, byte for byte.  The search itself (ORBmatcher.cc:159-290) is the oracle's
// (oracle.search_by_bow with the validity array this file makes): its table comes in as match[t].
//
// The arrays: the keyframe's match list as entries[nEntries] (the store's row: a pool id, bit 30 set for a point in the match
// slot that does not vote, or -1), the store's stride, the keyframe's feature count; the pool as pos[3 * id] and flags[id] (bit 0
// isBad, bit 1 Observations() > 0); the frame's mvKeysUn as keys[n]; match[t] = the keyframe feature matched to frame feature t.
#pragma once

#include "trackpose_ref.hpp"

namespace trackref_ref {

const int32_t kNoVote = 1 << 30;   // ORBU_ENTRY_NO_VOTE
enum Status { kTracked = 0, kTooFew = 1, kSearchOnly = 2 };   // ORBQ_REF_*

struct KeyFrame { const int32_t* entries; int nEntries; int stride; int nFeatures; };
struct Result { trackpose_ref::Result track; int32_t nBow, status; };
// which branches ran, for the tests that must see each one
struct Branches {
    int nNull, nBad, nNoVote, nBeyondStride, nValid;                                  // the validity rule, per keyframe feature
    int gateTaken, nDiscarded, nInlierObserved, nInlierUnobserved, nRepeatedId;       // behind the search
};

// the entry of keyframe feature q as the store holds it: nothing at or above the stride, nothing behind the row's end
inline int32_t entryOf(const KeyFrame& kf, int q) { return q < kf.stride && q < kf.nEntries ? kf.entries[q] : -1; }

// ORBmatcher.cc:185-197: const unsigned int realIdxKF = vIndicesKF[iKF]; MapPoint* pMP = vpMapPointsKF[realIdxKF];
// if(!pMP) continue; if(pMP->isBad()) continue;  -> valid[q] for every keyframe feature.  The keyframe's own isBad() is not asked.
inline void validity(const trackpose_ref::Pool& pool, const KeyFrame& kf, uint8_t* valid, Branches& b)
{
    for (int q = 0; q < kf.nFeatures; q++) {
        valid[q] = 0;
        if (q >= kf.stride) { b.nBeyondStride++; continue; }      // the store keeps `stride` entries a keyframe: no point there
        const int32_t e = entryOf(kf, q);
        if (e < 0) { b.nNull++; continue; }                        // :193 if(!pMP) continue;
        const int32_t id = e & ~kNoVote;                           // (bit 30: still a point in the match slot)
        if (e & kNoVote) b.nNoVote++;
        if (id >= pool.cap) { b.nNull++; continue; }
        if (pool.flags[id] & 1) { b.nBad++; continue; }            // :196 if(pMP->isBad()) continue;
        valid[q] = 1;
        b.nValid++;
    }
}

// Everything behind the search.  0, or -1: an input the device refuses with ORBX_E_INVALID behind its kernel (nothing written).
inline int trackReference(const trackpose_ref::Pool& pool, const KeyFrame& kf, const int32_t* match, const trackpose_ref::Key* keys, int n, int solve,
                          int minMatches, const poseopt_ref::Frame& frame, const float* invLevelSigma2, int nlevels, Result& res, int32_t* idsOut,
                          uint8_t* outlierOut, Branches* br)
{
    Branches b = br ? *br : Branches();
    // ORBmatcher.cc:236 vpMapPointMatches[bestIdxF]=pMP (pMP = vpMapPointsKF[realIdxKF]); :289 return nmatches (behind the rotation
    // pruning of :268-287, which the table has seen)
    std::vector<int32_t> ids((size_t)(kf.nFeatures > 0 ? kf.nFeatures : 0), -1);
    for (int q = 0; q < kf.nFeatures; q++) {
        const int32_t e = entryOf(kf, q);
        ids[(size_t)q] = e < 0 ? -1 : (e & ~kNoVote);
    }
    int nBow = 0;
    for (int t = 0; t < n; t++) {
        if (match[t] < 0) continue;
        if (match[t] >= kf.nFeatures || ids[(size_t)match[t]] < 0 || ids[(size_t)match[t]] >= pool.cap) return -1;   // (a match names a feature that holds a point)
        nBow++;
    }
    std::memset(&res, 0, sizeof res);
    res.nBow = nBow;
    const bool gate = nBow < minMatches;                           // Tracking.cc:814 / :1436 if(nmatches<15)
    if (gate) b.gateTaken++;
    if (gate || !solve) {
        // the reference returns (:815) or goes on to the PnP solver (:1441) before it touches the frame: no solve, the pose as it came
        res.status = gate ? kTooFew : kSearchOnly;
        for (int i = 0; i < 16; i++) res.track.opt.Tcw[i] = frame.Tcw[i];
        for (int t = 0; t < n; t++) { idsOut[t] = match[t] >= 0 ? ids[(size_t)match[t]] : -1; outlierOut[t] = 0; }   // Tracking.cc:817, were it reached
        res.track.nMatches = nBow; res.track.nMatchesMap = 0;
        if (br) *br = b;
        return 0;
    }
    // Tracking.cc:817 mCurrentFrame.mvpMapPoints = vpMapPointMatches (whole: no id survives from before); :818 SetPose(mLastFrame.mTcw);
    // :820 PoseOptimization; :824-841 the discard loop -- trackpose_ref's merge with no base ids, its edge list, solve and loop
    trackpose_ref::Job J;
    J.keys = keys; J.assign = match; J.ids = ids.data(); J.nq = kf.nFeatures; J.baseIds = nullptr; J.n = n; J.discard = 1; J.frame = frame;
    trackpose_ref::Branches tb;
    if (trackpose_ref::trackPose(pool, J, invLevelSigma2, nlevels, res.track, idsOut, outlierOut, &tb)) return -1;
    res.nBow = nBow; res.status = kTracked;
    b.nDiscarded += tb.nOutlierDiscarded; b.nInlierObserved += tb.nInlierObserved; b.nInlierUnobserved += tb.nInlierUnobserved;
    b.nRepeatedId += tb.nRepeatedId;
    if (br) *br = b;
    return 0;
}

// Tracking.cc:843 return nmatchesMap>=10; (behind :814's return false)
inline bool referenceVerdict(int status, int nMatchesMap) { return status == kTracked && nMatchesMap >= 10; }

}  // namespace trackref_ref
