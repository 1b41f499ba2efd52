// loopfuse_ref.hpp -- a literal C++ restatement of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (src/ORBmatcher.cc:979-1102 of both scenarios, monocular) for a target whose Scw the caller has already decomposed
// (:987-992) into Rcw, tcw and Ow, of LoopClosing::SearchAndFuse (src/LoopClosing.cc:601-627) and MultiMapper::SearchAndFuse
// (src/MultiMapper.cc:668-694) over a small map model, of MapPoint::Replace and MapPoint::ComputeDistinctiveDescriptors
// (MapPoint.cc:177-215, 242-307), of KeyFrame::GetMapPoints (KeyFrame.cc:246-259), of the keyframe grid (Frame.cc:230-245,
// 382-392, KeyFrame.cc:618-657) and of the OpenCV 3.0 pieces :1014-1044 call (gemm's small-matrix branch with C, norm and
// dot on CV_32F).  It is the checker of the device SearchAndFuse (orbslamm_amd/csrc/orbc_kernels.hip): it includes no
// header of the library and is built with g++ -ffp-contract=off (every operation one IEEE op).
//
// What the two Fuse overloads share is tools/fuse_ref.hpp's, re-exported here: the layouts, the gate sequence of project,
// the keyframe grid, the window walk, and the model's keyframes, points, Replace and ComputeDistinctiveDescriptors.  Here is
// what this overload alone has.
//
// Against Fuse(pKF, vpMapPoints, th) (tools/fuse_ref.hpp): invz is `1.0/z` rounded to float (:1021), there is NO chi-square
// test in the window (:1064-1081), a hit is bestDist <= TH_LOW with no Observations() comparison: a feature that holds a
// point goes to vpReplacePoint, and the Replace calls are issued after the loop over the points (LoopClosing.cc:616-625).
// PredictScale is the DIRECT formula, ceil(log(ratio)/logScaleFactor) in float, not a break table.  Defined choices
// (DESIGN.md section 8m), the same on the device:
//   - a level that is NaN or outside [0, nlevels) ends the pair (LEVEL_RANGE; the reference reads mvScaleFactors out of
//     bounds there) and is reported as -1 (below, or NaN) or nlevels (above)
//   - std::map<KeyFrame*, size_t> is walked in pointer order in the reference; the model walks observations in insertion order
#pragma once

#include <set>
#include <vector>

#include "fuse_ref.hpp"

namespace loopfuse_ref {

using fuse_ref::KeyPt;
using fuse_ref::Grid;
using fuse_ref::Target;
using fuse_ref::Point;
using fuse_ref::Result;
using fuse_ref::Gates;
using fuse_ref::CellGrid;
using fuse_ref::Event;
using fuse_ref::EV_REPLACE;
using fuse_ref::EV_ADD;
using fuse_ref::FOUND;
using fuse_ref::TH_LOW;
using fuse_ref::descriptorDistance;
using fuse_ref::predictLevel;
struct Hit { int32_t target, point, bestIdx, bestDist; };   // OrbcHit's layout

// :1021 `const float invz = 1.0/p3Dc.at<float>(2);` as written, and the float division a device may use in its place
inline float invzAsWritten(float z) { return (float)(1.0 / (double)z); }
using fuse_ref::invzFloatDivision;

// :1010-1051 for one pair: fuse_ref's gate sequence under this overload's invz
inline bool project(const Target& T, const Point& P, float th, const float* scaleFactors, int nlevels, float logScaleFactor, Result& r,
                    Gates* g = nullptr)
{
    return fuse_ref::project(T, P, th, scaleFactors, nlevels, logScaleFactor, r, g, invzAsWritten);
}
// :1010-1081 for one (target, point) pair: the window walk (:1053-1081) has no chi-square test
inline Result pair(const Target& T, const CellGrid& grid, const KeyPt* keys, const uint8_t* desc, const Point& P, float th,
                   const float* scaleFactors, int nlevels, float logScaleFactor, Gates* g = nullptr)
{
    return fuse_ref::pair(T, grid, keys, desc, P, th, scaleFactors, nullptr, nlevels, logScaleFactor, g, invzAsWritten);
}

// ------------------------------------------------------------------------------------------------ the serial map model
// fuse_ref's keyframes and points (a keyframe's own record, covisibles and the SearchInNeighbors marks go unused: the
// targets' records come with CorrectedSim3) under the SearchAndFuse loops
struct Model : fuse_ref::Model {
    struct Corrected { int kf; Target rec; };   // one entry of CorrectedSim3: the keyframe and its decomposed Scw
    long rescored = 0;   // searchAndFuseByRule: the pairs scored again on the host

    int addKeyFrame(const Grid& grid, const KeyPt* keys, const uint8_t* desc, int n)
    {
        Target rec = Target();
        rec.grid = grid;
        return fuse_ref::Model::addKeyFrame(rec, keys, desc, n);
    }
    // KeyFrame.cc:246-259
    std::set<int> getMapPoints(int kf) const
    {
        std::set<int> s;
        for (size_t i = 0; i < kfs[kf].slot.size(); i++) if (kfs[kf].slot[i] >= 0 && !mps[kfs[kf].slot[i]].bad) s.insert(kfs[kf].slot[i]);
        return s;
    }
    Result search(const Corrected& c, int mp, float th) const
    {
        const KF& K = kfs[c.kf];
        return pair(c.rec, K.grid, K.keys.data(), K.desc.data(), mps[mp].rec, th, sf.data(), (int)sf.size(), logScaleFactor);
    }
    // :1083-1098: what Fuse does with a pair's best
    void apply(const Corrected& c, int mp, int i, int bestIdx, std::vector<int>& vpReplacePoint)
    {
        KF& K = kfs[c.kf];
        const int inKF = K.slot[bestIdx];
        if (inKF >= 0) {
            if (!mps[inKF].bad) vpReplacePoint[i] = inKF;
        } else {
            events.push_back(Event{EV_ADD, mp, c.kf, bestIdx});
            addObservation(mp, c.kf, bestIdx);
            K.slot[bestIdx] = mp;
        }
    }
    // LoopClosing.cc:601-627 / MultiMapper.cc:668-694 with ORBmatcher.cc:979-1102 inside, serially: the total of nFused
    int searchAndFuse(const std::vector<Corrected>& corrected, const std::vector<int>& loopPoints, float th)
    {
        int total = 0;
        for (size_t t = 0; t < corrected.size(); t++) {
            const Corrected& c = corrected[t];
            std::vector<int> vpReplacePoints(loopPoints.size(), -1);
            const std::set<int> spAlreadyFound = getMapPoints(c.kf);
            for (size_t i = 0; i < loopPoints.size(); i++) {
                const int mp = loopPoints[i];
                if (mps[mp].bad || spAlreadyFound.count(mp)) continue;
                const Result r = search(c, mp, th);
                if (r.status != FOUND || r.bestDist > TH_LOW) continue;
                apply(c, mp, (int)i, r.bestIdx, vpReplacePoints);
                total++;
            }
            for (size_t i = 0; i < loopPoints.size(); i++)
                if (vpReplacePoints[i] >= 0) replace(vpReplacePoints[i], loopPoints[i], (int)t);
        }
        return total;
    }
    // The dense search of every loop point in every target on the map as it stands: what the device returns (hits in
    // target-major order, points ascending; hitStart of corrected.size() + 1 entries)
    void dense(const std::vector<Corrected>& corrected, const std::vector<int>& loopPoints, float th, int maxDist, std::vector<Hit>& hits,
               std::vector<int>& hitStart) const
    {
        hits.clear(); hitStart.assign(1, 0);
        for (size_t t = 0; t < corrected.size(); t++) {
            for (size_t i = 0; i < loopPoints.size(); i++) {
                const Result r = search(corrected[t], loopPoints[i], th);
                if (r.bestIdx >= 0 && r.bestDist <= maxDist) hits.push_back(Hit{(int32_t)t, (int32_t)i, r.bestIdx, r.bestDist});
            }
            hitStart.push_back((int)hits.size());
        }
    }
    // The parallel rule: all pairs searched up front on the map as it stands, the serial part replayed
    // in the reference's order, and a pair of a point that has SURVIVED a Replace (its descriptor may have changed) scored
    // again with the descriptor it holds now.  rescore = false leaves that out: the rule is then wrong, and the tests show it.
    int searchAndFuseByRule(const std::vector<Corrected>& corrected, const std::vector<int>& loopPoints, float th, bool rescore = true)
    {
        std::vector<Hit> hits;
        std::vector<int> hitStart;
        dense(corrected, loopPoints, th, TH_LOW, hits, hitStart);
        std::set<int> survivors;
        int total = 0;
        rescored = 0;
        for (size_t t = 0; t < corrected.size(); t++) {
            const Corrected& c = corrected[t];
            std::vector<int> vpReplacePoints(loopPoints.size(), -1);
            const std::set<int> spAlreadyFound = getMapPoints(c.kf);
            int cur = hitStart[t];
            for (size_t i = 0; i < loopPoints.size(); i++) {
                const int mp = loopPoints[i];
                while (cur < hitStart[t + 1] && hits[cur].point < (int)i) cur++;
                if (mps[mp].bad || spAlreadyFound.count(mp)) continue;
                int bestIdx = -1;
                if (rescore && survivors.count(mp)) {
                    rescored++;
                    const Result r = search(c, mp, th);
                    if (r.status == FOUND && r.bestDist <= TH_LOW) bestIdx = r.bestIdx;
                } else if (cur < hitStart[t + 1] && hits[cur].point == (int)i) bestIdx = hits[cur].bestIdx;
                if (bestIdx < 0) continue;
                apply(c, mp, (int)i, bestIdx, vpReplacePoints);
                total++;
            }
            for (size_t i = 0; i < loopPoints.size(); i++)
                if (vpReplacePoints[i] >= 0) { replace(vpReplacePoints[i], loopPoints[i], (int)t); survivors.insert(loopPoints[i]); }
        }
        return total;
    }
};

}  // namespace loopfuse_ref
