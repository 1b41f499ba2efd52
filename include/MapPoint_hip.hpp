// MapPoint_hip.hpp -- drop-in for MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
// MapPoint::UpdateNormalAndDepth (:330-371), batched, on liborbslamm_hip.so's refresh block (include/orbslamm_refresh.h,
// DESIGN.md §8w) over the keyframe store (include/orbslamm_localmap.h).  Header-only, C++11.
//
//   iORB_SLAM::RefreshMapPointsT<KeyFrame, MapPoint>::Run(store, points, what, moved, scaleFactors, hooks);
//
// replaces a loop of pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); over `points` (LocalMapping.cc:152-153,
// :442-444, :526-527; Optimizer.cc:250, :799, :1065, :1344; LoopClosing.cc:511, :543) by ONE device call that refreshes the
// pool's records in place, and then writes mDescriptor, mNormalVector, mfMinDistance and mfMaxDistance of each host MapPoint.
// what: ORBR_DESCRIPTOR | ORBR_NORMAL_DEPTH.  moved: the points' positions changed since the pool last saw them (SetWorldPos in
// front of the refresh): 12 bytes a point go up and are committed for every point, bad ones included.
// The store must hold, for every set keyframe: the match slots as UpdateLocalMapT::SyncKeyFrame (include/Tracking_hip.hpp)
// leaves them, and for the halves asked the descriptors (orbu_kf_set_descriptors*), the camera centre (orbu_kf_set_centres) and
// the octaves (orbu_kf_set_octaves) as they are NOW.  Slot = mnId is the DEFINED choice of the headers: where the reference
// iterates map<KeyFrame*,size_t> in heap-address order, the device takes the observations in ascending slot.
// `hooks` is the caller's object (the members it writes are protected in the reference):
//   int32_t IdOfPoint(MapPoint*)            the pool id (as the other drop-ins' idOfPoint)
//   int32_t SlotOfKF(KeyFrame*)             the store slot
//   void WorldPos(MapPoint*, float[3])      mWorldPos
//   void SetDescriptor(MapPoint*, const uint8_t[32])                                  mDescriptor = the winner's row (:305)
//   void SetNormalAndDepth(MapPoint*, const float normal[3], float minD, float maxD)  :367-369
// A half whose status is not ORBR_ST_DONE leaves the host point as the member leaves it: untouched.  ORBR_ST_NO_REF and
// ORBR_ST_LEVEL_RANGE, where the reference is undefined, are counted in the result.  A refusal of the library throws
// std::runtime_error with every point as it came.
#pragma once

#include <cstdint>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class KeyFrame, class MapPoint>
struct RefreshMapPointsT {
    struct Result {
        int nDescriptors, nNormals;      // halves that were DONE and written to the host points
        int nUndefined;                  // ORBR_ST_NO_REF + ORBR_ST_LEVEL_RANGE
        std::vector<OrbrPoint> records;  // one per point, in the order given
    };

    template <class Hooks>
    static Result Run(orbu_store_t* store, const std::vector<MapPoint*>& points, int what, bool moved, const std::vector<float>& scaleFactors, Hooks& hooks)
    {
        const char* who = "RefreshMapPoints(HIP): ";
        Result res; res.nDescriptors = 0; res.nNormals = 0; res.nUndefined = 0;
        const size_t n = points.size();
        if (!n) return res;
        // ---- the device call, with nothing touched
        std::vector<int32_t> ids(n), ref(n);
        std::vector<float> pos;
        if (moved) pos.resize(3 * n);
        for (size_t i = 0; i < n; i++) {
            MapPoint* pMP = points[i];
            ids[i] = hooks.IdOfPoint(pMP);
            KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
            ref[i] = pRefKF ? hooks.SlotOfKF(pRefKF) : -1;
            if (moved) hooks.WorldPos(pMP, &pos[3 * i]);
        }
        res.records.resize(n);
        detail::check(orbr_refresh_points(store, ids.data(), ref.data(), moved ? pos.data() : nullptr, (int)n, what, scaleFactors.data(), (int)scaleFactors.size(), 1,
                                          res.records.data()), who);
        // ---- the host points
        for (size_t i = 0; i < n; i++) {
            const OrbrPoint& r = res.records[i];
            if (r.st_descriptor == ORBR_ST_DONE) { hooks.SetDescriptor(points[i], r.desc); res.nDescriptors++; }
            if (r.st_normal_depth == ORBR_ST_DONE) { hooks.SetNormalAndDepth(points[i], r.normal, r.min_distance, r.max_distance); res.nNormals++; }
            if (r.st_normal_depth == ORBR_ST_NO_REF || r.st_normal_depth == ORBR_ST_LEVEL_RANGE) res.nUndefined++;
        }
        return res;
    }
};

}  // namespace iORB_SLAM
