// Tracking_hip.hpp -- drop-in for the body of Tracking::SearchLocalPoints (src/Tracking.cc:1206-1256), monocular, on
// liborbslamm_hip.so's map-point pool (include/orbslamm_mappool.h).  Header-only, C++11.
//
//   iORB_SLAM::SearchLocalPointsT<Frame, MapPoint>::Run(fs, slot, cap, pool, mCurrentFrame, mvpLocalMapPoints, idOf, opt);
//
// The frame lies in slot `slot` of the frame set (created with capacity `cap`), the local MapPoints in the pool under idOf(pMP) (the caller's accessor from
// MapPoint* to pool id; the pool's update rule is INTEGRATION.md's: orbw_pool_set when LocalMapping moves or re-describes a
// point, orbw_pool_set_flags when a point turns bad or gains its first observation).  Frame::isInFrustum for every local point
// and SearchByProjection(F, vpMapPoints, th) run on the device in one asynchronous call; what is serial in the function is
// replayed here on the host, in the reference's order, AFTER the device call has returned:
//   Tracking.cc:1209-1225   bad matches of the frame cleared, IncreaseVisible(1), mnLastFrameSeen, mbTrackInView = false
//   Tracking.cc:1230-1243   per local point not seen in this frame and not bad: mbTrackInView, IncreaseVisible(1), nToMatch
//   ORBmatcher.cc:123       F.mvpMapPoints[bestIdx] = pMP for the table's entries (nToMatch > 0 only)
// A refusal of the library throws std::runtime_error with everything as it came: no MapPoint and no slot of the frame has been
// touched.  mTrackProjX / mTrackProjY / mnTrackScaleLevel / mTrackViewCos stay on the device (nothing reads them after the
// search); mbTrackInView, which Tracking::TrackLocalMap's statistics do not read either, is kept as the reference leaves it.
//
// And for the body of Tracking::UpdateLocalMap (:1253-1261, UpdateLocalKeyFrames :1289-1397 + UpdateLocalPoints :1263-1286) on the
// keyframe store beside that pool (include/orbslamm_localmap.h):
//
//   iORB_SLAM::UpdateLocalMapT<Frame, KeyFrame, MapPoint>::SyncKeyFrame(store, pKF, idOfPoint, slotOfKF);      // LocalMapping's side
//   iORB_SLAM::UpdateLocalMapT<Frame, KeyFrame, MapPoint>::Run(store, mCurrentFrame, mvpLocalKeyFrames, mvpLocalMapPoints,
//                                                              mpReferenceKF, idOfPoint, slotOfKF, kfOfSlot, pointOfId);
//   iORB_SLAM::SearchLocalPointsT<Frame, MapPoint>::RunResident(fs, slot, cap, pool, store, mCurrentFrame, mvpLocalMapPoints, opt);
//
// slotOfKF is the DEFINED choice of the header: slot = mnId, which makes "ascending slot" the order of creation; the children
// go up ascending by mnId.  Run makes the device calls first and replays the host-visible effects afterwards, in the reference's
// order: the frame's bad matches nulled (:1306), the keyframes' and points' mnTrackReferenceForFrame (:1335, :1358, :1373, :1385,
// :1282), the two vectors, mpReferenceKF / F.mpReferenceKF (:1392-1396).  On ORBU_NO_VOTES the lists of keyframes stay (:1311) and
// UpdateLocalPoints runs over the old one (orbu_local_points).  A refusal throws with nothing touched.
//
// And for the line behind the search in Tracking::TrackWithMotionModel (:947-977) and Tracking::TrackLocalMap (:990-1023), monocular, on
// orbq_track_pose (include/orbslamm_trackpose.h): PoseOptimization from the pool, the resident frame and the search's own
// table, and the loop behind it.
//
//   iORB_SLAM::TrackWithMotionModelT<Frame, MapPoint>::Finish(h, fs, slot, pool, mCurrentFrame, mLastFrame.mvpMapPoints, mbOnlyTracking);
//   iORB_SLAM::TrackLocalMapT<Frame, KeyFrame, MapPoint>::Finish(h, fs, slot, pool, mCurrentFrame, baseIds, idOfPoint, verdict);
//   iORB_SLAM::TrackLocalMapT<Frame, KeyFrame, MapPoint>::Run(h, fs, slot, cap, pool, store, mCurrentFrame, mvpLocalKeyFrames,
//                                                             mvpLocalMapPoints, mpReferenceKF, idOfPoint, slotOfKF, kfOfSlot, pointOfId, opt);
//
//   iORB_SLAM::TrackReferenceKeyFrameT<Frame, KeyFrame, MapPoint>::Run(h, fs, kfSlot, slot, pool, store, kf, mCurrentFrame, mpReferenceKF,
//                                                                      mLastFrame.mTcw);            // Tracking.cc:802-844
//   iORB_SLAM::TrackWithMotionModelT<Frame, MapPoint>::Run(h, fs, curSlot, lastSlot, pool, mCurrentFrame, mLastFrame, mVelocity, idOfPoint,
//                                                          mbOnlyTracking);                         // Tracking.cc:917-978
//
// TrackWithMotionModelT::Finish stands behind orbw_track_frame_pose issued against (fs, slot) with mLastFrame's ids and `nmatches >= 20`
// (:944, the caller's, from orbm_track_results): it merges the table into mvpMapPoints (ORBmatcher.cc:1430), and writes back in the
// reference's order what PoseOptimization and :952-969 write: mvbOutlier, SetPose, the discarded slots, mbTrackInView and mnLastFrameSeen
// of the discarded points.  TrackLocalMapT::Finish stands behind SearchLocalPointsT::Run / RunResident, which has merged the table already:
// mvbOutlier, SetPose, IncreaseFound(1) on the inliers (:1000), mnMatchesInliers and the verdict of :1017-1023, the mnLastRelocFrameId rule
// applied from arguments.  Run composes UpdateLocalMapT::Run, SearchLocalPointsT::RunResident and Finish.  The counts come from the
// device (the pool's observed bit): the pool's update rule keeps it equal to Observations() > 0.  A refusal throws with the frame's pose,
// flags and points as the step before left them.
//
// And for Tracking::CreateInitialMapMonocular from its bundle adjustment on (:728-758), monocular, on orbb_initial_map
// (include/orbslamm_initmap.h): GlobalBundleAdjustemnt over the two keyframes, the median depth, the verdict of :734 and
// the rescaling in one device call.
//
//   iORB_SLAM::InitialMapT<KeyFrame, MapPoint>::Run(h, pKFini, pKFcur, pKFini->mnId == 0);          // Tracking.cc:728-758
//
// It flattens through the reference's members (GetPose, fx fy cx cy, mvKeysUn, mvInvLevelSigma2, mvScaleFactors, GetMapPointMatches,
// GetIndexInKeyFrame, GetWorldPos), makes ONE device call, and writes back in the reference's order: SetPose of both keyframes, then per
// point SetWorldPos and pMP->UpdateNormalAndDepth() (Optimizer.cc:214-258); with the verdict ORBB_OK the scaled SetPose of the current
// keyframe and the scaled SetWorldPos of every point (:745-757).  It returns the verdict: any other than ORBB_OK is the caller's Reset()
// (:737), which stays the caller's.  A refusal throws with nothing touched.
#pragma once

#include <algorithm>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class Frame, class MapPoint>
struct SearchLocalPointsT {
    struct Options {
        float nnratio = 0.8f;            // ORBmatcher matcher(0.8), Tracking.cc:1247
        int th = 1;                      // :1248-1253: 1, 3 for RGB-D, 5 shortly after a relocalisation
        float viewingCosLimit = 0.5f;    // :1238
        orbl_predict_fn predict = nullptr;   // the tree's own PredictScale where its log resolves to the double overload
    };
    struct Result { int nToMatch; int nmatches; };

    template <class IdOf>
    static Result Run(orbm_frameset_t* fs, int slot, int cap, orbw_pool_t* pool, Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, IdOf idOf,
                      const Options& opt = Options())
    {
        return Impl(fs, slot, cap, pool, nullptr, F, vpLocalMapPoints, idOf, opt);
    }

    // the same from the list UpdateLocalMapT::Run has just left on the device: vpLocalMapPoints is the mvpLocalMapPoints it wrote,
    // no id goes up.  The points that pass :1233 are, in order, the store's S; a list of another length is refused
    static Result RunResident(orbm_frameset_t* fs, int slot, int cap, orbw_pool_t* pool, orbu_store_t* store, Frame& F,
                              const std::vector<MapPoint*>& vpLocalMapPoints, const Options& opt = Options())
    {
        return Impl(fs, slot, cap, pool, store, F, vpLocalMapPoints, [](MapPoint*) { return 0; }, opt);
    }

    template <class IdOf>
    static Result Impl(orbm_frameset_t* fs, int slot, int cap, orbw_pool_t* pool, orbu_store_t* store, Frame& F,
                       const std::vector<MapPoint*>& vpLocalMapPoints, IdOf idOf, const Options& opt)
    {
        const char* who = "SearchLocalPoints(HIP): ";
        // ---- what the device needs, read without touching anything
        // the points :1209-1225 will stamp with this frame's id: they do not pass :1233
        std::unordered_set<MapPoint*> stamped;
        std::vector<uint8_t> occ(F.mvpMapPoints.size(), 0);
        for (size_t t = 0; t < F.mvpMapPoints.size(); t++) {
            MapPoint* pMP = F.mvpMapPoints[t];
            if (!pMP || pMP->isBad()) continue;
            stamped.insert(pMP);
            occ[t] = pMP->Observations() > 0 ? 1 : 0;   // ORBmatcher.cc:87-89
        }
        std::vector<MapPoint*> list;
        std::vector<int32_t> ids;
        list.reserve(vpLocalMapPoints.size()); ids.reserve(vpLocalMapPoints.size());
        for (size_t i = 0; i < vpLocalMapPoints.size(); i++) {
            MapPoint* pMP = vpLocalMapPoints[i];
            if (pMP->mnLastFrameSeen == F.mnId || stamped.count(pMP)) continue;   // :1233
            list.push_back(pMP); ids.push_back((int32_t)idOf(pMP));
        }
        OrbwView view;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) view.Rcw[3 * r + c] = F.mRcw.template at<float>(r, c);
            view.tcw[r] = F.mtcw.template at<float>(r, 0);
            view.Ow[r] = F.mOw.template at<float>(r, 0);
        }
        view.K[0] = Frame::fx; view.K[1] = Frame::fy; view.K[2] = Frame::cx; view.K[3] = Frame::cy;
        view.min_x = Frame::mnMinX; view.max_x = Frame::mnMaxX; view.min_y = Frame::mnMinY; view.max_y = Frame::mnMaxY;
        view.viewing_cos_limit = opt.viewingCosLimit;
        const int nlevels = (int)F.mvScaleFactors.size();
        std::vector<float> breaks((size_t)nlevels + 1);
        detail::check(orbl_level_breaks(F.mfLogScaleFactor, nlevels, opt.predict, breaks.data()), who);
        // ---- the device call
        OrbmProjParams pp;
        pp.mode = 3; pp.nnratio = opt.nnratio; pp.check_ori = 0; pp.th_dist = 100;   // TH_HIGH
        if ((int)occ.size() > cap) throw std::runtime_error(std::string(who) + "the frame holds more features than the frame set's capacity");
        occ.resize((size_t)cap, 0);   // (the library reads the occupancy of all `cap` features)
        if (store)
            detail::check(orbw_track_local_map_resident(fs, slot, pool, store, &pp, &view, (float)opt.th, F.mvScaleFactors.data(), breaks.data(),
                                                        nlevels, occ.data()), who);
        else
            detail::check(orbw_track_local_map(fs, slot, pool, &pp, &view, ids.data(), (int)ids.size(), (float)opt.th, F.mvScaleFactors.data(),
                                               breaks.data(), nlevels, occ.data()), who);
        const int32_t* assign = nullptr; const int32_t* nmatch = nullptr;
        int npairs = 0;
        detail::check(orbm_track_results(fs, 0, &assign, &nmatch, &npairs, nullptr), who);
        const uint8_t* status = nullptr;
        int nq = 0;
        detail::check(orbw_track_status(fs, 0, &status, &nq), who);
        if (nq != (int)list.size()) throw std::runtime_error(std::string(who) + "the store's resident list is not this frame's mvpLocalMapPoints");
        // ---- the replay, in the reference's order
        for (size_t t = 0; t < F.mvpMapPoints.size(); t++) {   // :1209-1225
            MapPoint* pMP = F.mvpMapPoints[t];
            if (!pMP) continue;
            if (pMP->isBad()) F.mvpMapPoints[t] = static_cast<MapPoint*>(NULL);
            else { pMP->IncreaseVisible(1); pMP->mnLastFrameSeen = F.mnId; pMP->mbTrackInView = false; }
        }
        Result res; res.nToMatch = 0; res.nmatches = 0;
        for (size_t k = 0; k < list.size(); k++) {   // :1230-1243
            if (status[k] == ORBW_ST_BAD) continue;   // :1235
            MapPoint* pMP = list[k];
            pMP->mbTrackInView = status[k] == ORBW_ST_IN_VIEW;   // Frame.cc:271, :317
            if (pMP->mbTrackInView) { pMP->IncreaseVisible(1); res.nToMatch++; }
        }
        if (res.nToMatch > 0) {   // :1245-1255
            for (size_t t = 0; t < F.mvpMapPoints.size(); t++)
                if (assign[t] >= 0) F.mvpMapPoints[t] = list[(size_t)assign[t]];   // ORBmatcher.cc:123
            res.nmatches = nmatch[0];
        }
        return res;
    }
};

template <class Frame, class KeyFrame, class MapPoint>
struct UpdateLocalMapT {
    struct Result { int status; int nkf; int nL; int nS; };

    // the keyframe's record into the store: GetMapPointMatches (ORBU_ENTRY_NO_VOTE where !pMP->IsInKeyFrame(pKF)),
    // GetBestCovisibilityKeyFrames(10), GetChilds ascending by mnId, GetParent, isBad.  Call it where LocalMapping has changed any
    // of them.
    // Returns the number of observations of the keyframe that have no match slot, AS FAR AS THE KEYFRAME SHOWS THEM: the points
    // that sit in one of its match slots and whose own observation of it (GetIndexInKeyFrame) names another slot, which does not
    // hold them.  An observing point that sits in NO match slot of the keyframe cannot be found from the keyframe (only a walk
    // over the map's points would find it) and is not counted; its vote is missing from the store.  0 outside races; reported,
    // not hidden.
    template <class IdOf, class SlotOf>
    static int SyncKeyFrame(orbu_store_t* store, KeyFrame* pKF, IdOf idOfPoint, SlotOf slotOfKF)
    {
        const char* who = "UpdateLocalMap(HIP) SyncKeyFrame: ";
        const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
        std::vector<int32_t> entries(vpMPs.size(), -1);
        int orphans = 0;
        for (size_t i = 0; i < vpMPs.size(); i++) {
            MapPoint* pMP = vpMPs[i];
            if (!pMP) continue;
            entries[i] = (int32_t)idOfPoint(pMP);
            if (!pMP->IsInKeyFrame(pKF)) entries[i] |= ORBU_ENTRY_NO_VOTE;
            else {
                const int idx = pMP->GetIndexInKeyFrame(pKF);
                if (idx != (int)i && (idx < 0 || idx >= (int)vpMPs.size() || vpMPs[(size_t)idx] != pMP)) orphans++;
            }
        }
        int32_t neigh[ORBU_MAX_NEIGHBOURS];
        for (int j = 0; j < ORBU_MAX_NEIGHBOURS; j++) neigh[j] = -1;
        const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(ORBU_MAX_NEIGHBOURS);
        for (size_t j = 0; j < vNeighs.size() && j < (size_t)ORBU_MAX_NEIGHBOURS; j++) neigh[j] = (int32_t)slotOfKF(vNeighs[j]);
        const std::set<KeyFrame*> spChilds = pKF->GetChilds();
        std::vector<std::pair<long unsigned int, int32_t> > byId;
        for (typename std::set<KeyFrame*>::const_iterator sit = spChilds.begin(); sit != spChilds.end(); sit++) byId.push_back(std::make_pair((*sit)->mnId, (int32_t)slotOfKF(*sit)));
        std::sort(byId.begin(), byId.end());
        std::vector<int32_t> children(byId.size());
        for (size_t c = 0; c < byId.size(); c++) children[c] = byId[c].second;
        KeyFrame* pParent = pKF->GetParent();
        const int32_t slot = (int32_t)slotOfKF(pKF), n = (int32_t)entries.size(), parent = pParent ? (int32_t)slotOfKF(pParent) : -1, nch = (int32_t)children.size();
        const uint8_t flags = pKF->isBad() ? ORBU_KF_BAD : 0;
        OrbuKeyFrames rec;
        rec.nkf = 1; rec.slot = &slot; rec.flags = &flags; rec.n = &n; rec.entries = entries.data(); rec.neigh = neigh; rec.parent = &parent;
        rec.nchildren = &nch; rec.children = children.data();
        detail::check(orbu_kf_set(store, &rec), who);
        return orphans;
    }

    template <class IdOf, class SlotOf, class KfOf, class PointOf>
    static Result Run(orbu_store_t* store, Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, std::vector<MapPoint*>& vpLocalMapPoints, KeyFrame*& pReferenceKF,
                      IdOf idOfPoint, SlotOf slotOfKF, KfOf kfOfSlot, PointOf pointOfId, int maxKeyFrames = 80)
    {
        const char* who = "UpdateLocalMap(HIP): ";
        // ---- the device calls, with nothing touched
        std::vector<int32_t> ids(F.mvpMapPoints.size(), -1);
        for (size_t i = 0; i < F.mvpMapPoints.size(); i++)
            if (F.mvpMapPoints[i]) ids[i] = (int32_t)idOfPoint(F.mvpMapPoints[i]);
        OrbuResult r;
        detail::check(orbu_update_local_map(store, ids.data(), (int)ids.size(), maxKeyFrames, &r), who);
        const bool noVotes = r.status == ORBU_NO_VOTES;
        if (noVotes) {   // :1311: the keyframe list stays; UpdateLocalPoints still runs over it (:1260)
            std::vector<int32_t> old(vpLocalKeyFrames.size());
            for (size_t j = 0; j < old.size(); j++) old[j] = (int32_t)slotOfKF(vpLocalKeyFrames[j]);
            detail::check(orbu_local_points(store, old.data(), (int)old.size(), ids.data(), (int)ids.size(), &r), who);
        }
        // ---- the replay, in the reference's order
        for (size_t i = 0; i < F.mvpMapPoints.size(); i++)   // :1295-1307
            if (F.mvpMapPoints[i] && F.mvpMapPoints[i]->isBad()) F.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
        if (!noVotes) {
            vpLocalKeyFrames.clear();   // :1317
            vpLocalKeyFrames.reserve((size_t)r.nkf);
            for (int j = 0; j < r.nkf; j++) {
                KeyFrame* pKF = kfOfSlot(r.kf[j]);
                vpLocalKeyFrames.push_back(pKF);
                pKF->mnTrackReferenceForFrame = F.mnId;
            }
            if (r.kf_max >= 0) {   // :1392-1396
                pReferenceKF = kfOfSlot(r.kf_max);
                F.mpReferenceKF = pReferenceKF;
            }
        }
        vpLocalMapPoints.clear();   // :1265
        vpLocalMapPoints.reserve((size_t)r.nL);
        for (int i = 0; i < r.nL; i++) {
            MapPoint* pMP = pointOfId(r.L[i]);
            vpLocalMapPoints.push_back(pMP);   // :1281
            pMP->mnTrackReferenceForFrame = F.mnId;   // :1282
        }
        Result res; res.status = noVotes ? ORBU_NO_VOTES : ORBU_OK; res.nkf = (int)vpLocalKeyFrames.size(); res.nL = r.nL; res.nS = r.nS;
        return res;
    }
};

namespace detail {

// mTcw and the camera of a frame as orbq_track_pose takes them
template <class Frame>
inline OrbqJob track_pose_job(orbm_frameset_t* fs, int slot, int back, const int32_t* baseIds, int discard, const Frame& F)
{
    OrbqJob J;
    J.fs = fs; J.slot = slot; J.back = back; J.base_ids = baseIds; J.n = F.N; J.discard = discard;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) J.frame.Tcw[4 * r + c] = F.mTcw.template at<float>(r, c);
    J.frame.K[0] = Frame::fx; J.frame.K[1] = Frame::fy; J.frame.K[2] = Frame::cx; J.frame.K[3] = Frame::cy;
    return J;
}

// Optimizer.cc:470: pFrame->SetPose(pose) -- reached only with 3 correspondences or more (:386)
template <class Frame>
inline void set_pose(Frame& F, const OrboResult& opt)
{
    if (opt.rounds <= 0) return;
    auto pose = F.mTcw.clone();
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = opt.Tcw[4 * r + c];
    F.SetPose(pose);
}

}  // namespace detail

template <class Frame, class MapPoint>
struct TrackWithMotionModelT {
    struct Result { bool ok; bool vo; int nmatches; int nmatchesMap; OrboResult opt; };

    // vpLastMapPoints: mLastFrame.mvpMapPoints, the queries of the search (orbw_track_frame_pose's last_ids are their pool ids);
    // back: which of the set's last searches that was.  result.vo is mbVO as :973 would set it (meaningful under onlyTracking)
    static Result Finish(orbm_t* h, orbm_frameset_t* fs, int slot, orbw_pool_t* pool, Frame& F, const std::vector<MapPoint*>& vpLastMapPoints,
                         bool onlyTracking, int back = 0)
    {
        const char* who = "TrackWithMotionModel(HIP): ";
        const int32_t* assign = nullptr;
        detail::check(orbm_track_results(fs, back, &assign, nullptr, nullptr, nullptr), who);
        const int N = F.N;
        for (int t = 0; t < N; t++)
            if (assign[t] >= (int)vpLastMapPoints.size()) throw std::runtime_error(std::string(who) + "the search's table names a query the list does not hold");
        const OrbqJob J = detail::track_pose_job(fs, slot, back, nullptr, 1, F);
        OrbqResult r;
        std::vector<int32_t> ids((size_t)N + 1);
        std::vector<uint8_t> outlier((size_t)N + 1);
        int32_t* pi = ids.data(); uint8_t* po = outlier.data();
        detail::check(orbq_track_pose(h, pool, &J, 1, F.mvInvLevelSigma2.data(), (int)F.mvInvLevelSigma2.size(), &r, &pi, &po), who);
        // the device merged the table into NULLs (:940's fill) and discarded the outliers: the frame must have been filled with NULL
        // before the search, and the ids that come back must be the table's matches without the flagged ones
        for (int t = 0; t < N; t++) {
            if (assign[t] < 0 && F.mvpMapPoints[t]) throw std::runtime_error(std::string(who) + "mvpMapPoints was not filled with NULL before the search (Tracking.cc:940)");
            if ((ids[t] >= 0) != (assign[t] >= 0 && !outlier[t]) || (outlier[t] && assign[t] < 0))
                throw std::runtime_error(std::string(who) + "the ids returned are not the search's matches without the outliers");
        }
        // ---- the replay, in the reference's order
        for (int t = 0; t < N; t++)
            if (assign[t] >= 0) F.mvpMapPoints[t] = vpLastMapPoints[(size_t)assign[t]];   // ORBmatcher.cc:1430
        for (int i = 0; i < N; i++)
            if (F.mvpMapPoints[i]) F.mvbOutlier[i] = outlier[i] != 0;   // Optimizer.cc:310, :410, :416
        detail::set_pose(F, r.opt);   // :470
        for (int i = 0; i < N; i++) {   // Tracking.cc:952-969
            if (!F.mvpMapPoints[i] || !F.mvbOutlier[i]) continue;
            MapPoint* pMP = F.mvpMapPoints[i];
            F.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
            F.mvbOutlier[i] = false;
            pMP->mbTrackInView = false;
            pMP->mnLastFrameSeen = F.mnId;
        }
        Result res;
        res.opt = r.opt; res.nmatches = r.n_matches; res.nmatchesMap = r.n_matches_map;
        res.vo = r.n_matches_map < 10;                                          // :973
        res.ok = onlyTracking ? r.n_matches > 20 : r.n_matches_map >= 10;       // :974, :977
        return res;
    }

    // Tracking::TrackWithMotionModel (Tracking.cc:917-978, monocular) behind UpdateLastFrame (:923, the caller's) on
    // orbq_track_motion_model (include/orbslamm_motion.h): the pose product, the search, its retry with 2 * th, the gate,
    // PoseOptimization and the discard loop in ONE call.  The current frame lies in curSlot and mLastFrame in lastSlot of fs, the last
    // frame's points in the pool under idOfPoint(pMP).  Run makes the device call first and replays the host-visible effects afterwards,
    // in the reference's order.  A refusal throws with the frame untouched.
    struct RunOptions {
        float th = 15.f;          // :932
        int minMatches = 20;      // :938, :944
        bool checkOri = true;     // ORBmatcher matcher(0.9,true), :919
    };
    // status, wide, nSearch: as OrbqMotionResult; nmatches is the reference's counter at :971 (the count of the search that stands less
    // the discarded outliers), nmatchesMap that of :967; vo is mbVO as :973 would set it (meaningful under onlyTracking)
    struct RunResult { bool ok; bool vo; int status; bool wide; int nSearch[2]; int nmatches; int nmatchesMap; OrboResult opt; };

    template <class MatT, class IdOf>
    static RunResult Run(orbm_t* h, orbm_frameset_t* fs, int curSlot, int lastSlot, orbw_pool_t* pool, Frame& F, const Frame& L, const MatT& velocity,
                         IdOf idOfPoint, bool onlyTracking, const RunOptions& o = RunOptions())
    {
        const char* who = "TrackWithMotionModel(HIP): ";
        const int N = F.N, NQ = L.N;
        std::vector<int32_t> lastIds((size_t)NQ + 1, -1);
        for (int i = 0; i < NQ; i++)   // ORBmatcher.cc:1355-1359
            if (L.mvpMapPoints[i] && !L.mvbOutlier[i]) lastIds[(size_t)i] = (int32_t)idOfPoint(L.mvpMapPoints[i]);
        OrbqMotionJob J;
        J.fs = fs; J.cur_slot = curSlot; J.last_slot = lastSlot; J.n = N; J.nq = NQ; J.last_ids = lastIds.data();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) { J.velocity[4 * r + c] = velocity.template at<float>(r, c); J.last_Tcw[4 * r + c] = L.mTcw.template at<float>(r, c); }
        J.K[0] = Frame::fx; J.K[1] = Frame::fy; J.K[2] = Frame::cx; J.K[3] = Frame::cy;
        OrbqMotionResult r;
        std::vector<int32_t> ids((size_t)N + 1), assign((size_t)N + 1);
        std::vector<uint8_t> outlier((size_t)N + 1);
        int32_t* pi = ids.data(); uint8_t* po = outlier.data(); int32_t* pa = assign.data();
        detail::check(orbq_track_motion_model(h, pool, &J, 1, o.th, o.minMatches, o.checkOri ? 1 : 0, F.mvInvLevelSigma2.data(), F.mvScaleFactors.data(),
                                              (int)F.mvInvLevelSigma2.size(), &r, &pi, &po, &pa, nullptr), who);
        int nDiscarded = 0;
        for (int t = 0; t < N; t++) {
            if (assign[t] >= NQ || (assign[t] >= 0 && lastIds[(size_t)assign[t]] < 0))
                throw std::runtime_error(std::string(who) + "the table names a last-frame feature without a MapPoint");
            if ((ids[t] >= 0) != (assign[t] >= 0 && !outlier[t]) || (outlier[t] && assign[t] < 0))
                throw std::runtime_error(std::string(who) + "the ids returned are not the search's matches without the outliers");
            nDiscarded += outlier[t] ? 1 : 0;
        }
        // ---- the replay, in the reference's order
        auto pose = velocity.clone();
        for (int rr = 0; rr < 4; rr++) for (int c = 0; c < 4; c++) pose.template at<float>(rr, c) = r.Tcw_pred[4 * rr + c];
        F.SetPose(pose);   // :925
        std::fill(F.mvpMapPoints.begin(), F.mvpMapPoints.end(), static_cast<MapPoint*>(NULL));   // :927 (and :940)
        for (int t = 0; t < N; t++)
            if (assign[t] >= 0) F.mvpMapPoints[t] = L.mvpMapPoints[(size_t)assign[t]];   // ORBmatcher.cc:1430, behind the pruning of :1464
        RunResult res;
        res.status = r.status; res.wide = r.wide != 0; res.nSearch[0] = r.n_search[0]; res.nSearch[1] = r.n_search[1];
        res.nmatches = r.n_search[r.wide ? 1 : 0]; res.nmatchesMap = 0; res.opt = r.track.opt;
        res.ok = false; res.vo = false;
        if (r.status == ORBQ_MM_TOO_FEW) return res;   // :944-945: the frame keeps the predicted pose and the matches
        for (int i = 0; i < N; i++)
            if (F.mvpMapPoints[i]) F.mvbOutlier[i] = outlier[i] != 0;   // Optimizer.cc:310, :410, :416
        detail::set_pose(F, r.track.opt);   // :470
        for (int i = 0; i < N; i++) {   // Tracking.cc:952-969
            if (!F.mvpMapPoints[i] || !F.mvbOutlier[i]) continue;
            MapPoint* pMP = F.mvpMapPoints[i];
            F.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
            F.mvbOutlier[i] = false;
            pMP->mbTrackInView = false;
            pMP->mnLastFrameSeen = F.mnId;
        }
        res.nmatches -= nDiscarded;                                                   // :964
        res.nmatchesMap = r.track.n_matches_map;                                      // :967
        res.vo = res.nmatchesMap < 10;                                                // :973
        res.ok = onlyTracking ? res.nmatches > 20 : res.nmatchesMap >= 10;            // :974, :977
        return res;
    }
};

template <class Frame, class KeyFrame, class MapPoint>
struct TrackLocalMapT {
    struct Verdict {
        bool onlyTracking = false;                 // mbOnlyTracking
        long unsigned int lastRelocFrameId = 0;    // mnLastRelocFrameId
        int maxFrames = 30;                        // mMaxFrames
    };
    struct Options {
        Verdict verdict;
        typename SearchLocalPointsT<Frame, MapPoint>::Options search;
        int maxKeyFrames = 80;
    };
    struct Result { bool ok; int nMatchesInliers; int nMatches; int nMatchesMap; OrboResult opt; };

    // baseIds[t]: the pool id of mvpMapPoints[t] as the search was issued (-1 = NULL), F.N of them; F.mvpMapPoints holds the search's
    // matches already (SearchLocalPointsT's replay); back: which of the set's last searches that was
    template <class IdOf>
    static Result Finish(orbm_t* h, orbm_frameset_t* fs, int slot, orbw_pool_t* pool, Frame& F, const std::vector<int32_t>& baseIds, IdOf idOfPoint,
                         const Verdict& v = Verdict(), int back = 0)
    {
        const char* who = "TrackLocalMap(HIP): ";
        const int N = F.N;
        if ((int)baseIds.size() < N) throw std::runtime_error(std::string(who) + "fewer ids than the frame has features");
        const OrbqJob J = detail::track_pose_job(fs, slot, back, baseIds.data(), 0, F);
        OrbqResult r;
        std::vector<int32_t> ids((size_t)N + 1);
        std::vector<uint8_t> outlier((size_t)N + 1);
        int32_t* pi = ids.data(); uint8_t* po = outlier.data();
        detail::check(orbq_track_pose(h, pool, &J, 1, F.mvInvLevelSigma2.data(), (int)F.mvInvLevelSigma2.size(), &r, &pi, &po), who);
        for (int i = 0; i < N; i++)
            if ((F.mvpMapPoints[i] ? (int32_t)idOfPoint(F.mvpMapPoints[i]) : -1) != ids[i])
                throw std::runtime_error(std::string(who) + "the frame's points are not the merge of baseIds and that search");
        // ---- the replay, in the reference's order
        for (int i = 0; i < N; i++)
            if (F.mvpMapPoints[i]) F.mvbOutlier[i] = outlier[i] != 0;   // Optimizer.cc:310, :410, :416
        detail::set_pose(F, r.opt);   // :470
        for (int i = 0; i < N; i++)   // Tracking.cc:994-1013
            if (F.mvpMapPoints[i] && !F.mvbOutlier[i]) F.mvpMapPoints[i]->IncreaseFound(1);
        Result res;
        res.opt = r.opt; res.nMatches = r.n_matches; res.nMatchesMap = r.n_matches_map;
        res.nMatchesInliers = v.onlyTracking ? r.n_matches : r.n_matches_map;   // :1001-1007
        res.ok = !(F.mnId < v.lastRelocFrameId + (long unsigned int)v.maxFrames && res.nMatchesInliers < 50) && !(res.nMatchesInliers < 20);   // :1017-1023
        return res;
    }

    // Tracking::TrackLocalMap: UpdateLocalMap, SearchLocalPoints from the list the update left on the device, PoseOptimization, the verdict
    template <class IdOf, class SlotOf, class KfOf, class PointOf>
    static Result Run(orbm_t* h, orbm_frameset_t* fs, int slot, int cap, orbw_pool_t* pool, orbu_store_t* store, Frame& F,
                      std::vector<KeyFrame*>& vpLocalKeyFrames, std::vector<MapPoint*>& vpLocalMapPoints, KeyFrame*& pReferenceKF, IdOf idOfPoint,
                      SlotOf slotOfKF, KfOf kfOfSlot, PointOf pointOfId, const Options& opt = Options())
    {
        UpdateLocalMapT<Frame, KeyFrame, MapPoint>::Run(store, F, vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF, idOfPoint, slotOfKF, kfOfSlot, pointOfId,
                                                        opt.maxKeyFrames);   // :985
        std::vector<int32_t> baseIds((size_t)F.N, -1);   // (the update's replay has nulled the bad matches: what is left is what the search sees)
        for (int i = 0; i < F.N; i++)
            if (F.mvpMapPoints[i]) baseIds[(size_t)i] = (int32_t)idOfPoint(F.mvpMapPoints[i]);
        SearchLocalPointsT<Frame, MapPoint>::RunResident(fs, slot, cap, pool, store, F, vpLocalMapPoints, opt.search);   // :987
        return Finish(h, fs, slot, pool, F, baseIds, idOfPoint, opt.verdict);   // :990-1023
    }
};

// Tracking::TrackReferenceKeyFrame (Tracking.cc:802-844, monocular) on orbq_track_reference (include/orbslamm_trackpose.h, DESIGN.md
// §8t): SearchByBoW with the validity rule, the merge, the gate, PoseOptimization and the discard loop in ONE call.  The caller has the
// current frame in `slot` and pReferenceKF in `kfSlot` of fs with orbm_frameset_compute_bow run on both (:805 ComputeBoW), the
// keyframe's match list in slot `kf` of the store (UpdateLocalMapT::SyncKeyFrame) and its points in the pool.  Run makes the device
// call first and replays the host-visible effects afterwards, in the reference's order; on ORBQ_REF_TOO_FEW (:814) it returns false
// and writes nothing to the frame.  A refusal throws with nothing touched.
template <class Frame, class KeyFrame, class MapPoint>
struct TrackReferenceKeyFrameT {
    struct Options {
        float nnratio = 0.7f;     // ORBmatcher matcher(0.7,true), :808
        bool checkOri = true;
        int minMatches = 15;      // :814
    };
    struct Result { bool ok; int status; int nBow; int nmatches; int nmatchesMap; OrboResult opt; };

    // lastTcw: mLastFrame.mTcw (:818)
    template <class MatT>
    static Result Run(orbm_t* h, orbm_frameset_t* fs, int kfSlot, int slot, orbw_pool_t* pool, orbu_store_t* store, int kf, Frame& F, KeyFrame* pKF,
                      const MatT& lastTcw, const Options& o = Options())
    {
        const char* who = "TrackReferenceKeyFrame(HIP): ";
        const int N = F.N;
        OrbqRefJob J;
        J.fs = fs; J.kf_slot = kfSlot; J.slot = slot; J.kf = kf; J.n = N; J.solve = 1;
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) J.frame.Tcw[4 * r + c] = lastTcw.template at<float>(r, c);
        J.frame.K[0] = Frame::fx; J.frame.K[1] = Frame::fy; J.frame.K[2] = Frame::cx; J.frame.K[3] = Frame::cy;
        OrbqRefResult r;
        std::vector<int32_t> ids((size_t)N + 1), match((size_t)N + 1);
        std::vector<uint8_t> outlier((size_t)N + 1);
        int32_t* pi = ids.data(); uint8_t* po = outlier.data(); int32_t* pm = match.data();
        detail::check(orbq_track_reference(h, pool, store, &J, 1, o.nnratio, o.checkOri ? 1 : 0, o.minMatches, F.mvInvLevelSigma2.data(),
                                           (int)F.mvInvLevelSigma2.size(), &r, &pi, &po, &pm), who);
        Result res;
        res.status = r.status; res.nBow = r.n_bow; res.nmatches = r.track.n_matches; res.nmatchesMap = r.track.n_matches_map; res.opt = r.track.opt;
        res.ok = false;
        if (r.status == ORBQ_REF_TOO_FEW) return res;   // :814-815: before the frame is touched
        // the pointers are the keyframe's own (ORBmatcher.cc:187 vpMapPointsKF = pKF->GetMapPointMatches(), :236)
        const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
        for (int t = 0; t < N; t++) {
            if (match[t] >= (int)vpMapPointsKF.size() || (match[t] >= 0 && !vpMapPointsKF[(size_t)match[t]]))
                throw std::runtime_error(std::string(who) + "the table names a keyframe feature without a MapPoint: the store is behind the keyframe");
            if ((ids[t] >= 0) != (match[t] >= 0 && !outlier[t]) || (outlier[t] && match[t] < 0))
                throw std::runtime_error(std::string(who) + "the ids returned are not the search's matches without the outliers");
        }
        // ---- the replay, in the reference's order
        for (int t = 0; t < N; t++)   // :817 mCurrentFrame.mvpMapPoints = vpMapPointMatches
            F.mvpMapPoints[t] = match[t] >= 0 ? vpMapPointsKF[(size_t)match[t]] : static_cast<MapPoint*>(NULL);
        F.SetPose(lastTcw);   // :818
        for (int i = 0; i < N; i++)
            if (F.mvpMapPoints[i]) F.mvbOutlier[i] = outlier[i] != 0;   // Optimizer.cc:310, :410, :416
        detail::set_pose(F, r.track.opt);   // :470
        for (int i = 0; i < N; i++) {   // Tracking.cc:824-841
            if (!F.mvpMapPoints[i] || !F.mvbOutlier[i]) continue;
            MapPoint* pMP = F.mvpMapPoints[i];
            F.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
            F.mvbOutlier[i] = false;
            pMP->mbTrackInView = false;
            pMP->mnLastFrameSeen = F.mnId;
        }
        res.ok = r.track.n_matches_map >= 10;   // :843
        return res;
    }
};

// Tracking::CreateInitialMapMonocular from its bundle adjustment on (:728-758)
template <class KeyFrame, class MapPoint>
struct InitialMapT {
    struct Result { int verdict; float medianDepth, invMedianDepth; OrbbResult ba; };

    static Result Run(orbm_t* h, KeyFrame* pKFini, KeyFrame* pKFcur, bool fixedFirst, int nIterations = 20, bool bRobust = true)
    {
        typedef typename std::decay<decltype(pKFini->GetPose())>::type Mat;
        const Mat T1 = pKFini->GetPose(), T2 = pKFcur->GetPose();
        OrbbProblem pr;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { pr.Tcw1[4 * r + c] = T1.template at<float>(r, c); pr.Tcw2[4 * r + c] = T2.template at<float>(r, c); }
        pr.K[0] = pKFini->fx; pr.K[1] = pKFini->fy; pr.K[2] = pKFini->cx; pr.K[3] = pKFini->cy;
        pr.fixed_first = fixedFirst ? 1 : 0; pr.fixed_second = 0; pr.iterations = nIterations; pr.robust = bRobust ? 1 : 0;
        const std::vector<MapPoint*> vpMP = pKFini->GetMapPointMatches();   // :750: one point per matched feature of the initial frame
        pr.n1 = (int)vpMP.size(); pr.n2 = (int)pKFcur->mvKeysUn.size();
        std::vector<OrbxKeyPoint> keys[2];
        KeyFrame* kfs[2] = {pKFini, pKFcur};
        for (int s = 0; s < 2; s++) {
            keys[s].resize(kfs[s]->mvKeysUn.size());
            for (size_t i = 0; i < keys[s].size(); i++) {
                OrbxKeyPoint k = {kfs[s]->mvKeysUn[i].pt.x, kfs[s]->mvKeysUn[i].pt.y, kfs[s]->mvKeysUn[i].size, kfs[s]->mvKeysUn[i].angle,
                                  kfs[s]->mvKeysUn[i].response, kfs[s]->mvKeysUn[i].octave, kfs[s]->mvKeysUn[i].class_id};
                keys[s][i] = k;
            }
        }
        std::vector<int32_t> matches12(vpMP.size(), -1);
        std::vector<float> P3D(3 * vpMP.size(), 0.f);
        for (size_t i = 0; i < vpMP.size(); i++) {
            MapPoint* pMP = vpMP[i];
            if (!pMP || pMP->isBad()) continue;
            matches12[i] = pMP->GetIndexInKeyFrame(pKFcur);
            const Mat X = pMP->GetWorldPos();
            for (int c = 0; c < 3; c++) P3D[3 * i + c] = X.template at<float>(c, 0);
        }
        std::vector<OrbbPoint> points(vpMP.size() ? vpMP.size() : 1);
        const OrbxKeyPoint* k1 = keys[0].data();
        const OrbxKeyPoint* k2 = keys[1].data();
        const int32_t* m12 = matches12.data();
        const float* p3d = P3D.data();
        OrbbPoint* pts = points.data();
        Result res;
        detail::check(orbb_initial_map(h, &pr, 1, &k1, &k2, &m12, &p3d, pKFini->mvInvLevelSigma2.data(), pKFini->mvScaleFactors.data(),
                               (int)pKFini->mvScaleFactors.size(), &res.ba, &pts), "InitialMap(HIP): ");
        res.verdict = res.ba.verdict; res.medianDepth = res.ba.median_depth; res.invMedianDepth = res.ba.inv_median_depth;
        // Optimizer.cc:214-258: the keyframes, then the points
        const float last[4] = {0.f, 0.f, 0.f, 1.f};
        float T[16];
        for (int i = 0; i < 12; i++) T[i] = res.ba.Tcw1[i];
        for (int i = 0; i < 4; i++) T[12 + i] = last[i];
        pKFini->SetPose(detail::mat32f<Mat>(T, 4, 4));
        for (int i = 0; i < 12; i++) T[i] = res.ba.Tcw2[i];
        pKFcur->SetPose(detail::mat32f<Mat>(T, 4, 4));
        for (size_t i = 0; i < vpMP.size(); i++) {
            if (!points[i].matched) continue;
            vpMP[i]->SetWorldPos(detail::mat32f<Mat>(points[i].pos, 3, 1));
            vpMP[i]->UpdateNormalAndDepth();
        }
        if (res.verdict != ORBB_OK) return res;   // :734-739: the caller's Reset()
        // :745-757
        for (int i = 0; i < 12; i++) T[i] = res.ba.Tcw2_scaled[i];
        pKFcur->SetPose(detail::mat32f<Mat>(T, 4, 4));
        for (size_t i = 0; i < vpMP.size(); i++)
            if (points[i].matched) vpMP[i]->SetWorldPos(detail::mat32f<Mat>(points[i].pos_scaled, 3, 1));
        return res;
    }
};

}  // namespace iORB_SLAM
