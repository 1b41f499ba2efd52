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
#pragma once

#include <algorithm>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
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

}  // namespace iORB_SLAM
