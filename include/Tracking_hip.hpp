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
#pragma once

#include <cstdint>
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
        detail::check(orbw_track_local_map(fs, slot, pool, &pp, &view, ids.data(), (int)ids.size(), (float)opt.th, F.mvScaleFactors.data(),
                                           breaks.data(), nlevels, occ.data()), who);
        const int32_t* assign = nullptr; const int32_t* nmatch = nullptr;
        int npairs = 0;
        detail::check(orbm_track_results(fs, 0, &assign, &nmatch, &npairs, nullptr), who);
        const uint8_t* status = nullptr;
        int nq = 0;
        detail::check(orbw_track_status(fs, 0, &status, &nq), who);
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

}  // namespace iORB_SLAM
