// LocalMapping_hip.hpp -- the reference's LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452 of both scenarios,
// monocular) over the C ABI of liborbslamm_hip.so (orbl_*).  Header-only, C++11.
//
//   CreateNewMapPointsT<KeyFrame, MapPoint, Map, Mat>::Run(pKF, pMap, recent, checkNewKeyFrames)
//       the drop-in for the body of CreateNewMapPoints.  In the reference tree:
//           typedef iORB_SLAM::CreateNewMapPointsT<KeyFrame, MapPoint, Map, cv::Mat> NewPoints;
//           void LocalMapping::CreateNewMapPoints()
//           { NewPoints::Run(mpCurrentKeyFrame, mpMap, mlpRecentAddedMapPoints, [this] { return CheckNewKeyFrames(); }); }
//       It flattens the current keyframe and GetBestCovisibilityKeyFrames(20), computes ComputeSceneMedianDepth(2) of every
//       neighbour on the host (the reference's own member: it reads MapPoint positions from the object graph), makes ONE
//       device call (orbl_create_new_map_points: the search against all neighbours, the triangulation, the gates) and
//       replays the result in the reference's order: new MapPoint, both AddObservation, both AddMapPoint, the point's own
//       ComputeDistinctiveDescriptors and UpdateNormalAndDepth, mpMap->AddMapPoint, the recent-points list.
//       The reference's `if(i>0 && CheckNewKeyFrames()) return;` is honoured at replay: the predicate is polled before the
//       first record of each neighbour i > 0 that holds records -- and, as in the reference, before every other neighbour i > 0
//       in between -- and on true the remaining records are dropped: the map then sees exactly what the early return leaves.
//   Monocular only (mbMonocular == true; no mvuRight is read).  It is a template so that it compiles (and is tested,
//   tests/cpp/newpoints_dropin_gpu.cpp) without OpenCV: Mat needs a (rows, cols, type) constructor and at<float>(r, c);
//   the keyframe's mDescriptors needs ptr<unsigned char>(row).
//   Every call runs on the calling thread's matcher handle (orbm_thread_handle), as the other drop-ins do.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class KeyFrame, class MapPoint, class Map, class Mat>
class CreateNewMapPointsT {
public:
    static const int kNeighbours = 20;   // nn = 20 when mbMonocular (:210-213)

    // Returns nnew.  status (optional): the n_neighbours x N table of ORBL_ST_* codes; neighbours (optional): vpNeighKFs.
    template <class RecentList, class Pred>
    static int Run(KeyFrame* pKF1, Map* pMap, RecentList& recent, Pred checkNewKeyFrames, int device = 0, std::vector<uint8_t>* status = nullptr,
                   std::vector<KeyFrame*>* neighbours = nullptr)
    {
        const std::vector<KeyFrame*> vpNeighKFs = pKF1->GetBestCovisibilityKeyFrames(kNeighbours);
        if (neighbours) *neighbours = vpNeighKFs;
        const int K = (int)vpNeighKFs.size();
        if (K > ORBL_MAX_NEIGHBOURS) throw std::runtime_error("CreateNewMapPoints: more neighbours than ORBL_MAX_NEIGHBOURS");
        Side cur;
        flatten(pKF1, cur);
        std::vector<Side> nb((size_t)K);
        std::vector<OrblKeyFrame> kf2((size_t)K);
        std::vector<const OrbxKeyPoint*> keys2((size_t)K);
        std::vector<const uint8_t*> desc2((size_t)K), skip2((size_t)K);
        std::vector<int32_t> n2((size_t)K);
        std::vector<OrbmFeatVec> fv2((size_t)K);
        for (int k = 0; k < K; k++) {
            flatten(vpNeighKFs[k], nb[k]);
            nb[k].kf.median_depth = vpNeighKFs[k]->ComputeSceneMedianDepth(2);
            kf2[k] = nb[k].kf;
            keys2[k] = nb[k].keys.data(); desc2[k] = nb[k].desc.data(); skip2[k] = nb[k].skip.data(); n2[k] = nb[k].n; fv2[k] = nb[k].fv();
        }
        const OrbmFeatVec fv1 = cur.fv();
        std::vector<OrblNewPoint> out((size_t)cur.n);
        if (status) status->assign((size_t)K * cur.n, 0);
        int nOut = 0;
        orbm_t* h = nullptr;
        check(orbm_thread_handle(device, &h));
        check(orbl_create_new_map_points(h, cur.keys.data(), cur.desc.data(), cur.n, &fv1, cur.skip.data(), &cur.kf, keys2.data(), desc2.data(), n2.data(),
                                         fv2.data(), skip2.data(), kf2.data(), K, pKF1->mvScaleFactors.data(), pKF1->mvLevelSigma2.data(),
                                         (int)pKF1->mvScaleFactors.size(), pKF1->mfScaleFactor, 0, out.data(), cur.n, &nOut,
                                         status && !status->empty() ? status->data() : nullptr, nullptr));
        // the replay: neighbours in order, the early return where the reference has it
        int nnew = 0, r = 0;
        for (int i = 0; i < K; i++) {
            if (i > 0 && checkNewKeyFrames()) return nnew;
            KeyFrame* pKF2 = vpNeighKFs[i];
            for (; r < nOut && out[r].neighbour == i; r++) {
                const OrblNewPoint& p = out[r];
                Mat x3D = detail::mat32f<Mat>(p.pos, 3, 1);
                MapPoint* pMP = new MapPoint(x3D, pKF1, pMap);
                pMP->AddObservation(pKF1, p.idx1);
                pMP->AddObservation(pKF2, p.idx2);
                pKF1->AddMapPoint(pMP, p.idx1);
                pKF2->AddMapPoint(pMP, p.idx2);
                pMP->ComputeDistinctiveDescriptors();
                pMP->UpdateNormalAndDepth();
                pMap->AddMapPoint(pMP);
                recent.push_back(pMP);
                nnew++;
            }
        }
        return nnew;
    }

private:
    struct Side {
        int n = 0;
        std::vector<OrbxKeyPoint> keys;
        std::vector<uint8_t> desc, skip;
        std::vector<uint32_t> node;
        std::vector<int32_t> start, idx;
        OrblKeyFrame kf;
        OrbmFeatVec fv() const { OrbmFeatVec f; f.n_nodes = (int32_t)node.size(); f.node_id = node.data(); f.start = start.data(); f.idx = idx.data(); return f; }
    };

    static void flatten(KeyFrame* pKF, Side& s)
    {
        s.n = pKF->N;
        s.keys.resize((size_t)s.n); s.desc.resize((size_t)s.n * 32); s.skip.resize((size_t)s.n);
        for (int i = 0; i < s.n; i++) {
            const auto& kp = pKF->mvKeysUn[i];
            OrbxKeyPoint& o = s.keys[i];
            o.x = kp.pt.x; o.y = kp.pt.y; o.size = kp.size; o.angle = kp.angle; o.response = kp.response; o.octave = kp.octave; o.class_id = kp.class_id;
            const unsigned char* d = pKF->mDescriptors.template ptr<unsigned char>(i);
            for (int b = 0; b < 32; b++) s.desc[(size_t)i * 32 + b] = d[b];
            s.skip[i] = pKF->GetMapPoint(i) ? 1 : 0;
        }
        s.start.assign(1, 0);
        for (auto it = pKF->mFeatVec.begin(); it != pKF->mFeatVec.end(); ++it) {
            s.node.push_back(it->first);
            for (size_t j = 0; j < it->second.size(); j++) s.idx.push_back((int32_t)it->second[j]);
            s.start.push_back((int32_t)s.idx.size());
        }
        const auto R = pKF->GetRotation();
        const auto t = pKF->GetTranslation();
        const auto O = pKF->GetCameraCenter();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) s.kf.Rcw[3 * r + c] = R.template at<float>(r, c);
            s.kf.tcw[r] = t.template at<float>(r, 0);
            s.kf.Ow[r] = O.template at<float>(r, 0);
        }
        s.kf.K[0] = pKF->fx; s.kf.K[1] = pKF->fy; s.kf.K[2] = pKF->cx; s.kf.K[3] = pKF->cy;
        s.kf.median_depth = 0.f;
    }

    static void check(int rc) { detail::check(rc, "orbslamm_hip: "); }
};

}  // namespace iORB_SLAM
