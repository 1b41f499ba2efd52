// Optimizer_hip.hpp -- the reference's Optimizer::PoseOptimization (include/Optimizer.h, src/Optimizer.cc:261-473 of both
// scenarios), monocular, over the C ABI of liborbslamm_hip.so (orbo_*).  Header-only, C++11.  The rest of
// Optimizer (the bundle adjustments, the essential graph, Sim3) stays with g2o.
//
//   PoseOptimizationT<Frame, MapPoint>::Run(pFrame)
//       the drop-in for Optimizer::PoseOptimization(pFrame): the reference's walk over mvpMapPoints on the host (:302-341:
//       mvbOutlier[i] = false for every observation, the key, its level's information, the point's position), ONE device
//       call, then mvbOutlier written, SetPose called with the optimised pose and nInitialCorrespondences - nBad returned.
//       With fewer than 3 observations it returns 0 and leaves the pose alone, as :386 does.  In the reference tree:
//           int Optimizer::PoseOptimization(Frame* pFrame) { return iORB_SLAM::PoseOptimizationT<Frame, MapPoint>::Run(pFrame); }
//   PoseOptimizationT<Frame, MapPoint>::RunAll(frames)
//       the same for several frames in ONE device call and launch: Tracking::Relocalization's candidates, each a copy of
//       the lost frame with its own matches and its PnP pose (null entries, the discarded candidates, are skipped and get
//       0).  The frames must share the level table (mvInvLevelSigma2), as the frames of one extractor do.
//   A frame with a stereo observation (mvuRight[i] >= 0 at a matched feature) is refused with a std::runtime_error:
//   monocular is the scope of every solver of this library.  A call that throws has written nothing: no flag, no pose, of
//   no frame of the list.
//   Frame needs N, mvpMapPoints, mvuRight, mvKeysUn, mvbOutlier, mvInvLevelSigma2, mTcw (with clone() and at<float>(r, c)),
//   fx fy cx cy and SetPose; MapPoint needs GetWorldPos().  Every call runs on the calling thread's matcher handle
//   (orbm_thread_handle), as the other drop-ins do.  The arithmetic is the DEFINED one of DESIGN.md §8o.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class Frame, class MapPoint>
class PoseOptimizationT {
public:
    static int Run(Frame* pFrame, int device = 0) { return RunAll(std::vector<Frame*>(1, pFrame), device)[0]; }

    static std::vector<int> RunAll(const std::vector<Frame*>& frames, int device = 0, std::vector<OrboResult>* results = nullptr)
    {
        std::vector<Frame*> live;
        std::vector<size_t> slot;
        for (size_t k = 0; k < frames.size(); k++) if (frames[k]) { live.push_back(frames[k]); slot.push_back(k); }
        std::vector<int> ret(frames.size(), 0);
        if (results) results->assign(frames.size(), OrboResult());
        if (live.empty()) return ret;
        const int nf = (int)live.size();
        std::vector<OrboFrame> rec((size_t)nf);
        std::vector<std::vector<OrbxKeyPoint> > keys((size_t)nf);
        std::vector<const OrbxKeyPoint*> keyPtr((size_t)nf);
        std::vector<int32_t> nKeys((size_t)nf), start(1, 0);
        std::vector<OrboEdge> edges;
        const std::vector<float>& sigma = live[0]->mvInvLevelSigma2;
        for (int f = 0; f < nf; f++) {
            Frame* F = live[f];
            if (F->mvInvLevelSigma2 != sigma) throw std::runtime_error("PoseOptimization(HIP): the frames of one call must share mvInvLevelSigma2");
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) rec[f].Tcw[4 * r + c] = F->mTcw.template at<float>(r, c);
            rec[f].K[0] = F->fx; rec[f].K[1] = F->fy; rec[f].K[2] = F->cx; rec[f].K[3] = F->cy;
            const int N = F->N;
            keys[f].resize((size_t)N);
            for (int i = 0; i < N; i++) {
                const auto& kp = F->mvKeysUn[i];
                OrbxKeyPoint& o = keys[f][i];
                o.x = kp.pt.x; o.y = kp.pt.y; o.size = kp.size; o.angle = kp.angle; o.response = kp.response; o.octave = kp.octave; o.class_id = kp.class_id;
                MapPoint* pMP = F->mvpMapPoints[i];
                if (!pMP) continue;
                if (!(F->mvuRight[i] < 0))
                    throw std::runtime_error("PoseOptimization(HIP): feature " + std::to_string(i) + " is a stereo observation (mvuRight >= 0); the device PoseOptimization is monocular");
                OrboEdge e;
                e.feature = i;
                const auto Xw = pMP->GetWorldPos();
                for (int r = 0; r < 3; r++) e.Xw[r] = Xw.template at<float>(r, 0);
                edges.push_back(e);
            }
            keyPtr[f] = keys[f].data();
            nKeys[f] = N;
            start.push_back((int32_t)edges.size());
        }
        std::vector<OrboResult> out((size_t)nf);
        std::vector<uint8_t> flags(edges.size() + 1, 0);
        orbm_t* h = nullptr;
        detail::check(orbm_thread_handle(device, &h), "PoseOptimization(HIP): ");
        detail::check(orbo_pose_optimize(h, rec.data(), keyPtr.data(), nKeys.data(), nf, start.data(), edges.data(), sigma.data(), (int)sigma.size(),
                                         out.data(), flags.data()),
                      "PoseOptimization(HIP): ");
        // nothing of any frame has been written up to here: a refusal (a stereo observation, another level table, a ceiling, an
        // octave outside the table) throws with every frame as it came.  Every observation's flag is written now, which also
        // is :311's mvbOutlier[i] = false (below 3 observations the call returns all flags clear)
        for (int f = 0; f < nf; f++) {
            Frame* F = live[f];
            for (int32_t e = start[f]; e < start[f + 1]; e++) F->mvbOutlier[edges[e].feature] = flags[e] != 0;
            if (out[f].rounds > 0) {   // (below 3 observations the reference returns before SetPose)
                auto pose = F->mTcw.clone();
                for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) pose.template at<float>(r, c) = out[f].Tcw[4 * r + c];
                F->SetPose(pose);
            }
            ret[slot[f]] = out[f].n_good;
            if (results) (*results)[slot[f]] = out[f];
        }
        return ret;
    }
};

}  // namespace iORB_SLAM
