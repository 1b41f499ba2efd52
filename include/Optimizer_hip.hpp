// Optimizer_hip.hpp -- the reference's Optimizer::PoseOptimization (include/Optimizer.h, src/Optimizer.cc:261-473 of both
// scenarios), monocular, over the C ABI of liborbslamm_hip.so (orbo_*), and its Optimizer::OptimizeSim3
// (src/Optimizer.cc:1348-1543; orbz_*; OptimizeSim3T, below PoseOptimizationT).  Header-only, C++11.  The two-keyframe bundle
// adjustment of the initial map runs on the device as well (orbb_*; its drop-in is InitialMapT in Tracking_hip.hpp).  The rest of
// Optimizer (the local and the global bundle adjustment, the essential graph) stays with g2o.
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

//   OptimizeSim3T<KeyFrame, MapPoint, Sim3>::Run(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)
//       the drop-in for Optimizer::OptimizeSim3: the reference's walk over vpMatches1 on the host (:1401-1440: null and bad points
//       and a negative GetIndexInKeyFrame skipped), ONE device call, then vpMatches1 nulled exactly where the reference nulls it,
//       g2oS12 written only when the reference writes it (not on the early return of :1514) and nIn returned.  In the reference tree:
//           int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12,
//                                       const float th2, const bool bFixScale)
//           { return iORB_SLAM::OptimizeSim3T<KeyFrame, MapPoint, g2o::Sim3>::Run(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale); }
//   OptimizeSim3T<...>::RunAll(jobs)
//       the same for a list of such argument packs in ONE device call and launch: the candidates of one ComputeSim3 (the first Sim3
//       of every candidate is known once Sim3SolverT::RunAll has run), or every keyframe of every newer map in MultiMapper::Run.
//       Every job's outputs are written as if Run had been called on it alone; the caller walks them in the reference's candidate
//       order and stops at the first with >= 20.  All pKF1 of a call must share one level table and all pKF2 another (they may be
//       the same), as the keyframes of one extractor do.
//   Sim3 needs rotation() (with coeffs()[0..3], x y z w), translation() (indexable), scale() and a constructor from
//   (rotation, translation, scale), as g2o::Sim3 has.  KeyFrame needs GetMapPointMatches, GetRotation, GetTranslation, mvKeysUn,
//   mvuRight, mvInvLevelSigma2 and fx fy cx cy (mK's entries); MapPoint needs isBad, GetIndexInKeyFrame and GetWorldPos.  A used
//   feature with a stereo observation (mvuRight >= 0) is refused.  Nothing is written before the device call returns: a refusal
//   throws with every job as it came.
template <class KeyFrame, class MapPoint, class Sim3>
class OptimizeSim3T {
public:
    struct Job {
        KeyFrame* pKF1;
        KeyFrame* pKF2;
        std::vector<MapPoint*>* vpMatches1;
        Sim3* g2oS12;
        float th2;
        bool bFixScale;
    };

    static int Run(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, Sim3& g2oS12, const float th2, const bool bFixScale, int device = 0)
    {
        Job j;
        j.pKF1 = pKF1; j.pKF2 = pKF2; j.vpMatches1 = &vpMatches1; j.g2oS12 = &g2oS12; j.th2 = th2; j.bFixScale = bFixScale;
        return RunAll(std::vector<Job>(1, j), device)[0];
    }

    static std::vector<int> RunAll(const std::vector<Job>& jobs, int device = 0, std::vector<OrbzResult>* results = nullptr)
    {
        const int nj = (int)jobs.size();
        std::vector<int> ret(jobs.size(), 0);
        if (results) results->assign(jobs.size(), OrbzResult());
        if (!nj) return ret;
        std::vector<OrbzProblem> prob((size_t)nj);
        std::vector<int32_t> start(1, 0);
        std::vector<OrbzCorr> corrs;
        const std::vector<float>& sigma1 = jobs[0].pKF1->mvInvLevelSigma2;
        const std::vector<float>& sigma2 = jobs[0].pKF2->mvInvLevelSigma2;
        if (sigma1.size() != sigma2.size()) throw std::runtime_error("OptimizeSim3(HIP): the two keyframes' level tables differ in length");
        for (int k = 0; k < nj; k++) {
            const Job& J = jobs[k];
            KeyFrame* pKF1 = J.pKF1;
            KeyFrame* pKF2 = J.pKF2;
            if (pKF1->mvInvLevelSigma2 != sigma1 || pKF2->mvInvLevelSigma2 != sigma2)
                throw std::runtime_error("OptimizeSim3(HIP): the jobs of one call must share the two keyframes' mvInvLevelSigma2");
            OrbzProblem& P = prob[k];
            for (int c = 0; c < 4; c++) P.q[c] = J.g2oS12->rotation().coeffs()[c];
            for (int c = 0; c < 3; c++) P.t[c] = J.g2oS12->translation()[c];
            P.s = J.g2oS12->scale();
            const auto R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation(), R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) { P.R1w[3 * r + c] = R1w.template at<float>(r, c); P.R2w[3 * r + c] = R2w.template at<float>(r, c); }
                P.t1w[r] = t1w.template at<float>(r, 0); P.t2w[r] = t2w.template at<float>(r, 0);
            }
            P.K1[0] = pKF1->fx; P.K1[1] = pKF1->fy; P.K1[2] = pKF1->cx; P.K1[3] = pKF1->cy;
            P.K2[0] = pKF2->fx; P.K2[1] = pKF2->fy; P.K2[2] = pKF2->cx; P.K2[3] = pKF2->cy;
            P.th2 = J.th2;
            P.fix_scale = J.bFixScale ? 1 : 0;
            // :1401-1440
            const std::vector<MapPoint*>& vpMatches1 = *J.vpMatches1;
            const int N = (int)vpMatches1.size();
            const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
            for (int i = 0; i < N; i++) {
                if (!vpMatches1[i]) continue;
                MapPoint* pMP1 = vpMapPoints1[i];
                MapPoint* pMP2 = vpMatches1[i];
                const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
                if (!pMP1 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
                if (((size_t)i < pKF1->mvuRight.size() && !(pKF1->mvuRight[i] < 0)) || ((size_t)i2 < pKF2->mvuRight.size() && !(pKF2->mvuRight[i2] < 0)))
                    throw std::runtime_error("OptimizeSim3(HIP): match " + std::to_string(i) + " uses a stereo observation (mvuRight >= 0); the device OptimizeSim3 is monocular");
                OrbzCorr c;
                c.idx1 = i;
                const auto& kp1 = pKF1->mvKeysUn[i];
                const auto& kp2 = pKF2->mvKeysUn[i2];
                c.obs1[0] = kp1.pt.x; c.obs1[1] = kp1.pt.y; c.oct1 = kp1.octave;
                c.obs2[0] = kp2.pt.x; c.obs2[1] = kp2.pt.y; c.oct2 = kp2.octave;
                const auto X1 = pMP1->GetWorldPos(), X2 = pMP2->GetWorldPos();
                for (int r = 0; r < 3; r++) { c.X1w[r] = X1.template at<float>(r, 0); c.X2w[r] = X2.template at<float>(r, 0); }
                corrs.push_back(c);
            }
            start.push_back((int32_t)corrs.size());
        }
        std::vector<OrbzResult> out((size_t)nj);
        std::vector<uint8_t> removed(corrs.size() + 1, 0);
        orbm_t* h = nullptr;
        detail::check(orbm_thread_handle(device, &h), "OptimizeSim3(HIP): ");
        detail::check(orbz_optimize_sim3(h, prob.data(), nj, start.data(), corrs.data(), sigma1.data(), sigma2.data(), (int)sigma1.size(), out.data(),
                                         removed.data()),
                      "OptimizeSim3(HIP): ");
        // nothing of any job has been written up to here
        for (int k = 0; k < nj; k++) {
            const Job& J = jobs[k];
            for (int32_t c = start[k]; c < start[k + 1]; c++)
                if (removed[c]) (*J.vpMatches1)[corrs[c].idx1] = static_cast<MapPoint*>(nullptr);   // :1499, :1533
            if (out[k].written) {   // :1541; not reached on the early return of :1514
                auto r = J.g2oS12->rotation();
                auto t = J.g2oS12->translation();
                for (int c = 0; c < 4; c++) r.coeffs()[c] = out[k].q[c];
                for (int c = 0; c < 3; c++) t[c] = out[k].t[c];
                *J.g2oS12 = Sim3(r, t, out[k].s);
            }
            ret[k] = out[k].n_in;
            if (results) (*results)[k] = out[k];
        }
        return ret;
    }
};

}  // namespace iORB_SLAM
