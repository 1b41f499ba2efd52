// LoopClosing_hip.hpp -- the reference's LoopClosing::SearchAndFuse (src/LoopClosing.cc:601-627) and
// MultiMapper::SearchAndFuse (src/MultiMapper.cc:668-694), monocular, over the C ABI of liborbslamm_hip.so (orbc_*,
// include/orbslamm_loopfuse.h).  Header-only, C++11.
//
//   SearchAndFuseT<KeyFrame, MapPoint, Mat>::Run(corrected, vpLoopMapPoints, th)
//       the drop-in for the body of both functions.  `corrected` holds (KeyFrame*, Scw) in the caller's iteration order
//       (CorrectedSim3's; for the merge, mvpCurrentMapKFs' with each keyframe's corrected pose), Scw a 4x4 CV_32F Mat as
//       Converter::toCvMat(g2oScw) gives it.  In the reference tree:
//           typedef iORB_SLAM::SearchAndFuseT<KeyFrame, MapPoint, cv::Mat> LoopFuse;
//           void LoopClosing::SearchAndFuse(const KeyFrameAndPose& CorrectedPosesMap)
//           {
//               std::vector<std::pair<KeyFrame*, cv::Mat> > corrected;
//               for (auto mit = CorrectedPosesMap.begin(); mit != CorrectedPosesMap.end(); mit++)
//                   corrected.push_back(std::make_pair(mit->first, Converter::toCvMat(mit->second)));
//               LoopFuse::Run(corrected, mvpLoopMapPoints, 4, [this] { return std::unique_lock<std::mutex>(mpMap->mMutexMapUpdate); });
//           }
//       Run decomposes every Scw (ORBmatcher.cc:987-992, cvsem::decomposeSim3), makes ONE device call over all targets
//       (orbc_search_and_fuse: every loop point against every corrected keyframe; a keyframe listed twice is flattened and
//       uploaded once) and then replays the serial part on the host, target by target, in the reference's order:
//         1. spAlreadyFound = pKF->GetMapPoints(), read at this target's turn: it depends on every earlier Replace.
//         2. for iMP ascending: skip isBad() and already-found points; take the pair's hit from the device list with a cursor
//            over hit_start; apply :1084-1097 (GetMapPoint(bestIdx), vpReplacePoint[iMP], or AddObservation + AddMapPoint at
//            once); count nFused.
//         3. under the caller's lock: vpReplacePoints[i]->Replace(vpLoopMapPoints[i]) for i ascending (:616-625).
//       The map mutex.  The reference takes mpMap->mMutexMapUpdate per target, after Fuse and around the Replace loop only.
//       Run takes the lock as a functor: lock() is called once per target, right before step 3, and what it returns lives
//       until that target's Replace loop has ended.  The default functor returns nothing worth holding: a caller that
//       holds the mutex around the whole call, or has no other thread, passes none.
//
//       Which dependencies cross pairs, and how each is resolved:
//         - Replace ends in ComputeDistinctiveDescriptors() on the SURVIVING point (MapPoint.cc:212), and in step 3 the
//           survivor is the loop point.  Its descriptor may change, so its device results at LATER targets are stale.  Run
//           keeps the set of survivors (by pointer).  For a pair whose point is in the set the device's hit, or its absence,
//           is ignored and that ONE pair is searched again on the host: the projection forms of
//           ORBmatcherT::projectIntoKeyFrame (cvsem, with :1021's 1.0/z), the level from the same break table the device
//           uses, pKF->GetFeaturesInArea and :1060-1081 with the point's current GetDescriptor().  Position, normal and
//           distance bounds do not change inside SearchAndFuse, so every other pair's device result is what the serial loop
//           computes.
//         - A point that Replace turns bad: pMPinKF may itself be a loop point, placed there by an earlier AddMapPoint or
//           Replace.  The isBad() read at replay (step 2) skips it from then on.
//         - Two loop points choosing the same feature of one target: the second finds the first as pMPinKF and replaces it.
//           That is GetMapPoint(bestIdx) read at replay, in order; the device is not involved.
//       Run returns the total of nFused; Stats::rescored counts the pairs searched again on the host.
//       MapPoint::mfMinDistance / mfMaxDistance are read raw, as SearchInNeighborsT does.  predict: the
//       tree's own PredictScale as (ratio, logScaleFactor) -> level where its log resolves to the double overload; null: the
//       float form.  Monocular only.  Every call runs on the calling thread's matcher handle (orbm_thread_handle).
//
//   CorrectLoopPosesT<KeyFrame, MapPoint, Sim3>::Run(store, keyframes, pCurrentKF, Scw, alreadyCorrected, scaleFactors,
//                                                    CorrectedSim3, NonCorrectedSim3, hooks)
//       the drop-in for LoopClosing.cc:455-524 and MultiMapper.cc:523-595 (orbe_correct_sim3, include/orbslamm_correct.h,
//       DESIGN.md §8x): documented at the class, below.
#pragma once

#include <algorithm>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ORBmatcher_hip.hpp"
#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

struct SearchAndFuseNoLock { int operator()() const { return 0; } };

template <class KeyFrame, class MapPoint, class Mat>
class SearchAndFuseT {
public:
    static const int TH_LOW = 50;
    struct Stats { int targets = 0, distinctTargets = 0, points = 0, hits = 0, fused = 0, replaced = 0, added = 0; long pairs = 0, rescored = 0; };
    // rescoreStale = false leaves the host re-score of survivors out: WRONG, and there for the test that shows it
    struct Options { int device = 0; orbl_predict_fn predict = nullptr; bool rescoreStale = true; };

    static int Run(const std::vector<std::pair<KeyFrame*, Mat> >& corrected, const std::vector<MapPoint*>& vpLoopMapPoints, float th,
                   Stats* stats = nullptr, const Options& opt = Options())
    {
        return Run(corrected, vpLoopMapPoints, th, SearchAndFuseNoLock(), stats, opt);
    }

    template <class Lock>
    static int Run(const std::vector<std::pair<KeyFrame*, Mat> >& corrected, const std::vector<MapPoint*>& vpLoopMapPoints, float th, Lock lock,
                   Stats* stats = nullptr, const Options& opt = Options())
    {
        Stats st;
        const int T = (int)corrected.size(), P = (int)vpLoopMapPoints.size();
        st.targets = T; st.points = P; st.pairs = (long)T * P;
        if (!T || !P) { if (stats) *stats = st; return 0; }
        KeyFrame* pFirst = corrected[0].first;
        const int nlevels = (int)pFirst->mvScaleFactors.size();
        std::vector<float> breaks((size_t)nlevels + 1);
        check(orbl_level_breaks(pFirst->mfLogScaleFactor, nlevels, opt.predict, breaks.data()));

        // the targets: the decomposed Scw, the keyframe's intrinsics, bounds and grid; every distinct keyframe flattened once
        std::vector<OrblFuseTarget> rec((size_t)T);
        std::map<KeyFrame*, int> flatOf;
        std::vector<detail::FlatFeatures> flat;
        flat.reserve((size_t)T);
        std::vector<const OrbxKeyPoint*> keys((size_t)T);
        std::vector<const uint8_t*> desc((size_t)T);
        std::vector<int32_t> n((size_t)T);
        for (int t = 0; t < T; t++) {
            KeyFrame* k = corrected[t].first;
            cvsem::Mat33 Rcw; cvsem::Vec3 tcw, Ow;
            cvsem::decomposeSim3(corrected[t].second, Rcw, tcw, Ow);
            detail::fuse_target(k, Rcw.m, tcw.v, Ow.v, rec[t]);   // (Mat33::m is row-major)
            if (!flatOf.count(k)) {
                flatOf[k] = (int)flat.size();
                flat.push_back(detail::FlatFeatures());
                detail::flatten_features(k, flat.back());
            }
            const detail::FlatFeatures& f = flat[flatOf[k]];   // (flat was reserved: the addresses stay)
            keys[t] = f.keys.data(); desc[t] = f.desc.data(); n[t] = k->N;
        }
        st.distinctTargets = (int)flat.size();
        std::vector<OrblFusePoint> pool((size_t)P);
        for (int i = 0; i < P; i++) pool[i] = detail::fuse_point<Mat>(vpLoopMapPoints[i]);

        // ONE device call; the hit list is small against T x P, its size unknown: a first guess, then the count the library names
        orbm_t* h = nullptr;
        check(orbm_thread_handle(opt.device, &h));
        std::vector<OrbcHit> hits((size_t)std::max(4 * P, 4096));
        std::vector<int32_t> hitStart((size_t)T + 1);
        int nHits = 0;
        for (int attempt = 0;; attempt++) {
            const int rc = orbc_search_and_fuse(h, rec.data(), keys.data(), desc.data(), n.data(), T, pool.data(), P, th, TH_LOW,
                                                pFirst->mvScaleFactors.data(), nlevels, breaks.data(), hits.data(), (int)hits.size(), &nHits,
                                                hitStart.data(), nullptr);
            if (rc == ORBX_E_CAPACITY && attempt == 0) { hits.resize((size_t)nHits); continue; }
            check(rc);
            break;
        }
        st.hits = nHits;

        // the serial part, in the reference's order
        std::set<MapPoint*> survivors;
        int total = 0;
        for (int t = 0; t < T; t++) {
            KeyFrame* pKF = corrected[t].first;
            std::vector<MapPoint*> vpReplacePoints((size_t)P, static_cast<MapPoint*>(nullptr));
            const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();   // :995
            int cur = hitStart[t];
            const int end = hitStart[t + 1];
            int nFused = 0;
            for (int iMP = 0; iMP < P; iMP++) {
                MapPoint* pMP = vpLoopMapPoints[iMP];
                while (cur < end && hits[cur].point < iMP) cur++;
                if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;   // :1007
                int bestIdx = -1;
                if (opt.rescoreStale && survivors.count(pMP)) {
                    st.rescored++;
                    bestIdx = searchOnHost(pKF, rec[t], pMP, th, breaks);
                } else if (cur < end && hits[cur].point == iMP) bestIdx = hits[cur].best_idx;
                if (bestIdx < 0) continue;
                MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);   // :1084-1097
                if (pMPinKF) {
                    if (!pMPinKF->isBad()) vpReplacePoints[iMP] = pMPinKF;
                } else {
                    pMP->AddObservation(pKF, bestIdx);
                    pKF->AddMapPoint(pMP, bestIdx);
                    st.added++;
                }
                nFused++;
            }
            total += nFused;
            {
                auto guard = lock();   // Get Map Mutex (LoopClosing.cc:616)
                (void)guard;
                for (int i = 0; i < P; i++) {
                    MapPoint* pRep = vpReplacePoints[i];
                    if (pRep) {
                        pRep->Replace(vpLoopMapPoints[i]);
                        survivors.insert(vpLoopMapPoints[i]);
                        st.replaced++;
                    }
                }
            }
        }
        st.fused = total;
        if (stats) *stats = st;
        return total;
    }

private:
    // ORBmatcher.cc:1010-1081 for ONE pair with the descriptor the point holds now; the best feature when bestDist <= TH_LOW, else -1
    static int searchOnHost(KeyFrame* pKF, const OrblFuseTarget& T, MapPoint* pMP, float th, const std::vector<float>& breaks)
    {
        using namespace cvsem;
        Mat33 Rcw; Vec3 tcw, Ow;
        for (int i = 0; i < 9; i++) Rcw.m[i] = T.Rcw[i];
        for (int i = 0; i < 3; i++) { tcw.v[i] = T.tcw[i]; Ow.v[i] = T.Ow[i]; }
        const Vec3 p3Dw = col3(pMP->GetWorldPos());
        const Vec3 p3Dc = mulAdd(Rcw, p3Dw, tcw);
        if (p3Dc[2] < 0.0f) return -1;
        const float invz = (float)(1.0 / (double)p3Dc[2]);
        const float x = p3Dc[0] * invz, y = p3Dc[1] * invz;
        const float u = T.K[0] * x + T.K[2], v = T.K[1] * y + T.K[3];
        if (!(u >= T.min_x && u < T.max_x && v >= T.min_y && v < T.max_y)) return -1;
        const float maxDistance = 1.2f * pMP->mfMaxDistance, minDistance = 0.8f * pMP->mfMinDistance;
        const Vec3 PO = sub(p3Dw, Ow);
        const float dist3D = (float)norm(PO);
        if (dist3D < minDistance || dist3D > maxDistance) return -1;
        if (dot(PO, col3(pMP->GetNormal())) < 0.5 * dist3D) return -1;
        const float ratio = pMP->mfMaxDistance / dist3D;
        int c = 0;
        for (size_t j = 0; j < breaks.size(); j++) c += ratio > breaks[j] ? 1 : 0;
        const int nlevels = (int)breaks.size() - 1;
        if (c < 1 || c > nlevels) return -1;
        int bestDist, bestIdx;
        detail::fuse_rescore<false, Mat>(pKF, pMP, u, v, c - 1, th, bestDist, bestIdx);
        return bestDist <= TH_LOW ? bestIdx : -1;
    }

    static void check(int rc) { detail::check(rc, "orbslamm_hip: "); }
};

// ---------------------------------------------------------------------------------------------------------------------
//   ComputeSim3T<KeyFrame, MapPoint, Sim3>::RunAll(h, pool, store, jobs, idOf)
//       what LoopClosing::ComputeSim3 (src/LoopClosing.cc:316-331) and MultiMapper::Run do per candidate behind Sim3Solver::iterate --
//       matcher.SearchBySim3(pKF1, pKF2, vpMapPointMatches, s, R, t, 7.5) and Optimizer::OptimizeSim3(pKF1, pKF2, vpMapPointMatches,
//       gScm, 10, mbFixScale) -- for a list of candidates in ONE device call (orby_compute_sim3, include/orbslamm_computesim3.h,
//       DESIGN.md section 8v).  The caller has both keyframes of a job in two slots of one frame set, their match lists in the keyframe
//       store (UpdateLocalMapT::SyncKeyFrame) and their points in the pool; idOf(MapPoint*) is a point's pool id.  Per job RunAll builds
//       m12_id / m12_idx2 from vpMapPointMatches as it enters (the solver's inliers, :319-324: the pool id and
//       GetIndexInKeyFrame(pKF2)), and writes back vpMapPointMatches, gScm (only when the reference writes it: not on the early return
//       of Optimizer.cc:1514) and nInliers as if SearchBySim3 followed by OptimizeSim3T::Run had run on that job alone.  The caller
//       walks the results in the reference's candidate order and stops at the first with nInliers >= 20 (:333); the jobs behind the
//       accepted one have run, which the reference does not do -- their outputs are simply not read (OptimizeSim3T::RunAll's note).
//       All pKF1 of a call share one set of level tables and all pKF2 another.  Monocular: a keyframe with a stereo observation is
//       refused.  Nothing is written before the device call returns: a refusal throws with everything as it came.
//       PRECONDITION (orbslamm_computesim3.h): a point that votes at slot q of a keyframe's store row has GetIndexInKeyFrame == q.
template <class KeyFrame, class MapPoint, class Sim3>
class ComputeSim3T {
public:
    struct Job {
        orbm_frameset_t* fs; int slot1, slot2;   // the two keyframes as slots of one resident frame set
        int kf1, kf2;                            // ... and as slots of the keyframe store
        KeyFrame* pKF1;                          // mpCurrentKF
        KeyFrame* pKF2;                          // the candidate
        std::vector<MapPoint*>* vpMapPointMatches;
        float R12[9], t12[3], s12;               // pSolver->GetEstimatedRotation / Translation / Scale (setSim3)
        Sim3* gScm;                              // g2o::Sim3(toMatrix3d(R), toVector3d(t), s), :329
        bool bFixScale;
        float th, th2;                           // 7.5 and 10 in both callers
        template <class Mat> void setSim3(const Mat& R, const Mat& t, float s)
        {
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R12[3 * r + c] = R.template at<float>(r, c); t12[r] = t.template at<float>(r, 0); }
            s12 = s;
        }
    };
    struct Result { int nFound; int nInliers; OrbzResult opt; };

    template <class IdOf>
    static std::vector<Result> RunAll(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const std::vector<Job>& jobs, IdOf idOf,
                                      orbl_predict_fn predict = nullptr)
    {
        const char* who = "ComputeSim3(HIP): ";
        const int nj = (int)jobs.size();
        std::vector<Result> ret(jobs.size());
        if (!nj) return ret;
        KeyFrame* first1 = jobs[0].pKF1;
        KeyFrame* first2 = jobs[0].pKF2;
        const int nlevels = (int)first1->mvScaleFactors.size();
        if ((int)first2->mvScaleFactors.size() != nlevels) throw std::runtime_error(std::string(who) + "the two keyframes' level tables differ in length");
        std::vector<float> breaks1((size_t)nlevels + 1), breaks2((size_t)nlevels + 1);
        detail::check(orbl_level_breaks(first1->mfLogScaleFactor, nlevels, predict, breaks1.data()), who);
        detail::check(orbl_level_breaks(first2->mfLogScaleFactor, nlevels, predict, breaks2.data()), who);
        std::vector<OrbyJob> rec((size_t)nj);
        std::vector<std::vector<int32_t> > id((size_t)nj), idx2((size_t)nj), matchOut((size_t)nj), idsOut((size_t)nj);
        std::vector<int32_t*> pMatch((size_t)nj), pIds((size_t)nj);
        for (int k = 0; k < nj; k++) {
            const Job& J = jobs[k];
            KeyFrame* pKF1 = J.pKF1;
            KeyFrame* pKF2 = J.pKF2;
            if (pKF1->mvScaleFactors != first1->mvScaleFactors || pKF2->mvScaleFactors != first2->mvScaleFactors ||
                pKF1->mvInvLevelSigma2 != first1->mvInvLevelSigma2 || pKF2->mvInvLevelSigma2 != first2->mvInvLevelSigma2 ||
                pKF1->mfLogScaleFactor != first1->mfLogScaleFactor || pKF2->mfLogScaleFactor != first2->mfLogScaleFactor)
                throw std::runtime_error(std::string(who) + "the jobs of one call must share the two keyframes' level tables");
            for (size_t i = 0; i < pKF1->mvuRight.size(); i++)
                if (!(pKF1->mvuRight[i] < 0)) throw std::runtime_error(std::string(who) + "pKF1 holds a stereo observation (mvuRight >= 0); the device ComputeSim3 is monocular");
            for (size_t i = 0; i < pKF2->mvuRight.size(); i++)
                if (!(pKF2->mvuRight[i] < 0)) throw std::runtime_error(std::string(who) + "pKF2 holds a stereo observation (mvuRight >= 0); the device ComputeSim3 is monocular");
            const std::vector<MapPoint*>& vp = *J.vpMapPointMatches;
            const int N1 = (int)vp.size(), N2 = (int)pKF2->GetMapPointMatches().size();
            OrbyJob& R = rec[(size_t)k];
            R.fs = J.fs; R.slot1 = J.slot1; R.slot2 = J.slot2; R.kf1 = J.kf1; R.kf2 = J.kf2; R.n1 = N1; R.n2 = N2;
            OrbzProblem& P = R.prob;
            for (int c = 0; c < 4; c++) P.q[c] = J.gScm->rotation().coeffs()[c];
            for (int c = 0; c < 3; c++) P.t[c] = J.gScm->translation()[c];
            P.s = J.gScm->scale();
            const auto R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation(), R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) { P.R1w[3 * r + c] = R1w.template at<float>(r, c); P.R2w[3 * r + c] = R2w.template at<float>(r, c); }
                P.t1w[r] = t1w.template at<float>(r, 0); P.t2w[r] = t2w.template at<float>(r, 0);
            }
            P.K1[0] = pKF1->fx; P.K1[1] = pKF1->fy; P.K1[2] = pKF1->cx; P.K1[3] = pKF1->cy;
            P.K2[0] = pKF2->fx; P.K2[1] = pKF2->fy; P.K2[2] = pKF2->cx; P.K2[3] = pKF2->cy;
            P.th2 = J.th2;
            P.fix_scale = J.bFixScale ? 1 : 0;
            for (int c = 0; c < 9; c++) R.R12[c] = J.R12[c];
            for (int c = 0; c < 3; c++) R.t12[c] = J.t12[c];
            R.s12 = J.s12;
            R.bounds1[0] = (float)pKF1->mnMinX; R.bounds1[1] = (float)pKF1->mnMaxX; R.bounds1[2] = (float)pKF1->mnMinY; R.bounds1[3] = (float)pKF1->mnMaxY;
            R.bounds2[0] = (float)pKF2->mnMinX; R.bounds2[1] = (float)pKF2->mnMaxX; R.bounds2[2] = (float)pKF2->mnMinY; R.bounds2[3] = (float)pKF2->mnMaxY;
            R.th = J.th;
            // LoopClosing.cc:319-324 as it reaches SearchBySim3 (ORBmatcher.cc:1131-1144) and OptimizeSim3 (Optimizer.cc:1412)
            id[(size_t)k].assign((size_t)N1 + 1, -1);
            idx2[(size_t)k].assign((size_t)N1 + 1, -1);
            for (int i = 0; i < N1; i++)
                if (vp[(size_t)i]) { id[(size_t)k][(size_t)i] = (int32_t)idOf(vp[(size_t)i]); idx2[(size_t)k][(size_t)i] = (int32_t)vp[(size_t)i]->GetIndexInKeyFrame(pKF2); }
            R.m12_id = id[(size_t)k].data(); R.m12_idx2 = idx2[(size_t)k].data();
            matchOut[(size_t)k].assign((size_t)N1 + 1, -1); idsOut[(size_t)k].assign((size_t)N1 + 1, -1);
            pMatch[(size_t)k] = matchOut[(size_t)k].data(); pIds[(size_t)k] = idsOut[(size_t)k].data();
        }
        std::vector<OrbyResult> out((size_t)nj);
        detail::check(orby_compute_sim3(h, pool, store, rec.data(), nj, first1->mvScaleFactors.data(), first2->mvScaleFactors.data(), breaks1.data(),
                                        breaks2.data(), first1->mvInvLevelSigma2.data(), first2->mvInvLevelSigma2.data(), nlevels, out.data(), pMatch.data(),
                                        pIds.data(), nullptr, nullptr, nullptr),
                      who);
        // nothing of any job has been written up to here
        for (int k = 0; k < nj; k++) {
            const Job& J = jobs[k];
            std::vector<MapPoint*>& vp = *J.vpMapPointMatches;
            const std::vector<MapPoint*> vpMapPoints2 = J.pKF2->GetMapPointMatches();
            for (size_t i = 0; i < vp.size(); i++) {
                if (idsOut[(size_t)k][i] < 0) { vp[i] = static_cast<MapPoint*>(nullptr); continue; }   // no match, or nulled by a check (Optimizer.cc:1497, :1532)
                if (vp[i]) continue;                                                                      // an entering match that stays
                const int m = matchOut[(size_t)k][i];
                if (m < 0 || m >= (int)vpMapPoints2.size() || !vpMapPoints2[(size_t)m])
                    throw std::runtime_error(std::string(who) + "a new match names a feature of pKF2 without a MapPoint: the store is behind the keyframe");
                vp[i] = vpMapPoints2[(size_t)m];   // ORBmatcher.cc:1318
            }
            const OrbzResult& o = out[(size_t)k].opt;
            if (o.written) {   // Optimizer.cc:1541; not reached on the early return of :1514
                auto r = J.gScm->rotation();
                auto t = J.gScm->translation();
                for (int c = 0; c < 4; c++) r.coeffs()[c] = o.q[c];
                for (int c = 0; c < 3; c++) t[c] = o.t[c];
                *J.gScm = Sim3(r, t, o.s);
            }
            ret[(size_t)k].nFound = out[(size_t)k].n_found; ret[(size_t)k].nInliers = o.n_in; ret[(size_t)k].opt = o;
        }
        return ret;
    }
};

// CorrectLoopPosesT -- the correction of LoopClosing::CorrectLoop (src/LoopClosing.cc:455-524) and of
// MultiMapper::UpdatePosesAndAdd (src/MultiMapper.cc:523-595) in ONE device call over the keyframe store (orbe_correct_sim3):
//     KeyFrameAndPose CorrectedSim3, NonCorrectedSim3;                       // :444; :445 and :446 are the call's
//     { unique_lock<mutex> lock(mpMap->mMutexMapUpdate);                     // :451
//       CorrectLoopPosesT<KeyFrame, MapPoint, g2o::Sim3>::Run(store, mvpCurrentConnectedKFs, mpCurrentKF, mg2oScw, {}, mvScaleFactors,
//                                                            CorrectedSim3, NonCorrectedSim3, hooks);
//       ... :523 pKFi->UpdateConnections() of every listed keyframe stays the caller's (it reads no pose: orbn_update_connections
//       serves it in one call), then :526 the loop fusion as before }
// keyframes: mvpCurrentConnectedKFs with mpCurrentKF pushed back (:441-442), or mvpCurrentMapKFs; slot = mnId, as the other
// drop-ins.  alreadyCorrected: the MapPoints that carry mnCorrectedByKF == pCurrentKF->mnId from an earlier call (:496; none in
// a first correction by this keyframe).  The store must hold every listed keyframe's match slots, every set keyframe's centre and
// octaves as they are NOW, and mpRefKF of the points (orbu_point_set_ref_kf).  Run fills the two maps (:469, :476), calls
// SetPose with the corrected poses (:520), and writes SetWorldPos, mnCorrectedByKF, mnCorrectedReference (:505-507) and, where
// UpdateNormalAndDepth is defined and ran (:508), the normal and the bounds of every moved point from the call's records; the
// pool's records and the store's centres are committed by the same call.  Where the reference walks map<KeyFrame*, g2o::Sim3> in
// heap-address order the device takes ascending mnId: the DEFINED choice of the headers.  `hooks` is the caller's object:
//   int32_t SlotOfKF(KeyFrame*); int32_t IdOfPoint(MapPoint*); MapPoint* PointOfId(int32_t)
//   void Pose(KeyFrame*, float Tiw[12])              GetPose() as three rows [R | t]
//   void SetPose(KeyFrame*, const float Tiw[12])     pKFi->SetPose(correctedTiw)
//   void SetWorldPos(MapPoint*, const float[3]); void SetNormalAndDepth(MapPoint*, const float normal[3], float minD, float maxD)
// A refusal of the library throws std::runtime_error with every keyframe and point as it came.  Monocular.
template <class KeyFrame, class MapPoint, class Sim3>
struct CorrectLoopPosesT {
    struct Result {
        int nMoved, nNormals;                 // the points moved; those whose normal and bounds were written
        int nUndefined;                       // ORBR_ST_NO_REF + ORBR_ST_LEVEL_RANGE, where the reference is undefined
        std::vector<OrbeKeyFrame> keyframes;  // in the order of `keyframes`
        std::vector<OrbePoint> points;        // in the reference's visiting order
    };

    static Sim3 MakeSim3(const Sim3& like, const double* v)
    {
        auto r = like.rotation();
        auto t = like.translation();
        for (int c = 0; c < 4; c++) r.coeffs()[c] = v[c];
        for (int c = 0; c < 3; c++) t[c] = v[4 + c];
        return Sim3(r, t, v[7]);
    }

    template <class Map, class Hooks>
    static Result Run(orbu_store_t* store, const std::vector<KeyFrame*>& keyframes, KeyFrame* pCurrentKF, const Sim3& Scw, const std::vector<MapPoint*>& alreadyCorrected,
                      const std::vector<float>& scaleFactors, Map& CorrectedSim3, Map& NonCorrectedSim3, Hooks& hooks)
    {
        const char* who = "CorrectLoopPoses(HIP): ";
        Result res; res.nMoved = 0; res.nNormals = 0; res.nUndefined = 0;
        const size_t K = keyframes.size();
        std::vector<int32_t> slots(K), skip(alreadyCorrected.size());
        std::vector<float> Tiw(12 * K);
        int anchor = -1;
        size_t room = 0;
        for (size_t i = 0; i < K; i++) {
            slots[i] = hooks.SlotOfKF(keyframes[i]);
            hooks.Pose(keyframes[i], &Tiw[12 * i]);
            if (keyframes[i] == pCurrentKF) anchor = (int)i;
            room += keyframes[i]->GetMapPointMatches().size();
        }
        if (anchor < 0) throw std::runtime_error(std::string(who) + "the current keyframe is not among the listed ones");
        for (size_t i = 0; i < skip.size(); i++) skip[i] = hooks.IdOfPoint(alreadyCorrected[i]);
        double S[8];
        for (int c = 0; c < 4; c++) S[c] = Scw.rotation().coeffs()[c];
        for (int c = 0; c < 3; c++) S[4 + c] = Scw.translation()[c];
        S[7] = Scw.scale();
        // ---- the device call, with nothing touched
        res.keyframes.resize(K);
        res.points.resize(room);
        int n = 0;
        detail::check(orbe_correct_sim3(store, slots.data(), Tiw.data(), (int)K, anchor, S, skip.data(), (int)skip.size(), scaleFactors.data(), (int)scaleFactors.size(), 1,
                                        res.keyframes.data(), res.points.data(), (int)room, &n), who);
        res.points.resize((size_t)n);
        // ---- the host objects
        for (size_t i = 0; i < K; i++) {
            const OrbeKeyFrame& k = res.keyframes[i];
            CorrectedSim3[keyframes[i]] = MakeSim3(Scw, k.corrected);          // :445, :469
            NonCorrectedSim3[keyframes[i]] = MakeSim3(Scw, k.non_corrected);   // :476
            hooks.SetPose(keyframes[i], k.Tiw);                                // :520
        }
        for (size_t i = 0; i < res.points.size(); i++) {
            const OrbePoint& o = res.points[i];
            MapPoint* pMP = hooks.PointOfId(o.id);
            hooks.SetWorldPos(pMP, o.pos);                                     // :505
            pMP->mnCorrectedByKF = pCurrentKF->mnId;                           // :506
            pMP->mnCorrectedReference = (long unsigned int)o.owner_slot;       // :507 (slot = mnId)
            if (o.status == ORBR_ST_DONE) { hooks.SetNormalAndDepth(pMP, o.normal, o.min_distance, o.max_distance); res.nNormals++; }   // :508
            if (o.status == ORBR_ST_NO_REF || o.status == ORBR_ST_LEVEL_RANGE) res.nUndefined++;
            res.nMoved++;
        }
        return res;
    }
};

}  // namespace iORB_SLAM
