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
//
//   SearchInNeighborsT<KeyFrame, MapPoint, Mat>::Run(pKF)
//       the drop-in for the body of LocalMapping::SearchInNeighbors (:454-534, monocular; orbl_fuse_batch):
//           typedef iORB_SLAM::SearchInNeighborsT<KeyFrame, MapPoint, cv::Mat> Neighbors;
//           void LocalMapping::SearchInNeighbors() { Neighbors::Run(mpCurrentKeyFrame); }
//       It builds vpTargetKFs exactly as :456-479 do (marks included), makes ONE device call for the first phase (the
//       distinct targets x GetMapPointMatches(), nulls left out), replays it target by target in vpTargetKFs' order, repeats
//       included, with :851 and :953-973 on the host; gathers the candidates (:493-512) AFTER that replay, because they
//       depend on its isBad state; makes one call for the second phase and replays it; then runs the "update points" loop
//       and UpdateConnections() through the reference's own members.
//       The serial dependency.  The search of a (target, point) pair reads the point's position, normal, distance bounds and
//       descriptor.  Nothing in the two Fuse loops touches the first three (UpdateNormalAndDepth runs in the update loop).
//       The descriptor changes in exactly one place: Replace ends in ComputeDistinctiveDescriptors() on the SURVIVING point
//       (MapPoint.cc:212).  A point of the current keyframe that survived a Replace at target k is therefore searched with a
//       new descriptor at targets k+1...  The drop-in keeps the set of survivors of every Replace it issues (both branches,
//       by pointer).  For a pair whose point is in that set the device's best is stale but its (u, v, level) is not: such a
//       pair is re-scored on the host through the reference's own pKF->GetFeaturesInArea(u, v, radius) and :905-951 with the
//       point's current GetDescriptor().  Every other pair's device result is what the serial loop computes, since it
//       depends on nothing the loop writes.  The second phase reads every descriptor after the first phase's replay, and
//       within it no candidate that is processed later can change before it is processed: the survivor of a Replace there
//       is either the candidate just processed (candidates are distinct: mnFuseCandidateForKF) or a point of the current
//       keyframe, which :851's IsInKeyFrame skips.  (The set is consulted there all the same.)
//       MapPoint::mfMinDistance / mfMaxDistance are read raw (the library forms the invariance bounds and PredictScale's
//       ratio itself); they are protected in the reference: INTEGRATION.md.  predict: the tree's own PredictScale as
//       (ratio, logScaleFactor) -> level where its log resolves to the double overload; null: the float form.
//
//   KeyFrameCullingT<KeyFrame, MapPoint>::Run(pool, store, mpCurrentKeyFrame, idOfPoint, slotOfKF)
//       the drop-in for the body of LocalMapping::KeyFrameCulling (:632-698, monocular; orbn_culling_counts) over
//       the keyframe store and its pool; SyncOctaves(store, pKF, slotOfKF) sends mvKeysUn[i].octave of a keyframe once, behind
//       its first UpdateLocalMapT::SyncKeyFrame.  It asks the counts of GetVectorCovisibleKeyFrames() without mnId == 0 and
//       isOtherMapFirst() (:643) in ONE call and walks the list in order; at the first redundant keyframe it calls the
//       keyframe's own SetBadFlag() (:696), whose effects it then sends up -- the keyframe's entries without their vote, the
//       points that EraseObservation turned bad and the match slots they left, the bad flag, the graph records of the
//       keyframes SetBadFlag rewired -- and, when anything went up, asks again for the rest of the list: the one serial
//       dependency of the loop, so the verdicts are the serial loop's.  SetBadFlag's spanning-tree repair stays the reference's.
#pragma once

#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "KeyFrame_hip.hpp"
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
    struct Side : detail::FlatFeatures {   // (keys, desc)
        int n = 0;
        std::vector<uint8_t> skip;
        std::vector<uint32_t> node;
        std::vector<int32_t> start, idx;
        OrblKeyFrame kf;
        OrbmFeatVec fv() const { OrbmFeatVec f; f.n_nodes = (int32_t)node.size(); f.node_id = node.data(); f.start = start.data(); f.idx = idx.data(); return f; }
    };

    static void flatten(KeyFrame* pKF, Side& s)
    {
        s.n = pKF->N;
        detail::flatten_features(pKF, s);
        s.skip.resize((size_t)s.n);
        for (int i = 0; i < s.n; i++) s.skip[i] = pKF->GetMapPoint(i) ? 1 : 0;
        s.start.assign(1, 0);
        for (auto it = pKF->mFeatVec.begin(); it != pKF->mFeatVec.end(); ++it) {
            s.node.push_back(it->first);
            for (size_t j = 0; j < it->second.size(); j++) s.idx.push_back((int32_t)it->second[j]);
            s.start.push_back((int32_t)s.idx.size());
        }
        detail::keyframe_pose(pKF, s.kf.Rcw, s.kf.tcw, s.kf.Ow);
        s.kf.K[0] = pKF->fx; s.kf.K[1] = pKF->fy; s.kf.K[2] = pKF->cx; s.kf.K[3] = pKF->cy;
        s.kf.median_depth = 0.f;
    }

    static void check(int rc) { detail::check(rc, "orbslamm_hip: "); }
};

template <class KeyFrame, class MapPoint, class Mat>
class SearchInNeighborsT {
public:
    static const int TH_LOW = 50;
    struct Stats { int targets = 0, distinctTargets = 0, pairs1 = 0, pairs2 = 0, fused1 = 0, fused2 = 0, dirtyRescored = 0, replaced = 0, added = 0; };

    static void Run(KeyFrame* pKF, int device = 0, Stats* stats = nullptr, orbl_predict_fn predict = nullptr, float th = 3.0f)
    {
        Stats st;
        // Retrieve neighbor keyframes (:456-479)
        const int nn = 20;
        const std::vector<KeyFrame*> vpNeighKFs = pKF->GetBestCovisibilityKeyFrames(nn);
        std::vector<KeyFrame*> vpTargetKFs;
        for (size_t a = 0; a < vpNeighKFs.size(); a++) {
            KeyFrame* pKFi = vpNeighKFs[a];
            if (pKFi->isBad() || pKFi->mnFuseTargetForKF == pKF->mnId) continue;
            vpTargetKFs.push_back(pKFi);
            pKFi->mnFuseTargetForKF = pKF->mnId;
            const std::vector<KeyFrame*> vpSecondNeighKFs = pKFi->GetBestCovisibilityKeyFrames(5);
            for (size_t b = 0; b < vpSecondNeighKFs.size(); b++) {
                KeyFrame* pKFi2 = vpSecondNeighKFs[b];
                if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == pKF->mnId || pKFi2->mnId == pKF->mnId) continue;
                vpTargetKFs.push_back(pKFi2);
            }
        }
        st.targets = (int)vpTargetKFs.size();
        orbm_t* h = nullptr;
        check(orbm_thread_handle(device, &h));
        const int nlevels = (int)pKF->mvScaleFactors.size();
        std::vector<float> breaks((size_t)nlevels + 1);
        check(orbl_level_breaks(pKF->mfLogScaleFactor, nlevels, predict, breaks.data()));
        std::set<MapPoint*> dirty;

        // Search matches by projection from current KF in target KFs (:482-490): one call over the distinct targets
        std::vector<MapPoint*> vpMapPointMatches = pKF->GetMapPointMatches();
        {
            std::map<KeyFrame*, int> slotOf;
            std::vector<KeyFrame*> distinct;
            for (size_t t = 0; t < vpTargetKFs.size(); t++)
                if (!slotOf.count(vpTargetKFs[t])) { slotOf[vpTargetKFs[t]] = (int)distinct.size(); distinct.push_back(vpTargetKFs[t]); }
            st.distinctTargets = (int)distinct.size();
            std::vector<OrblFusePoint> pool;
            std::vector<int> poolOf(vpMapPointMatches.size(), -1);
            for (size_t i = 0; i < vpMapPointMatches.size(); i++)
                if (vpMapPointMatches[i]) { poolOf[i] = (int)pool.size(); pool.push_back(detail::fuse_point<Mat>(vpMapPointMatches[i])); }
            std::vector<OrblFuseResult> res;
            search(h, pKF, distinct, pool, th, breaks, res);
            st.pairs1 = (int)res.size();
            for (size_t t = 0; t < vpTargetKFs.size(); t++)
                st.fused1 += replay(vpTargetKFs[t], vpMapPointMatches, poolOf, res.data() + (size_t)slotOf[vpTargetKFs[t]] * pool.size(), th, dirty, st);
        }

        // Search matches by projection from target KFs in current KF (:492-514): the candidates as the replay left them
        {
            std::vector<MapPoint*> vpFuseCandidates;
            vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
            for (size_t t = 0; t < vpTargetKFs.size(); t++) {
                const std::vector<MapPoint*> vpMapPointsKFi = vpTargetKFs[t]->GetMapPointMatches();
                for (size_t j = 0; j < vpMapPointsKFi.size(); j++) {
                    MapPoint* pMP = vpMapPointsKFi[j];
                    if (!pMP) continue;
                    if (pMP->isBad() || pMP->mnFuseCandidateForKF == pKF->mnId) continue;
                    pMP->mnFuseCandidateForKF = pKF->mnId;
                    vpFuseCandidates.push_back(pMP);
                }
            }
            std::vector<OrblFusePoint> pool(vpFuseCandidates.size());
            std::vector<int> poolOf(vpFuseCandidates.size());
            for (size_t i = 0; i < vpFuseCandidates.size(); i++) { pool[i] = detail::fuse_point<Mat>(vpFuseCandidates[i]); poolOf[i] = (int)i; }
            std::vector<OrblFuseResult> res;
            search(h, pKF, std::vector<KeyFrame*>(1, pKF), pool, th, breaks, res);
            st.pairs2 = (int)res.size();
            dirty.clear();   // (every descriptor was read after the first phase's replay)
            st.fused2 = replay(pKF, vpFuseCandidates, poolOf, res.data(), th, dirty, st);
        }

        // Update points (:517-530)
        vpMapPointMatches = pKF->GetMapPointMatches();
        for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
            MapPoint* pMP = vpMapPointMatches[i];
            if (pMP && !pMP->isBad()) { pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); }
        }
        // Update connections in covisibility graph
        pKF->UpdateConnections();
        if (stats) *stats = st;
    }

private:
    // every pool point against every target, one call: res[t * pool.size() + i]
    static void search(orbm_t* h, KeyFrame* pCur, const std::vector<KeyFrame*>& targets, const std::vector<OrblFusePoint>& pool, float th,
                       const std::vector<float>& breaks, std::vector<OrblFuseResult>& res)
    {
        const int T = (int)targets.size(), P = (int)pool.size();
        res.assign((size_t)T * P, OrblFuseResult());
        if (!T || !P) return;
        if (T > ORBL_FUSE_MAX_TARGETS) throw std::runtime_error("SearchInNeighbors: more targets than ORBL_FUSE_MAX_TARGETS");
        std::vector<OrblFuseTarget> rec((size_t)T);
        std::vector<detail::FlatFeatures> flat((size_t)T);
        std::vector<const OrbxKeyPoint*> keys((size_t)T);
        std::vector<const uint8_t*> desc((size_t)T);
        std::vector<int32_t> n((size_t)T), jobStart((size_t)T + 1), jobPoint((size_t)T * P);
        for (int t = 0; t < T; t++) {
            KeyFrame* k = targets[t];
            float Rcw[9], tcw[3], Ow[3];
            detail::keyframe_pose(k, Rcw, tcw, Ow);
            detail::fuse_target(k, Rcw, tcw, Ow, rec[t]);
            detail::flatten_features(k, flat[t]);
            keys[t] = flat[t].keys.data(); desc[t] = flat[t].desc.data(); n[t] = k->N;
            jobStart[t] = t * P;
            for (int i = 0; i < P; i++) jobPoint[(size_t)t * P + i] = i;
        }
        jobStart[T] = T * P;
        check(orbl_fuse_batch(h, rec.data(), keys.data(), desc.data(), n.data(), T, pool.data(), P, jobStart.data(), jobPoint.data(), th,
                              pCur->mvScaleFactors.data(), pCur->mvInvLevelSigma2.data(), (int)pCur->mvScaleFactors.size(), breaks.data(), res.data()));
    }

    // Fuse's loop (:844-974) over results the device holds for this target; a dirty point is re-scored on the host
    static int replay(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const std::vector<int>& poolOf, const OrblFuseResult* res, float th,
                      std::set<MapPoint*>& dirty, Stats& st)
    {
        int nFused = 0;
        for (size_t i = 0; i < vpMapPoints.size(); i++) {
            MapPoint* pMP = vpMapPoints[i];
            if (!pMP) continue;
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            const OrblFuseResult& r = res[poolOf[i]];
            if (r.status < ORBL_FUSE_ST_NO_CANDIDATE) continue;   // a projection gate, or the level outside mvScaleFactors
            int bestDist = r.best_dist, bestIdx = r.best_idx;
            if (dirty.count(pMP)) {
                // :894-951 with the descriptor the point holds NOW; u, v and the level do not depend on it
                st.dirtyRescored++;
                detail::fuse_rescore<true, Mat>(pKF, pMP, r.u, r.v, r.level, th, bestDist, bestIdx);
            }
            if (bestDist <= TH_LOW && bestIdx >= 0) {   // :954-973
                MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
                if (pMPinKF) {
                    if (!pMPinKF->isBad()) {
                        if (pMPinKF->Observations() > pMP->Observations()) { pMP->Replace(pMPinKF); dirty.insert(pMPinKF); }
                        else { pMPinKF->Replace(pMP); dirty.insert(pMP); }
                        st.replaced++;
                    }
                } else {
                    pMP->AddObservation(pKF, bestIdx);
                    pKF->AddMapPoint(pMP, bestIdx);
                    st.added++;
                }
                nFused++;
            }
        }
        return nFused;
    }

    static void check(int rc) { detail::check(rc, "orbslamm_hip: "); }
};

template <class KeyFrame, class MapPoint>
struct KeyFrameCullingT {
    struct Result { int nCulled; int nCalls; };

    template <class SlotOf>
    static void SyncOctaves(orbu_store_t* store, KeyFrame* pKF, SlotOf slotOfKF)
    {
        std::vector<uint8_t> oct(pKF->mvKeysUn.size());
        for (size_t i = 0; i < oct.size(); i++) oct[i] = (uint8_t)pKF->mvKeysUn[i].octave;
        detail::check(orbu_kf_set_octaves(store, (int)slotOfKF(pKF), oct.data(), (int)oct.size()), "KeyFrameCulling(HIP) SyncOctaves: ");
    }

    template <class IdOf, class SlotOf>
    static Result Run(orbw_pool_t* pool, orbu_store_t* store, KeyFrame* pCurrentKF, IdOf idOfPoint, SlotOf slotOfKF, int thObs = 3)
    {
        const char* who = "KeyFrameCulling(HIP): ";
        Result res; res.nCulled = 0; res.nCalls = 0;
        const std::vector<KeyFrame*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();   // :638
        std::vector<KeyFrame*> list;
        for (size_t i = 0; i < vpLocalKeyFrames.size(); i++)
            if (!(vpLocalKeyFrames[i]->mnId == 0 || vpLocalKeyFrames[i]->isOtherMapFirst())) list.push_back(vpLocalKeyFrames[i]);   // :643
        size_t from = 0;
        while (from < list.size()) {
            std::vector<int32_t> targets;
            for (size_t i = from; i < list.size(); i++) targets.push_back((int32_t)slotOfKF(list[i]));
            OrbnCulling r;
            detail::check(orbn_culling_counts(store, targets.data(), (int)targets.size(), thObs, &r), who);
            res.nCalls++;
            const std::vector<uint8_t> redundant(r.redundant, r.redundant + r.K);   // (the view ends at the store's next call)
            bool again = false;
            const size_t base = from;
            for (size_t i = base; i < list.size() && !again; i++) {
                from = i + 1;
                if (!redundant[i - base]) continue;   // :695
                again = Cull(pool, store, list[i], idOfPoint, slotOfKF, who);
                res.nCulled++;
            }
        }
        return res;
    }

    // pKF->SetBadFlag() (:696) and its effects into the pool and the store; false when nothing changed there
    template <class IdOf, class SlotOf>
    static bool Cull(orbw_pool_t* pool, orbu_store_t* store, KeyFrame* pKF, IdOf idOfPoint, SlotOf slotOfKF, const char* who)
    {
        // ---- as it is: the keyframe's points with their observations, the keyframes whose graph record SetBadFlag may rewrite
        const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
        std::vector<std::map<KeyFrame*, size_t> > obs(vpMPs.size());
        std::vector<bool> wasBad(vpMPs.size(), true), voted(vpMPs.size(), false);
        for (size_t i = 0; i < vpMPs.size(); i++)
            if (vpMPs[i]) { obs[i] = vpMPs[i]->GetObservations(); wasBad[i] = vpMPs[i]->isBad(); voted[i] = vpMPs[i]->IsInKeyFrame(pKF); }
        const bool kfWasBad = pKF->isBad();
        detail::GraphWatch<KeyFrame, SlotOf> watch(slotOfKF);
        watch.watch(pKF);
        watch.watch(pKF->GetParent());
        const std::set<KeyFrame*> connected = pKF->GetConnectedKeyFrames(), childs = pKF->GetChilds();
        for (typename std::set<KeyFrame*>::const_iterator sit = connected.begin(); sit != connected.end(); sit++) watch.watch(*sit);
        for (typename std::set<KeyFrame*>::const_iterator sit = childs.begin(); sit != childs.end(); sit++) watch.watch(*sit);
        pKF->SetBadFlag();
        // ---- what changed, into the pool and the store
        bool changed = false;
        std::vector<int32_t> badIds;
        std::vector<uint8_t> badFlags;
        std::map<KeyFrame*, std::vector<std::pair<int32_t, int32_t> > > slots;   // keyframe -> (idx, value) of its rewritten match slots
        const std::vector<MapPoint*> now = pKF->GetMapPointMatches();
        for (size_t i = 0; i < vpMPs.size(); i++) {
            MapPoint* pMP = vpMPs[i];
            if (!pMP) continue;
            if (!wasBad[i] && pMP->isBad()) {   // MapPoint::SetBadFlag through EraseObservation: the observers' match slots are nulled
                badIds.push_back((int32_t)idOfPoint(pMP)); badFlags.push_back(ORBW_FLAG_BAD);
                for (typename std::map<KeyFrame*, size_t>::const_iterator mit = obs[i].begin(); mit != obs[i].end(); mit++)
                    if (mit->first != pKF) slots[mit->first].push_back(std::make_pair((int32_t)mit->second, (int32_t)-1));
            }
            const int32_t value = i < now.size() && now[i] ? ((int32_t)idOfPoint(now[i]) | (now[i]->IsInKeyFrame(pKF) ? 0 : ORBU_ENTRY_NO_VOTE)) : -1;
            const int32_t was = (int32_t)idOfPoint(pMP) | (voted[i] ? 0 : ORBU_ENTRY_NO_VOTE);
            if (value != was) slots[pKF].push_back(std::make_pair((int32_t)i, value));
        }
        if (!badIds.empty()) { detail::check(orbw_pool_set_flags(pool, badIds.data(), badFlags.data(), (int)badIds.size()), who); changed = true; }
        for (typename std::map<KeyFrame*, std::vector<std::pair<int32_t, int32_t> > >::const_iterator it = slots.begin(); it != slots.end(); it++) {
            std::vector<int32_t> idx, vals;
            for (size_t q = 0; q < it->second.size(); q++) { idx.push_back(it->second[q].first); vals.push_back(it->second[q].second); }
            detail::check(orbu_kf_set_entries(store, (int)slotOfKF(it->first), idx.data(), vals.data(), (int)idx.size()), who);
            changed = true;
        }
        if (pKF->isBad() != kfWasBad) {
            const int32_t slot = (int32_t)slotOfKF(pKF);
            const uint8_t flags = pKF->isBad() ? ORBU_KF_BAD : 0;
            detail::check(orbu_kf_set_flags(store, &slot, &flags, 1), who);
        }
        watch.push(store, who);
        return changed;
    }
};

}  // namespace iORB_SLAM
