// KeyFrame_hip.hpp -- drop-in for KeyFrame::UpdateConnections (src/KeyFrame.cc:300-400) on liborbslamm_hip.so's covisibility
// block (include/orbslamm_covis.h) over the keyframe store (include/orbslamm_localmap.h).  Header-only, C++11.
//
//   iORB_SLAM::UpdateConnectionsT<KeyFrame, MapPoint>::Run(store, pKF, slotOfKF, kfOfSlot);
//   iORB_SLAM::UpdateConnectionsT<KeyFrame, MapPoint>::RunAll(store, vpKFs, slotOfKF, kfOfSlot);   // CorrectLoop's and the merge's loops
//
// The store holds every keyframe's match slots as UpdateLocalMapT::SyncKeyFrame (include/Tracking_hip.hpp) leaves them; slotOfKF
// is slot = mnId, the DEFINED choice of the headers: where the reference iterates map<KeyFrame*,int> and compares KeyFrame* in
// heap-address order, the device uses ascending slot.  RunAll makes ONE device call for the whole vector -- the counters of
// different keyframes do not depend on each other -- and then, per keyframe in the given order, replays what is serial:
//   KeyFrame.cc:355, :362   (mit->first)->AddConnection(this, w) for the members with w >= th in ascending slot, or for pKFmax alone
//   :368-398                pKF->AssignConnections(KFcounter, vpOrdered, vOrderedWs): the other-map marks, the assignment of
//                           mConnectedKeyFrameWeights / mvpOrderedConnectedKeyFrames / mvOrderedWeights and the first-connection
//                           parent.  This is the ONE public member the reference's KeyFrame lacks (INTEGRATION.md states the patch).
// A keyframe whose counter is empty is left as it was (:334).  It ends with one orbu_kf_set_graph for the keyframes whose graph
// record (ten best neighbours, parent, children) changed: the targets, the receivers of an AddConnection and the new parents.
// A refusal of the library throws std::runtime_error with every keyframe as it came.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

namespace detail {

// a keyframe's graph record as the store holds it: GetBestCovisibilityKeyFrames(10), GetParent, GetChilds ascending by mnId
struct GraphRecord {
    int32_t neigh[ORBU_MAX_NEIGHBOURS];
    int32_t parent;
    std::vector<int32_t> children;
    bool operator==(const GraphRecord& o) const { return std::equal(neigh, neigh + ORBU_MAX_NEIGHBOURS, o.neigh) && parent == o.parent && children == o.children; }
};

template <class KeyFrame, class SlotOf>
GraphRecord graph_record(KeyFrame* pKF, SlotOf slotOfKF)
{
    GraphRecord g;
    for (int j = 0; j < ORBU_MAX_NEIGHBOURS; j++) g.neigh[j] = -1;
    const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(ORBU_MAX_NEIGHBOURS);
    for (size_t j = 0; j < vNeighs.size() && j < (size_t)ORBU_MAX_NEIGHBOURS; j++) g.neigh[j] = (int32_t)slotOfKF(vNeighs[j]);
    const std::set<KeyFrame*> spChilds = pKF->GetChilds();
    std::vector<std::pair<long unsigned int, int32_t> > byId;
    for (typename std::set<KeyFrame*>::const_iterator sit = spChilds.begin(); sit != spChilds.end(); sit++) byId.push_back(std::make_pair((*sit)->mnId, (int32_t)slotOfKF(*sit)));
    std::sort(byId.begin(), byId.end());
    for (size_t c = 0; c < byId.size(); c++) g.children.push_back(byId[c].second);
    KeyFrame* pParent = pKF->GetParent();
    g.parent = pParent ? (int32_t)slotOfKF(pParent) : -1;
    return g;
}

// the graph records of the keyframes that may change, as they were; push() sends the ones that did change in one call
template <class KeyFrame, class SlotOf>
struct GraphWatch {
    SlotOf slotOfKF;
    std::vector<KeyFrame*> order;
    std::map<KeyFrame*, GraphRecord> before;
    explicit GraphWatch(SlotOf s) : slotOfKF(s) {}
    void watch(KeyFrame* pKF)
    {
        if (!pKF || before.count(pKF)) return;
        before[pKF] = graph_record(pKF, slotOfKF);
        order.push_back(pKF);
    }
    int push(orbu_store_t* store, const char* who)
    {
        std::vector<int32_t> slot, neigh, parent, nchildren, children;
        for (size_t i = 0; i < order.size(); i++) {
            const GraphRecord g = graph_record(order[i], slotOfKF);
            if (g == before[order[i]]) continue;
            slot.push_back((int32_t)slotOfKF(order[i]));
            neigh.insert(neigh.end(), g.neigh, g.neigh + ORBU_MAX_NEIGHBOURS);
            parent.push_back(g.parent);
            nchildren.push_back((int32_t)g.children.size());
            children.insert(children.end(), g.children.begin(), g.children.end());
        }
        if (slot.empty()) return 0;
        OrbuKeyFrames rec;
        rec.nkf = (int32_t)slot.size(); rec.slot = slot.data(); rec.flags = nullptr; rec.n = nullptr; rec.entries = nullptr; rec.neigh = neigh.data();
        rec.parent = parent.data(); rec.nchildren = nchildren.data(); rec.children = children.data();
        check(orbu_kf_set_graph(store, &rec), who);
        return (int)slot.size();
    }
};

}  // namespace detail

template <class KeyFrame, class MapPoint>
struct UpdateConnectionsT {
    struct Result { int nUpdated; int nEmpty; int nGraphRecords; };

    template <class SlotOf, class KfOf>
    static Result Run(orbu_store_t* store, KeyFrame* pKF, SlotOf slotOfKF, KfOf kfOfSlot, int th = 15)
    {
        return RunAll(store, std::vector<KeyFrame*>(1, pKF), slotOfKF, kfOfSlot, th);
    }

    template <class SlotOf, class KfOf>
    static Result RunAll(orbu_store_t* store, const std::vector<KeyFrame*>& vpKFs, SlotOf slotOfKF, KfOf kfOfSlot, int th = 15)
    {
        const char* who = "UpdateConnections(HIP): ";
        Result res; res.nUpdated = 0; res.nEmpty = 0; res.nGraphRecords = 0;
        if (vpKFs.empty()) return res;
        // ---- the device call, with nothing touched
        std::vector<int32_t> targets(vpKFs.size());
        for (size_t t = 0; t < vpKFs.size(); t++) targets[t] = (int32_t)slotOfKF(vpKFs[t]);
        OrbnConnections r;
        detail::check(orbn_update_connections(store, targets.data(), (int)targets.size(), th, &r), who);
        // ---- the replay, per keyframe in the given order
        detail::GraphWatch<KeyFrame, SlotOf> watch(slotOfKF);
        for (size_t t = 0; t < vpKFs.size(); t++) {
            KeyFrame* pKF = vpKFs[t];
            if (r.status[t] == ORBN_EMPTY) { res.nEmpty++; continue; }   // KeyFrame.cc:334
            std::map<KeyFrame*, int> KFcounter;
            bool any = false;
            for (int32_t q = r.cnt_start[t]; q < r.cnt_start[t + 1]; q++) {   // :345 in ascending slot
                KeyFrame* pOther = kfOfSlot(r.cnt_kf[q]);
                KFcounter[pOther] = r.cnt_w[q];
                if (r.cnt_w[q] >= th) {   // :352-356
                    watch.watch(pOther);
                    pOther->AddConnection(pKF, r.cnt_w[q]);
                    any = true;
                }
            }
            if (!any) {   // :359-363
                KeyFrame* pKFmax = kfOfSlot(r.kf_max[t]);
                watch.watch(pKFmax);
                pKFmax->AddConnection(pKF, r.n_max[t]);
            }
            std::vector<KeyFrame*> vpOrdered;
            std::vector<int> vOrderedWs;
            for (int32_t q = r.ord_start[t]; q < r.ord_start[t + 1]; q++) { vpOrdered.push_back(kfOfSlot(r.ord_kf[q])); vOrderedWs.push_back(r.ord_w[q]); }
            watch.watch(pKF);
            watch.watch(vpOrdered.front());   // (the parent a first connection takes: its children change)
            pKF->AssignConnections(KFcounter, vpOrdered, vOrderedWs);   // :368-398
            res.nUpdated++;
        }
        res.nGraphRecords = watch.push(store, who);
        return res;
    }
};

}  // namespace iORB_SLAM
