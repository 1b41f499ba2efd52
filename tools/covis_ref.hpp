// covis_ref.hpp -- KeyFrame::UpdateConnections (src/KeyFrame.cc:300-400) and the body of LocalMapping::KeyFrameCulling's outer
// loop (src/LocalMapping.cc:632-698, monocular) restated over the arrays of a keyframe store (include/orbslamm_covis.h,
// DESIGN.md §8u).  Plain C++11, no project header: the side the device kernels are held to, element for element.
//
// The arrays: per keyframe slot k < kfcap: entries[k * stride .. + stride) (pool id, -1 empty, bit 30 = in the match slot but
// not in the point's observations), kfFlags[k] (bit 1 set), octaves[k * stride ..] (mvKeysUn[i].octave as a byte).  Per pool
// id: ptBad[id].  Both members go through MapPoint::mObservations, which is built here as an index per pool id of the voting
// entries (keyframe, feature) in ascending (keyframe, feature): the reference's walk, not the device's passes over the store.
// The orders the reference leaves to heap addresses are DEFINED as slot order (map<KeyFrame*,int> ascending, pair<int,
// KeyFrame*> compared by slot).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace covis_ref {

const int32_t kNoVote = 1 << 30;

struct Store {
    int kfcap, stride;
    const int32_t* entries;
    const uint8_t* kfFlags;
    const uint8_t* octaves;   // null where only UpdateConnections is asked
    const uint8_t* ptBad;     // per pool id
    int poolCap;
};

// which branches ran, for the tests that must see each one
struct Branches {
    int emptyCounter, fallbackToMax, tieAtMax, orderedTies, selfSkipped, badPointSkipped, noVoteTargetSlot, duplicateEntry;
    int obsAtTh, obsAtThPlus1, octavePlus1, octavePlus2, qualifyingBelow, qualifyingAt, redundantYes, redundantNo;
};
const int kBranchInts = 16;

// MapPoint::mObservations of every point: AddObservation(pKF, idx) for every voting entry of every set keyframe
struct Observations {
    std::vector<int32_t> start, kf, idx;
    explicit Observations(const Store& s) : start((size_t)s.poolCap + 1, 0)
    {
        for (int pass = 0; pass < 2; pass++) {
            std::vector<int32_t> fill(start.begin(), start.end() - 1);
            for (int k = 0; k < s.kfcap; k++) {
                if (!(s.kfFlags[k] & 2)) continue;
                for (int i = 0; i < s.stride; i++) {
                    const int32_t v = s.entries[(size_t)k * s.stride + i];
                    if (v < 0 || (v & kNoVote)) continue;
                    if (pass == 0) start[(size_t)v + 1]++;
                    else { kf[(size_t)fill[v]] = k; idx[(size_t)fill[v]] = i; fill[v]++; }
                }
            }
            if (pass == 0) {
                for (int p = 0; p < s.poolCap; p++) start[(size_t)p + 1] += start[(size_t)p];
                kf.resize((size_t)start[(size_t)s.poolCap]); idx.resize(kf.size());
            }
        }
    }
    int count(int32_t p) const { return start[(size_t)p + 1] - start[(size_t)p]; }   // MapPoint::Observations()
};

struct Connections {
    bool empty;                                        // KeyFrame.cc:334
    int kfMax, nMax;
    std::vector<std::pair<int32_t, int32_t> > counter;  // (kf, weight) ascending kf: mConnectedKeyFrameWeights (:388)
    std::vector<std::pair<int32_t, int32_t> > ordered;  // (kf, weight): mvpOrderedConnectedKeyFrames / mvOrderedWeights (:389-390)
};

inline Connections updateConnections(const Store& s, const Observations& obs, int k, int th, Branches* brp)
{
    Branches none = Branches();
    Branches& br = brp ? *brp : none;   // (brp null: the walk alone, as the benchmark times it)
    Connections r;
    std::map<int32_t, int> KFcounter;                                  // :302 map<KeyFrame*,int>, by slot
    std::vector<int32_t> met;
    for (int i = 0; i < s.stride; i++) {                               // :313 over vpMP = mvpMapPoints (:308)
        const int32_t raw = s.entries[(size_t)k * s.stride + i];
        if (raw < 0) continue;                                         // :317 !pMP
        const int32_t p = raw & ~kNoVote;
        if (raw & kNoVote) br.noVoteTargetSlot++;
        if (s.ptBad[p]) { br.badPointSkipped++; continue; }            // :320
        if (brp) met.push_back(p);
        for (int32_t o = obs.start[(size_t)p]; o < obs.start[(size_t)p + 1]; o++) {   // :323-325 GetObservations()
            if (obs.kf[(size_t)o] == k) { br.selfSkipped++; continue; }               // :327 mnId == mnId
            KFcounter[obs.kf[(size_t)o]]++;                            // :329
        }
    }
    std::sort(met.begin(), met.end());
    for (size_t q = 1; q < met.size(); q++) br.duplicateEntry += met[q] == met[q - 1] ? 1 : 0;
    r.empty = KFcounter.empty();
    r.kfMax = -1; r.nMax = 0;
    if (r.empty) { br.emptyCounter++; return r; }                      // :334
    int nmax = 0, pKFmax = -1;                                         // :339-340
    std::vector<std::pair<int, int32_t> > vPairs;                      // :343
    for (std::map<int32_t, int>::const_iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {   // :345
        r.counter.push_back(std::make_pair(mit->first, (int32_t)mit->second));
        if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; }     // :347-351
        if (mit->second >= th) vPairs.push_back(std::make_pair(mit->second, mit->first));   // :352-356
    }
    int atMax = 0;
    for (size_t q = 0; q < r.counter.size(); q++) atMax += r.counter[q].second == nmax ? 1 : 0;
    if (atMax > 1) br.tieAtMax++;
    if (vPairs.empty()) { vPairs.push_back(std::make_pair(nmax, pKFmax)); br.fallbackToMax++; }   // :359-363
    std::sort(vPairs.begin(), vPairs.end());                           // :365 pair<int,KeyFrame*>: weight, then slot
    bool ties = false;
    for (size_t q = 0; q < vPairs.size(); q++) {                       // :368-372 push_front: the order is reversed
        r.ordered.insert(r.ordered.begin(), std::make_pair(vPairs[q].second, (int32_t)vPairs[q].first));
        ties = ties || (q > 0 && vPairs[q].first == vPairs[q - 1].first);
    }
    if (ties) br.orderedTies++;
    r.kfMax = pKFmax; r.nMax = nmax;
    return r;
}

struct Culling { int nMPs, nRedundant; bool redundant; };

inline Culling cullingCounts(const Store& s, const Observations& obs, int k, int thObs, Branches* brp)
{
    Branches none = Branches();
    Branches& br = brp ? *brp : none;
    Culling r;
    int nRedundantObservations = 0, nMPs = 0;                          // LocalMapping.cc:651-652
    for (int i = 0; i < s.stride; i++) {                               // :653
        const int32_t raw = s.entries[(size_t)k * s.stride + i];
        if (raw < 0) continue;                                         // :656
        const int32_t p = raw & ~kNoVote;
        if (s.ptBad[p]) continue;                                      // :658
        nMPs++;                                                        // :666
        if (obs.count(p) == thObs) br.obsAtTh++;
        if (obs.count(p) == thObs + 1) br.obsAtThPlus1++;
        if (obs.count(p) > thObs) {                                    // :667
            const int scaleLevel = s.octaves[(size_t)k * s.stride + i];   // :669
            int nObs = 0, qualifying = 0;                              // :671
            for (int32_t o = obs.start[(size_t)p]; brp && o < obs.start[(size_t)p + 1]; o++) {   // counted without the break, for the branches alone
                if (obs.kf[(size_t)o] == k) continue;
                const int li = s.octaves[(size_t)obs.kf[(size_t)o] * s.stride + obs.idx[(size_t)o]];
                if (li == scaleLevel + 1) br.octavePlus1++;
                if (li == scaleLevel + 2) br.octavePlus2++;
                qualifying += li <= scaleLevel + 1 ? 1 : 0;
            }
            if (qualifying == thObs - 1) br.qualifyingBelow++;
            if (qualifying == thObs) br.qualifyingAt++;
            for (int32_t o = obs.start[(size_t)p]; o < obs.start[(size_t)p + 1]; o++) {   // :672
                if (obs.kf[(size_t)o] == k) continue;                  // :675
                const int scaleLeveli = s.octaves[(size_t)obs.kf[(size_t)o] * s.stride + obs.idx[(size_t)o]];   // :677
                if (scaleLeveli <= scaleLevel + 1) {                   // :679
                    nObs++;                                            // :681
                    if (nObs >= thObs) break;                          // :682
                }
            }
            if (nObs >= thObs) nRedundantObservations++;               // :686-688
        }
    }
    r.nMPs = nMPs; r.nRedundant = nRedundantObservations;
    r.redundant = nRedundantObservations > 0.9 * nMPs;                  // :695
    if (r.redundant) br.redundantYes++; else br.redundantNo++;
    return r;
}

}  // namespace covis_ref
