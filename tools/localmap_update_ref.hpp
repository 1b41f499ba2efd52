// localmap_update_ref.hpp -- Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1289-1397) and Tracking::UpdateLocalPoints
// (:1263-1286) restated over the arrays of a keyframe store (include/orbslamm_localmap.h).  Plain C++11, no
// project header: the side the device kernels are held to, element for element.
//
// The arrays: per keyframe slot k < kfcap: entries[k * stride .. + stride) (pool id, -1 empty, bit 30 = in the match slot but
// not in the point's observations), kfFlags[k] (bit 0 isBad, bit 1 set), neigh[k * 10 .. + 10) (-1: none), parent[k],
// nchildren[k] and children[k * maxc ..].  Per pool id: ptBad[id].  The frame: frameIds[n] (pool id or -1).
// The two orders the reference leaves to heap addresses are DEFINED: voted keyframes ascending by slot (for
// map<KeyFrame*,int>), children in the order given (for set<KeyFrame*>).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace localmap_update_ref {

const int32_t kNoVote = 1 << 30;

struct Store {
    int kfcap, stride, maxc;
    const int32_t* entries;
    const uint8_t* kfFlags;
    const int32_t* neigh;
    const int32_t* parent;
    const int32_t* nchildren;
    const int32_t* children;
    const uint8_t* ptBad;   // per pool id
    int poolCap;
};

struct KeyFramesResult {
    bool noVotes;
    int kfMax;
    std::vector<int32_t> votes;   // keyframeCounter, by slot (0: not in the map)
    std::vector<int32_t> list;    // mvpLocalKeyFrames
    // which branches ran, for the tests that must see each one
    int nNeighbourTaken, nNeighbourSkippedBad, nNeighbourSkippedIncluded, nNeighboursExhausted, nChildTaken, nChildSkippedBad, nParentTaken, nParentBadTaken,
        nSizeBreak, nStepsRun;
};

// :1293-1309 the multiplicity of every pool id among the frame's points that are not bad (what mnTrackReferenceForFrame /
// mnLastFrameSeen carry per point is, over arrays, "the point is in the frame")
inline std::vector<int32_t> frameCounts(const Store& s, const int32_t* frameIds, int n)
{
    std::vector<int32_t> count((size_t)s.poolCap, 0);
    for (int i = 0; i < n; i++) {                       // :1293
        const int32_t id = frameIds[i];
        if (id < 0) continue;                           // :1295 mvpMapPoints[i] is null
        if (s.ptBad[id]) continue;                      // :1298, :1306 (the slot is nulled: the caller's replay)
        count[(size_t)id]++;
    }
    return count;
}

// :1311-1397 from keyframeCounter (votes[k]; 0: the keyframe is not in the map)
inline void selectKeyFrames(const Store& s, int maxKeyFrames, KeyFramesResult& r);

inline KeyFramesResult updateLocalKeyFrames(const Store& s, const int32_t* frameIds, int n, int maxKeyFrames)
{
    KeyFramesResult r = KeyFramesResult();
    r.kfMax = -1;
    r.votes.assign((size_t)s.kfcap, 0);
    const std::vector<int32_t> count = frameCounts(s, frameIds, n);
    // :1300-1302 keyframeCounter[it->first]++ for every observation of every frame point: per keyframe, the sum over its
    // entries that the point's observations list (bit 30 clear) of the point's multiplicity in the frame
    for (int k = 0; k < s.kfcap; k++) {
        if (!(s.kfFlags[k] & 2)) continue;
        int32_t v = 0;
        for (int e = 0; e < s.stride; e++) {
            const int32_t x = s.entries[(size_t)k * s.stride + e];
            if (x < 0 || (x & kNoVote)) continue;
            v += count[(size_t)x];
        }
        r.votes[(size_t)k] = v;
    }
    selectKeyFrames(s, maxKeyFrames, r);
    return r;
}

// the same with the votes cast as the reference casts them, from per-point observation lists (obsKf[obsStart[id] ..
// obsStart[id + 1]): the keyframes of MapPoint::mObservations, one per voting entry): the walk :1293-1309 does, whose cost does
// not grow with the map.  What tools/localmap_update_bench.py times as the host's way
inline KeyFramesResult updateLocalKeyFramesFromObservations(const Store& s, const int32_t* obsStart, const int32_t* obsKf, const int32_t* frameIds, int n,
                                                            int maxKeyFrames)
{
    KeyFramesResult r = KeyFramesResult();
    r.kfMax = -1;
    r.votes.assign((size_t)s.kfcap, 0);
    for (int i = 0; i < n; i++) {                        // :1293
        const int32_t id = frameIds[i];
        if (id < 0 || s.ptBad[id]) continue;             // :1295, :1298
        for (int32_t o = obsStart[id]; o < obsStart[id + 1]; o++) r.votes[(size_t)obsKf[o]]++;   // :1301-1302
    }
    selectKeyFrames(s, maxKeyFrames, r);
    return r;
}

inline void selectKeyFrames(const Store& s, int maxKeyFrames, KeyFramesResult& r)
{
    bool any = false;
    for (int k = 0; k < s.kfcap; k++) any = any || r.votes[(size_t)k] > 0;
    if (!any) { r.noVotes = true; return; }              // :1311-1312
    int max = 0;                                         // :1314
    std::vector<uint8_t> included((size_t)s.kfcap, 0);   // pKF->mnTrackReferenceForFrame == mCurrentFrame.mnId
    for (int k = 0; k < s.kfcap; k++) {                  // :1321, ascending slot
        if (r.votes[(size_t)k] <= 0) continue;           // not in the map
        if (s.kfFlags[k] & 1) continue;                  // :1325
        if (r.votes[(size_t)k] > max) { max = r.votes[(size_t)k]; r.kfMax = k; }   // :1328-1332
        r.list.push_back(k);                             // :1334
        included[(size_t)k] = 1;                         // :1335
    }
    const size_t end = r.list.size();                    // :1340 itEndKF is taken before the loop
    for (size_t it = 0; it < end; it++) {
        if ((int)r.list.size() > maxKeyFrames) { r.nSizeBreak++; break; }   // :1343
        r.nStepsRun++;
        const int k = r.list[it];                        // :1346
        bool took = false;
        for (int j = 0; j < 10; j++) {                   // :1350 GetBestCovisibilityKeyFrames(10)
            const int nb = s.neigh[(size_t)k * 10 + j];
            if (nb < 0) continue;
            if (s.kfFlags[nb] & 1) { r.nNeighbourSkippedBad++; continue; }   // :1353
            if (included[(size_t)nb]) { r.nNeighbourSkippedIncluded++; continue; }   // :1355
            r.list.push_back(nb); included[(size_t)nb] = 1;   // :1357-1358
            r.nNeighbourTaken++; took = true;
            break;                                       // :1359
        }
        if (!took) r.nNeighboursExhausted++;
        for (int c = 0; c < s.nchildren[k]; c++) {       // :1365, in the order given
            const int ch = s.children[(size_t)k * s.maxc + c];
            if (s.kfFlags[ch] & 1) { r.nChildSkippedBad++; continue; }   // :1368
            if (included[(size_t)ch]) continue;          // :1370
            r.list.push_back(ch); included[(size_t)ch] = 1;   // :1372-1373
            r.nChildTaken++;
            break;                                       // :1374
        }
        const int par = s.parent[k];                     // :1379
        if (par >= 0) {                                  // :1380
            if (!included[(size_t)par]) {                // :1382 -- isBad() is not asked
                r.list.push_back(par); included[(size_t)par] = 1;   // :1384-1385
                r.nParentTaken++;
                if (s.kfFlags[par] & 1) r.nParentBadTaken++;
                break;                                   // :1386: this break leaves the loop over the keyframes
            }
        }
    }
}

struct PointsResult {
    std::vector<int32_t> L;     // mvpLocalMapPoints
    std::vector<uint8_t> seen;  // the point is among the frame's (not bad): Tracking.cc:1228 skips it
    std::vector<int32_t> S;     // L without those
};

inline PointsResult updateLocalPoints(const Store& s, const int32_t* list, int nkf, const int32_t* frameIds, int n)
{
    PointsResult r;
    const std::vector<int32_t> count = frameCounts(s, frameIds, n);
    std::vector<uint8_t> ref((size_t)s.poolCap, 0);      // pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId
    for (int j = 0; j < nkf; j++) {                      // :1267
        const int k = list[j];
        for (int e = 0; e < s.stride; e++) {             // :1272 GetMapPointMatches()
            const int32_t x = s.entries[(size_t)k * s.stride + e];
            if (x < 0) continue;                         // :1275
            const int32_t id = x & ~kNoVote;
            if (ref[(size_t)id]) continue;               // :1277
            if (!s.ptBad[id]) {                          // :1279
                r.L.push_back(id);                       // :1281
                ref[(size_t)id] = 1;                     // :1282
                const uint8_t seen = count[(size_t)id] > 0 ? 1 : 0;
                r.seen.push_back(seen);
                if (!seen) r.S.push_back(id);
            }
        }
    }
    return r;
}

}  // namespace localmap_update_ref
