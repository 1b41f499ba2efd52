// C shim over tools/localmap_update_ref.hpp for tests/ref_shim.py: the restatement of Tracking::UpdateLocalKeyFrames and
// Tracking::UpdateLocalPoints over a keyframe store's arrays.
#include "../../tools/localmap_update_ref.hpp"

#include <cstring>

using namespace localmap_update_ref;

// out_hdr[16]: noVotes, kfMax, nkf, then the branch counters in KeyFramesResult's order.  out_votes[kfcap], out_list[kfcap]
extern "C" void lmu_keyframes(const Store* s, const int32_t* frameIds, int n, int maxKeyFrames, int32_t* out_hdr, int32_t* out_votes, int32_t* out_list)
{
    const KeyFramesResult r = updateLocalKeyFrames(*s, frameIds, n, maxKeyFrames);
    const int32_t hdr[16] = {r.noVotes ? 1 : 0, r.kfMax, (int32_t)r.list.size(), r.nNeighbourTaken, r.nNeighbourSkippedBad, r.nNeighbourSkippedIncluded,
                             r.nNeighboursExhausted, r.nChildTaken, r.nChildSkippedBad, r.nParentTaken, r.nParentBadTaken, r.nSizeBreak, r.nStepsRun, 0, 0, 0};
    memcpy(out_hdr, hdr, sizeof hdr);
    memcpy(out_votes, r.votes.data(), r.votes.size() * 4);
    if (!r.list.empty()) memcpy(out_list, r.list.data(), r.list.size() * 4);
}

// the same with the votes cast from per-point observation lists (CSR over pool ids)
extern "C" void lmu_keyframes_obs(const Store* s, const int32_t* obsStart, const int32_t* obsKf, const int32_t* frameIds, int n, int maxKeyFrames,
                                  int32_t* out_hdr, int32_t* out_votes, int32_t* out_list)
{
    const KeyFramesResult r = updateLocalKeyFramesFromObservations(*s, obsStart, obsKf, frameIds, n, maxKeyFrames);
    out_hdr[0] = r.noVotes ? 1 : 0; out_hdr[1] = r.kfMax; out_hdr[2] = (int32_t)r.list.size();
    memcpy(out_votes, r.votes.data(), r.votes.size() * 4);
    if (!r.list.empty()) memcpy(out_list, r.list.data(), r.list.size() * 4);
}

// out_n[2] = nL, nS; out_L / out_seen / out_S hold up to cap elements (more: only the counts are written)
extern "C" void lmu_points(const Store* s, const int32_t* list, int nkf, const int32_t* frameIds, int n, int cap, int32_t* out_n, int32_t* out_L,
                           uint8_t* out_seen, int32_t* out_S)
{
    const PointsResult r = updateLocalPoints(*s, list, nkf, frameIds, n);
    out_n[0] = (int32_t)r.L.size(); out_n[1] = (int32_t)r.S.size();
    if ((int)r.L.size() > cap) return;
    if (!r.L.empty()) { memcpy(out_L, r.L.data(), r.L.size() * 4); memcpy(out_seen, r.seen.data(), r.seen.size()); }
    if (!r.S.empty()) memcpy(out_S, r.S.data(), r.S.size() * 4);
}
