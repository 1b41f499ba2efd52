// C shim over tools/trackpose_ref.hpp for the Python checkers (tests/trackpose_cases.py; built by tests/ref_shim.py).
#include "../../tools/trackpose_ref.hpp"

using namespace trackpose_ref;

extern "C" {

int trackposeref_sizes(int i) { return i == 0 ? (int)sizeof(Key) : i == 1 ? (int)sizeof(Result) : (int)sizeof(Branches); }

// one job: keys[n]; assign[n] / ids[nq] or null; base_ids[n] or null; the pool as pos[3 * cap] and flags[cap].  Returns 0, or -1
// for what the device refuses behind its kernel (nothing is written then)
int trackposeref_run(const Key* keys, int n, const int32_t* assign, const int32_t* ids, int nq, const int32_t* base_ids, int discard,
                     const float* Tcw, const float* K, const float* pos, const uint8_t* flags, int cap, const float* inv_level_sigma2, int nlevels,
                     Result* out, int32_t* ids_out, uint8_t* outlier_out, Branches* br)
{
    Job J;
    J.keys = keys; J.assign = assign; J.ids = ids; J.nq = nq; J.baseIds = base_ids; J.n = n; J.discard = discard;
    for (int i = 0; i < 16; i++) J.frame.Tcw[i] = Tcw[i];
    for (int i = 0; i < 4; i++) J.frame.K[i] = K[i];
    const Pool P = {pos, flags, cap};
    return trackPose(P, J, inv_level_sigma2, nlevels, *out, ids_out, outlier_out, br);
}

int trackposeref_motion_model_verdict(int n_matches, int n_matches_map, int only_tracking, int* vo)
{
    bool v = false;
    const bool r = motionModelVerdict(n_matches, n_matches_map, only_tracking != 0, &v);
    if (vo) *vo = v ? 1 : 0;
    return r ? 1 : 0;
}

int trackposeref_local_map_verdict(int n_matches, int n_matches_map, int only_tracking, long frame_id, long last_reloc, long max_frames)
{
    return localMapVerdict(n_matches, n_matches_map, only_tracking != 0, frame_id, last_reloc, max_frames) ? 1 : 0;
}

// The parent's way around orbo_pose_optimize_frames in its kindest host form (tools/trackpose_bench.py): the merge and the gather of Xw
// from a flat host copy of the pool into {feature, Xw[3]} records, no pointer chasing; returns the edge count
int trackposeref_host_edges(const int32_t* assign, const int32_t* ids, const int32_t* base_ids, int n, const float* pos, int32_t* merged, void* edges)
{
    struct E { int32_t feature; float Xw[3]; };
    E* e = (E*)edges;
    int m = 0;
    for (int t = 0; t < n; t++) {
        const int32_t id = assign && assign[t] >= 0 ? ids[assign[t]] : (base_ids ? base_ids[t] : -1);
        merged[t] = id;
        if (id < 0) continue;
        e[m].feature = t; e[m].Xw[0] = pos[3 * (size_t)id]; e[m].Xw[1] = pos[3 * (size_t)id + 1]; e[m].Xw[2] = pos[3 * (size_t)id + 2];
        m++;
    }
    return m;
}

// ... and the walk over mvbOutlier behind it: per-edge flags back onto the features, the discard, the two counts
void trackposeref_host_epilogue(const int32_t* merged, int n, const uint8_t* edge_outlier, const uint8_t* flags, int discard, int32_t* ids_out,
                                uint8_t* outlier_out, int32_t* counts)
{
    int m = 0, nMatches = 0, nMap = 0;
    for (int t = 0; t < n; t++) {
        const int32_t id = merged[t];
        ids_out[t] = id; outlier_out[t] = 0;
        if (id < 0) continue;
        const uint8_t o = edge_outlier[m++];
        outlier_out[t] = o;
        if (o) { if (discard) ids_out[t] = -1; }
        else { nMatches++; if (flags[id] & 2) nMap++; }
    }
    counts[0] = nMatches; counts[1] = nMap;
}

}  // extern "C"
