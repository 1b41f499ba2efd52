// The parent commit's way around Tracking::TrackReferenceKeyFrame as ONE C entry, for tools/trackref_bench.py (built by
// tests/ref_shim.py): what a C++ caller would write on the entries that existed before orbq_track_reference.  Every array and
// pointer is the caller's, made once; the library's entries come in as function pointers (the shim is not linked against it).
#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" {

typedef int (*BowFramesFn)(void* fs, const int32_t* kf_slots, const int32_t* frame_slots, int npairs, float nnratio, int check_ori);
typedef int (*BowResultsFn)(void* fs, int back, const int32_t** match, const int32_t** nmatches, int* npairs, int* cap);
typedef int (*PoseOptFn)(void* h, const void* frames, void* const* resident, int n_frames, const int32_t* edge_start, const void* edges,
                         const float* inv_level_sigma2, int nlevels, void* out, uint8_t* outlier);

struct ParentWay {
    BowFramesFn bowFrames; BowResultsFn bowResults; PoseOptFn poseOpt;
    void* h;
    // the searches: call c covers the pairs [call_start[c], call_start[c + 1]) of kf_slots / frame_slots on frame set call_fs[c];
    // pair i is job job_of[i]
    int32_t ncalls; void* const* call_fs; const int32_t* call_start; const int32_t* kf_slots; const int32_t* frame_slots; const int32_t* job_of;
    float nnratio; int32_t check_ori;
    // the jobs
    int32_t J, n;
    const int32_t* const* entries;   // per job: the keyframe's match list as pool ids, a flat host copy
    const float* pos; const uint8_t* flags;   // the pool, flat host copies
    const void* frames; void* const* resident; const float* sig; int32_t nlevels;
    // scratch and outputs
    const int32_t** tables;          // [J]
    int32_t* merged;                 // [J][n]
    void* edges; int32_t* start;     // [J * n] records of {feature, Xw[3]}, [J + 1]
    void* out; uint8_t* eflags;      // [J] OrboResult, one byte an edge
    int32_t* nbow; int32_t* ids_out; uint8_t* outlier_out; int32_t* counts;   // [J], [J][n], [J][n], [J][2]
    int32_t* match_copy;             // [J][n], or null: the tables stay where orbm_bow_results left them
};

// orbm_bow_frames + orbm_bow_results per frame set, the merge through the match list and the gather of Xw, ONE
// orbo_pose_optimize_frames, the walk over mvbOutlier with the discard and the two counts.  Returns the first non-zero code
int trackrefbench_parent_way(const ParentWay* w)
{
    struct E { int32_t feature; float Xw[3]; };
    const int n = w->n;
    for (int c = 0; c < w->ncalls; c++) {
        const int i0 = w->call_start[c], np = w->call_start[c + 1] - i0;
        if (int rc = w->bowFrames(w->call_fs[c], w->kf_slots + i0, w->frame_slots + i0, np, w->nnratio, w->check_ori)) return rc;
    }
    for (int c = 0; c < w->ncalls; c++) {
        const int i0 = w->call_start[c], np = w->call_start[c + 1] - i0;
        const int32_t *match = nullptr, *nm = nullptr;
        int cap = 0;
        if (int rc = w->bowResults(w->call_fs[c], 0, &match, &nm, nullptr, &cap)) return rc;
        for (int i = 0; i < np; i++) { const int j = w->job_of[i0 + i]; w->tables[j] = match + (size_t)i * cap; w->nbow[j] = nm[i]; }
    }
    E* e = (E*)w->edges;
    int m = 0;
    w->start[0] = 0;
    for (int j = 0; j < w->J; j++) {
        const int32_t* table = w->tables[j];
        const int32_t* ent = w->entries[j];
        int32_t* merged = w->merged + (size_t)j * n;
        if (w->match_copy) memcpy(w->match_copy + (size_t)j * n, table, (size_t)n * 4);
        for (int t = 0; t < n; t++) {
            const int32_t id = table[t] >= 0 ? ent[table[t]] : -1;
            merged[t] = id;
            if (id < 0) continue;
            e[m].feature = t; e[m].Xw[0] = w->pos[3 * (size_t)id]; e[m].Xw[1] = w->pos[3 * (size_t)id + 1]; e[m].Xw[2] = w->pos[3 * (size_t)id + 2];
            m++;
        }
        w->start[j + 1] = m;
    }
    if (int rc = w->poseOpt(w->h, w->frames, w->resident, w->J, w->start, w->edges, w->sig, w->nlevels, w->out, w->eflags)) return rc;
    for (int j = 0; j < w->J; j++) {
        const int32_t* merged = w->merged + (size_t)j * n;
        int32_t* ids = w->ids_out + (size_t)j * n;
        uint8_t* outl = w->outlier_out + (size_t)j * n;
        const uint8_t* eo = w->eflags + w->start[j];
        int k = 0, nMatches = 0, nMap = 0;
        for (int t = 0; t < n; t++) {
            const int32_t id = merged[t];
            ids[t] = id; outl[t] = 0;
            if (id < 0) continue;
            const uint8_t o = eo[k++];
            outl[t] = o;
            if (o) ids[t] = -1;
            else { nMatches++; if (w->flags[id] & 2) nMap++; }
        }
        w->counts[2 * j] = nMatches; w->counts[2 * j + 1] = nMap;
    }
    return 0;
}

int trackrefbench_sizeof(void) { return (int)sizeof(ParentWay); }

}  // extern "C"
