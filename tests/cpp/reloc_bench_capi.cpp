// The parent commit's way around the body of Tracking::Relocalization behind PnPsolver::iterate as ONE C entry, for
// tools/reloc_bench.py (built by tests/ref_shim.py): what a C++ caller would write on the entries that existed before
// orbq_relocalize.  Per stage ONE orbo_pose_optimize_frames over the jobs still running, the host discard and the gates between the
// stages, the host projection of the candidate's row over flat host copies of the pool (no pointer chasing: the kindest host form),
// and one resident mode-5 search a job (orbm_track_frame_projected + orbm_track_results).  Every array and pointer is the caller's,
// made once; the library's entries come in as function pointers (the shim is not linked against it).  The keyframe's slot holds, per
// row entry, the descriptor of the entry's point: orbm_track_frame_projected takes the query descriptors from that slot.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" {

typedef int (*PoseOptFn)(void* h, const void* frames, void* const* resident, int n_frames, const int32_t* edge_start, const void* edges,
                         const float* inv_level_sigma2, int nlevels, void* out, uint8_t* outlier);
struct ProjParams { int32_t mode; float nnratio; int32_t check_ori, th_dist; };
typedef int (*TrackProjectedFn)(void* fs, int cur_slot, int last_slot, const ProjParams* pp, const float* q_uvr, const int8_t* q_lvl, const uint8_t* qvalid,
                                const uint8_t* q_obs_pos, int nq, const uint8_t* t_occ);
typedef int (*TrackResultsFn)(void* fs, int back, const int32_t** assign, const int32_t** nmatches, int* npairs, int* cap);

struct Opt { float Tcw[16]; int32_t nInitial, nGood, rounds, iterations[4], trials[4], pad; double lambda[4], chi2[4]; };   // OrboResult
struct Res { Opt opt[3]; float Tcw[16]; int32_t exit, nGood[3], nAdditional[2]; };                                          // OrbqRelocResult
struct FrameRec { float Tcw[16]; float K[4]; };                                                                             // OrboFrame
struct Edge { int32_t feature; float Xw[3]; };                                                                              // OrboEdge

struct ParentWay {
    PoseOptFn poseOpt; TrackProjectedFn trackProjected; TrackResultsFn trackResults;
    void* h;
    int32_t J, n, stride, cap, nlevels, checkOri;
    // the jobs
    void* const* fs; const int32_t* slot; const int32_t* kfSlot; void* const* resident;
    const int32_t* const* entries; const int32_t* const* idsIn; const float* TcwIn; const float* K;
    // the pool, flat host copies; the tables; the image bounds
    const float* pos; const float* minD; const float* maxD; const uint8_t* flags; int32_t poolCap;
    const float* sig; const float* sf; const float* breaks; const float* bounds;
    // scratch
    FrameRec* frames; void** residentLive; Edge* edges; int32_t* start; Opt* optOut; uint8_t* eflags; int32_t* live;
    float* uvr; int8_t* lvl; uint8_t* qv; uint8_t* occ; uint8_t* mark;   // [3 stride], [2 stride], [stride], [cap], [poolCap] (all zero between calls)
    // outputs
    Res* out; int32_t* idsOut; uint8_t* outlierOut; uint8_t* status;     // [J], [J][n], [J][n], [J][2][stride]
};

enum { kRejected = 0, kFirst, kWideShort, kSecond, kNarrowShort, kThird };
enum { kNoPoint = 1, kBad, kFound, kOutOfImage, kDistance, kLevelRange, kInView };
static const int32_t kNoVote = 1 << 30;

// ORBmatcher.cc:1490-1530 for every entry of job j's row at the pose the job holds; `mark` says which points are in sFound
static void project(const ParentWay* w, int j, float th, uint8_t* st)
{
    const float* T = w->out[j].Tcw;
    const int32_t* ent = w->entries[j];
    float Ow[3];
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)T[4 * k + i] * (double)T[4 * k + 3];
        Ow[i] = (float)(s * -1.0);
    }
    for (int q = 0; q < w->stride; q++) {
        float u = 0.f, v = 0.f, rad = 0.f;
        int level = -1;
        uint8_t s = kNoPoint;
        const int32_t e = ent[q], id = e & ~kNoVote;
        if (e >= 0 && id < w->poolCap) {
            s = kBad;
            if (!(w->flags[id] & 1)) {
                s = kFound;
                if (!w->mark[id]) {
                    const float* X = w->pos + 3 * (size_t)id;
                    float pc[3];
                    for (int i = 0; i < 3; i++) {
                        const float t = T[4 * i] * X[0] + T[4 * i + 1] * X[1] + T[4 * i + 2] * X[2];
                        pc[i] = (float)((double)t * 1.0 + (double)T[4 * i + 3] * 1.0);
                    }
                    const float invzc = (float)(1.0 / (double)pc[2]);
                    u = w->K[0] * pc[0] * invzc + w->K[2]; v = w->K[1] * pc[1] * invzc + w->K[3];
                    s = kOutOfImage;
                    if (u >= w->bounds[0] && u <= w->bounds[1] && v >= w->bounds[2] && v <= w->bounds[3]) {
                        const float PO[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
                        const float dist = (float)std::sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
                        s = kDistance;
                        if (!(dist < 0.8f * w->minD[id] || dist > 1.2f * w->maxD[id])) {
                            const float ratio = w->maxD[id] / dist;
                            int c = 0;
                            for (int k = 0; k <= w->nlevels; k++) c += ratio > w->breaks[k] ? 1 : 0;
                            level = c - 1;
                            s = kLevelRange;
                            if (c >= 1 && c <= w->nlevels) { s = kInView; rad = th * w->sf[level]; }
                        }
                    }
                }
            }
        }
        w->uvr[3 * q] = u; w->uvr[3 * q + 1] = v; w->uvr[3 * q + 2] = rad;
        w->lvl[2 * q] = (int8_t)(level - 1); w->lvl[2 * q + 1] = (int8_t)(level + 1);
        w->qv[q] = s == kInView;
        st[q] = s;
    }
}

// Returns the first non-zero code of the library
int relocbench_parent_way(const ParentWay* w)
{
    const int n = w->n, J = w->J;
    int nLive = 0;
    for (int j = 0; j < J; j++) {
        memset(&w->out[j], 0, sizeof(Res));
        memcpy(w->out[j].Tcw, w->TcwIn + 16 * (size_t)j, 64);
        memcpy(w->idsOut + (size_t)j * n, w->idsIn[j], (size_t)n * 4);
        memset(w->outlierOut + (size_t)j * n, 0xff, (size_t)n);
        memset(w->status + (size_t)j * 2 * w->stride, 0, (size_t)2 * w->stride);
        w->live[nLive++] = j;
    }
    for (int stage = 0; stage < 3; stage++) {
        if (stage > 0) {
            // one resident search a job: the projection on the host, orbm_track_frame_projected, orbm_track_results
            const int sidx = stage - 1;
            const ProjParams pp = {5, 0.9f, w->checkOri, sidx == 0 ? 100 : 64};
            int keep = 0;
            for (int k = 0; k < nLive; k++) {
                const int j = w->live[k];
                int32_t* cur = w->idsOut + (size_t)j * n;
                // sFound: the ids as they came (Tracking.cc:1497), or every point the frame holds (:1526-1528)
                const int32_t* found = sidx == 0 ? w->idsIn[j] : cur;
                for (int t = 0; t < n; t++) if (found[t] >= 0) w->mark[found[t]] = 1;
                project(w, j, sidx == 0 ? 10.f : 3.f, w->status + ((size_t)2 * j + sidx) * w->stride);
                for (int t = 0; t < n; t++) if (found[t] >= 0) w->mark[found[t]] = 0;
                for (int t = 0; t < w->cap; t++) w->occ[t] = t >= n || cur[t] >= 0;
                if (int rc = w->trackProjected(w->fs[j], w->slot[j], w->kfSlot[j], &pp, w->uvr, w->lvl, w->qv, nullptr, w->stride, w->occ)) return rc;
                const int32_t *assign = nullptr, *nm = nullptr;
                if (int rc = w->trackResults(w->fs[j], 0, &assign, &nm, nullptr, nullptr)) return rc;
                for (int t = 0; t < n; t++) if (assign[t] >= 0) cur[t] = w->entries[j][assign[t]] & ~kNoVote;   // ORBmatcher.cc:1559
                Res& R = w->out[j];
                R.nAdditional[sidx] = nm[0];
                if (nm[0] + R.nGood[sidx] < 50) { R.exit = sidx == 0 ? kWideShort : kNarrowShort; continue; }   // :1517 / :1532
                w->live[keep++] = j;
            }
            nLive = keep;
        }
        if (!nLive) break;
        // ONE orbo_pose_optimize_frames over the jobs still running
        int m = 0;
        w->start[0] = 0;
        for (int k = 0; k < nLive; k++) {
            const int j = w->live[k];
            const int32_t* cur = w->idsOut + (size_t)j * n;
            memcpy(w->frames[k].Tcw, w->out[j].Tcw, 64);
            memcpy(w->frames[k].K, w->K, 16);
            w->residentLive[k] = w->resident[j];
            for (int t = 0; t < n; t++) {
                const int32_t id = cur[t];
                if (id < 0) continue;
                w->edges[m].feature = t;
                memcpy(w->edges[m].Xw, w->pos + 3 * (size_t)id, 12);
                m++;
            }
            w->start[k + 1] = m;
        }
        if (int rc = w->poseOpt(w->h, w->frames, w->residentLive, nLive, w->start, w->edges, w->sig, w->nlevels, w->optOut, w->eflags)) return rc;
        int keep = 0;
        for (int k = 0; k < nLive; k++) {
            const int j = w->live[k];
            Res& R = w->out[j];
            int32_t* cur = w->idsOut + (size_t)j * n;
            uint8_t* outl = w->outlierOut + (size_t)j * n;
            R.opt[stage] = w->optOut[k];
            memcpy(R.Tcw, R.opt[stage].Tcw, 64);
            const int nGood = R.opt[stage].nGood;
            R.nGood[stage] = nGood;
            const bool discard = stage == 0 ? nGood >= 10 : stage == 2;   // :1505 leaves before :1508-1510; :1519 discards nothing; :1536-1538
            const uint8_t* eo = w->eflags + w->start[k];
            int e = 0;
            for (int t = 0; t < n; t++) {
                if (cur[t] < 0) continue;
                const uint8_t o = eo[e++];
                outl[t] = o ? 1 : 0;
                if (o && discard) cur[t] = -1;
            }
            int exit = -1;
            if (stage == 0) exit = nGood < 10 ? kRejected : nGood >= 50 ? kFirst : -1;
            else if (stage == 1) exit = nGood >= 50 || nGood <= 30 ? kSecond : -1;
            else exit = kThird;
            if (exit >= 0) { R.exit = exit; continue; }
            w->live[keep++] = j;
        }
        nLive = keep;
    }
    return 0;
}

int relocbench_sizeof(void) { return (int)sizeof(ParentWay); }
int relocbench_sizeof_res(void) { return (int)sizeof(Res); }

}  // extern "C"
