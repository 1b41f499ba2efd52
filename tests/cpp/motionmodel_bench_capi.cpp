// The parent commit's way around Tracking::TrackWithMotionModel (Tracking.cc:925-969) as ONE C entry, for tools/motionmodel_bench.py
// (built by tests/ref_shim.py): what a C++ caller would write on the entries that existed before orbq_track_motion_model.  Per job the
// host product mVelocity * mLastFrame.mTcw and the view record, orbw_track_frame_pose and orbm_track_results (the wait that lets the
// host compare nmatches with 20), both again with 2 * th below 20; then ONE orbq_track_pose over the jobs that passed the gate (the
// kindest form: the solves are batched).  Every job has a frame set of its own (the last frame in slot 0, the current one in slot 1),
// so `back` is 0 for all.  Every array and pointer is the caller's, made once; the library's entries come in as function pointers (the
// shim is not linked against it).
#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" {

struct ProjParams { int32_t mode; float nnratio; int32_t check_ori, th_dist; };                                              // OrbmProjParams
struct View { float Rcw[9], tcw[3], Ow[3], K[4], min_x, max_x, min_y, max_y, viewing_cos_limit; };                           // OrbwView
struct Opt { float Tcw[16]; int32_t nInitial, nGood, rounds, iterations[4], trials[4], pad; double lambda[4], chi2[4]; };    // OrboResult
struct TrackRes { Opt opt; int32_t nMatches, nMatchesMap; };                                                                 // OrbqResult
struct TrackJob { void* fs; int32_t slot, back; const int32_t* base; int32_t n, discard; float Tcw[16]; float K[4]; };       // OrbqJob
typedef int (*TrackFramePoseFn)(void* fs, int cur_slot, int last_slot, void* pool, const ProjParams* pp, const View* view, const int32_t* last_ids, int nq,
                                float th, const float* scale_factors, const uint8_t* t_occ);
typedef int (*TrackResultsFn)(void* fs, int back, const int32_t** assign, const int32_t** nmatches, int* npairs, int* cap);
typedef int (*TrackPoseFn)(void* h, void* pool, const TrackJob* jobs, int n_jobs, const float* inv_level_sigma2, int nlevels, TrackRes* out,
                           int32_t* const* ids_out, uint8_t* const* outlier_out);

struct ParentWay {
    TrackFramePoseFn trackFramePose; TrackResultsFn trackResults; TrackPoseFn trackPose;
    void* h; void* pool;
    int32_t J, n, nq, nlevels, minMatches; float th;
    // the jobs
    void* const* fs; const int32_t* const* lastIds; const float* velocity; const float* lastTcw; const float* K; const float* bounds;
    const float* sig; const float* sf;
    // scratch
    TrackJob* tjobs; TrackRes* tout; int32_t** idsPtr; uint8_t** outlPtr; int32_t* which;
    // outputs
    float* TcwPred; int32_t* nSearch; int32_t* wide; int32_t* status; TrackRes* out; int32_t* idsOut; uint8_t* outlierOut; int32_t* assignOut;   // [J][16], [J][2], [J], [J], [J], [J][n] x 3
};

int motionbench_sizeof() { return (int)sizeof(ParentWay); }
int motionbench_sizeof_res() { return (int)sizeof(TrackRes); }

int motionbench_parent_way(const ParentWay* w)
{
    const ProjParams pp = {4, 0.9f, 1, 100};
    int nt = 0;
    for (int j = 0; j < w->J; j++) {
        const float* V = w->velocity + 16 * j;
        const float* T = w->lastTcw + 16 * j;
        float* P = w->TcwPred + 16 * j;
        for (int r = 0; r < 4; r++)   // Tracking.cc:925
            for (int c = 0; c < 4; c++) {
                const float s = V[4 * r] * T[c] + V[4 * r + 1] * T[4 + c] + V[4 * r + 2] * T[8 + c] + V[4 * r + 3] * T[12 + c];
                P[4 * r + c] = (float)((double)s * 1.0);
            }
        View view;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) view.Rcw[3 * r + c] = P[4 * r + c]; view.tcw[r] = P[4 * r + 3]; }
        for (int r = 0; r < 3; r++) {   // Frame.cc:258-267
            double s = 0;
            for (int c = 0; c < 3; c++) s += (double)view.Rcw[3 * c + r] * (double)view.tcw[c];
            view.Ow[r] = -(float)s;
        }
        memcpy(view.K, w->K, sizeof view.K);
        view.min_x = w->bounds[0]; view.max_x = w->bounds[1]; view.min_y = w->bounds[2]; view.max_y = w->bounds[3]; view.viewing_cos_limit = 0.5f;
        const int32_t* assign = nullptr; const int32_t* nm = nullptr;
        int rc = w->trackFramePose(w->fs[j], 1, 0, w->pool, &pp, &view, w->lastIds[j], w->nq, w->th, w->sf, nullptr);   // :935
        if (rc || (rc = w->trackResults(w->fs[j], 0, &assign, &nm, nullptr, nullptr))) return rc;
        int nmatches = nm[0];
        w->nSearch[2 * j] = nmatches; w->nSearch[2 * j + 1] = -1; w->wide[j] = 0;
        if (nmatches < w->minMatches) {   // :938-942
            rc = w->trackFramePose(w->fs[j], 1, 0, w->pool, &pp, &view, w->lastIds[j], w->nq, 2.0f * w->th, w->sf, nullptr);
            if (rc || (rc = w->trackResults(w->fs[j], 0, &assign, &nm, nullptr, nullptr))) return rc;
            nmatches = nm[0];
            w->nSearch[2 * j + 1] = nmatches; w->wide[j] = 1;
        }
        int32_t* asg = w->assignOut + (size_t)j * w->n;
        memcpy(asg, assign, (size_t)w->n * 4);
        if (nmatches < w->minMatches) {   // :944
            w->status[j] = 1;
            memset(&w->out[j], 0, sizeof(TrackRes));
            memcpy(w->out[j].opt.Tcw, P, 64);
            w->out[j].nMatches = nmatches;
            for (int t = 0; t < w->n; t++) { w->idsOut[(size_t)j * w->n + t] = asg[t] >= 0 ? w->lastIds[j][asg[t]] : -1; w->outlierOut[(size_t)j * w->n + t] = 0; }
            continue;
        }
        w->status[j] = 0;
        TrackJob& q = w->tjobs[nt];
        q.fs = w->fs[j]; q.slot = 1; q.back = 0; q.base = nullptr; q.n = w->n; q.discard = 1;
        memcpy(q.Tcw, P, 64); memcpy(q.K, w->K, 16);
        w->idsPtr[nt] = w->idsOut + (size_t)j * w->n; w->outlPtr[nt] = w->outlierOut + (size_t)j * w->n;
        w->which[nt++] = j;
    }
    if (nt) {   // :948-969
        const int rc = w->trackPose(w->h, w->pool, w->tjobs, nt, w->sig, w->nlevels, w->tout, w->idsPtr, w->outlPtr);
        if (rc) return rc;
        for (int k = 0; k < nt; k++) w->out[w->which[k]] = w->tout[k];
    }
    return 0;
}

}  // extern "C"
