// C shim over tools/fuse_ref.hpp for the Python checkers (tests/fuse_cases.py; built by tests/ref_shim.py).
#include "../../tools/fuse_ref.hpp"

using namespace fuse_ref;

extern "C" {

int fuseref_sizes(int i)
{
    return i == 0 ? (int)sizeof(Target) : i == 1 ? (int)sizeof(Point) : i == 2 ? (int)sizeof(Result) : i == 3 ? (int)sizeof(KeyPt) : (int)sizeof(Gates);
}

// :855-892 of the points idx[0..m) of the pool against one target; gates may be null
void fuseref_project(const Target* T, const Point* pool, const int32_t* idx, int m, float th, const float* sf, int nlevels, float lsf,
                     Result* out, Gates* gates)
{
    for (int i = 0; i < m; i++) project(*T, pool[idx[i]], th, sf, nlevels, lsf, out[i], gates ? gates + i : nullptr);
}

// :855-951 of the same, with the restatement's own grid and window walk
void fuseref_target(const Target* T, const KeyPt* keys, const uint8_t* desc, int n, const Point* pool, const int32_t* idx, int m, float th,
                    const float* sf, const float* invSigma2, int nlevels, float lsf, Result* out)
{
    CellGrid grid;
    grid.build(T->grid, keys, n);
    for (int i = 0; i < m; i++) out[i] = pair(*T, grid, keys, desc, pool[idx[i]], th, sf, invSigma2, nlevels, lsf);
}

// the break table against the direct formula over every float whose bit pattern lies in [lo, hi]: the count of floats
// where they disagree, and the first such pattern
int64_t fuseref_level_sweep(float lsf, int nlevels, const float* breaks, uint32_t lo, uint32_t hi, uint32_t* first_bad)
{
    int64_t bad = 0;
    for (uint64_t b = lo; b <= hi; b++) {
        const uint32_t bits = (uint32_t)b;
        float ratio;
        std::memcpy(&ratio, &bits, 4);
        int c = 0;
        for (int j = 0; j <= nlevels; j++) c += ratio > breaks[j] ? 1 : 0;
        const float lv = predictLevel(ratio, lsf);
        const int want = !(lv >= 0.f) ? -1 : !(lv < (float)nlevels) ? nlevels : (int)lv;
        if (c - 1 != want) { if (!bad && first_bad) *first_bad = bits; bad++; }
    }
    return bad;
}

// ------------------------------------------------------------------------------------------------ the serial map model
void* fuseref_model_new(float th, const float* sf, const float* invSigma2, int nlevels, float lsf)
{
    Model* m = new Model();
    m->th = th; m->sf.assign(sf, sf + nlevels); m->invSigma2.assign(invSigma2, invSigma2 + nlevels); m->logScaleFactor = lsf;
    return m;
}
void fuseref_model_free(void* m) { delete (Model*)m; }
int fuseref_add_keyframe(void* m, const Target* T, const KeyPt* keys, const uint8_t* desc, int n) { return ((Model*)m)->addKeyFrame(*T, keys, desc, n); }
void fuseref_set_covisibles(void* m, int kf, const int32_t* ids, int n) { ((Model*)m)->kfs[kf].covis.assign(ids, ids + n); }
int fuseref_add_map_point(void* m, const Point* P) { return ((Model*)m)->addMapPoint(*P); }
void fuseref_add_observation(void* m, int mp, int kf, int idx)
{
    Model* M = (Model*)m;
    M->addObservation(mp, kf, idx);
    M->kfs[kf].slot[idx] = mp;
}
// SearchInNeighbors(cur): the target list into targets (capacity tcap), the Replace / AddObservation sequence into events
// (capacity ecap records of four ints); the counts come back through n_targets / n_events
void fuseref_search_in_neighbors(void* m, int cur, int32_t* targets, int tcap, int* n_targets, int32_t* events, int ecap, int* n_events)
{
    Model* M = (Model*)m;
    std::vector<int> t;
    M->events.clear();
    M->searchInNeighbors(cur, t);
    *n_targets = (int)t.size();
    for (int i = 0; i < (int)t.size() && i < tcap; i++) targets[i] = t[i];
    *n_events = (int)M->events.size();
    for (int i = 0; i < (int)M->events.size() && i < ecap; i++) std::memcpy(events + 4 * i, &M->events[i], 16);
}
void fuseref_keyframe_slots(void* m, int kf, int32_t* out)
{
    const Model::KF& K = ((Model*)m)->kfs[kf];
    for (size_t i = 0; i < K.slot.size(); i++) out[i] = K.slot[i];
}
// bad flag, mpReplaced, the descriptor, and the observations as (keyframe, feature) pairs in insertion order
int fuseref_map_point(void* m, int mp, int* bad, int* replaced, uint8_t* desc, int32_t* obs, int cap)
{
    const Model::MP& P = ((Model*)m)->mps[mp];
    *bad = P.bad; *replaced = P.replaced;
    std::memcpy(desc, P.rec.desc, 32);
    for (int i = 0; i < (int)P.obs.size() && i < cap; i++) { obs[2 * i] = P.obs[i].first; obs[2 * i + 1] = P.obs[i].second; }
    return (int)P.obs.size();
}

}  // extern "C"
