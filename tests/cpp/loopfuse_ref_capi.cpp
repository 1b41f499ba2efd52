// C shim over tools/loopfuse_ref.hpp for the Python checkers (tests/loopfuse_cases.py; built by tests/ref_shim.py).
#include "../../tools/loopfuse_ref.hpp"

using namespace loopfuse_ref;

extern "C" {

int loopref_sizes(int i)
{
    return i == 0 ? (int)sizeof(Target) : i == 1 ? (int)sizeof(Point) : i == 2 ? (int)sizeof(Result) : i == 3 ? (int)sizeof(KeyPt) : i == 4 ? (int)sizeof(Gates)
                                                                                                                                            : (int)sizeof(Hit);
}

// :1010-1051 of the points [0, m) of the pool against one target; gates may be null
void loopref_project(const Target* T, const Point* pool, int m, float th, const float* sf, int nlevels, float lsf, Result* out, Gates* gates)
{
    for (int i = 0; i < m; i++) project(*T, pool[i], th, sf, nlevels, lsf, out[i], gates ? gates + i : nullptr);
}

// :1010-1081 of the same, with the restatement's own grid and window walk
void loopref_target(const Target* T, const KeyPt* keys, const uint8_t* desc, int n, const Point* pool, int m, float th, const float* sf, int nlevels,
                    float lsf, Result* out)
{
    CellGrid grid;
    grid.build(T->grid, keys, n);
    for (int i = 0; i < m; i++) out[i] = pair(*T, grid, keys, desc, pool[i], th, sf, nlevels, lsf);
}

// `1.0/z` rounded to float against the float division over the floats whose bit patterns are lo, lo + step, ... <= hi: the
// count of patterns where the two differ as bits, and the first such pattern
int64_t loopref_invz_sweep(uint32_t lo, uint32_t hi, uint32_t step, uint32_t* first_bad)
{
    int64_t bad = 0;
    for (uint64_t b = lo; b <= hi; b += step) {
        const uint32_t bits = (uint32_t)b;
        float z;
        std::memcpy(&z, &bits, 4);
        volatile float zz = z;   // (the division is done at run time, in the target's float arithmetic)
        const float a = invzAsWritten(zz), c = invzFloatDivision(zz);
        if (std::memcmp(&a, &c, 4) != 0 && !(a != a && c != c)) { if (!bad && first_bad) *first_bad = bits; bad++; }
    }
    return bad;
}

// ------------------------------------------------------------------------------------------------ the serial map model
void* loopref_model_new(const float* sf, int nlevels, float lsf)
{
    Model* m = new Model();
    m->sf.assign(sf, sf + nlevels); m->logScaleFactor = lsf;
    return m;
}
void loopref_model_free(void* m) { delete (Model*)m; }
int loopref_add_keyframe(void* m, const Grid* g, const KeyPt* keys, const uint8_t* desc, int n) { return ((Model*)m)->addKeyFrame(*g, keys, desc, n); }
int loopref_add_map_point(void* m, const Point* P) { return ((Model*)m)->addMapPoint(*P); }
void loopref_add_observation(void* m, int mp, int kf, int idx)
{
    Model* M = (Model*)m;
    M->addObservation(mp, kf, idx);
    M->kfs[kf].slot[idx] = mp;
}
// SearchAndFuse over the targets (kf[t], rec[t]) and the loop points.  mode 0: the serial loop; 1: the parallel rule; 2: the
// parallel rule WITHOUT the re-score of survivors.  Returns the total of nFused; the Replace / AddObservation sequence goes
// into events (capacity ecap records of four ints), the pairs scored again into rescored
int loopref_search_and_fuse(void* m, int mode, const int32_t* kf, const Target* rec, int nt, const int32_t* loop, int nl, float th, int32_t* events,
                            int ecap, int* n_events, int64_t* rescored)
{
    Model* M = (Model*)m;
    std::vector<Model::Corrected> c((size_t)nt);
    for (int t = 0; t < nt; t++) { c[t].kf = kf[t]; c[t].rec = rec[t]; }
    const std::vector<int> lp(loop, loop + nl);
    M->events.clear();
    M->rescored = 0;
    const int total = mode == 0 ? M->searchAndFuse(c, lp, th) : M->searchAndFuseByRule(c, lp, th, mode == 1);
    *n_events = (int)M->events.size();
    for (int i = 0; i < (int)M->events.size() && i < ecap; i++) std::memcpy(events + 4 * i, &M->events[i], 16);
    if (rescored) *rescored = M->rescored;
    return total;
}
void loopref_keyframe_slots(void* m, int kf, int32_t* out)
{
    const Model::KF& K = ((Model*)m)->kfs[kf];
    for (size_t i = 0; i < K.slot.size(); i++) out[i] = K.slot[i];
}
// bad flag, mpReplaced, the descriptor, and the observations as (keyframe, feature) pairs in insertion order
int loopref_map_point(void* m, int mp, int* bad, int* replaced, uint8_t* desc, int32_t* obs, int cap)
{
    const Model::MP& P = ((Model*)m)->mps[mp];
    *bad = P.bad; *replaced = P.replaced;
    std::memcpy(desc, P.rec.desc, 32);
    for (int i = 0; i < (int)P.obs.size() && i < cap; i++) { obs[2 * i] = P.obs[i].first; obs[2 * i + 1] = P.obs[i].second; }
    return (int)P.obs.size();
}

}  // extern "C"
