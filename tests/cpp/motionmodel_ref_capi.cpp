// C shim over tools/motionmodel_ref.hpp for the Python checkers (tests/motionmodel_cases.py; built by tests/ref_shim.py).
#include "../../tools/motionmodel_ref.hpp"

using namespace motionmodel_ref;

extern "C" {

// everything a job reads, as ctypes fills it (tests/motionmodel_cases.py: MotionRefArgs)
struct MotionRefArgs {
    const float* pos; const uint8_t* flags; int32_t cap;
    const Key* keys; const uint8_t* desc; int32_t nKeys;
    reloc_ref::Grid grid; float bounds[4];
    const Key* lastKeys; const uint8_t* lastDesc; int32_t nLastKeys;
    const float* invSigma2; const float* sf; int32_t nlevels;
    const int32_t* lastIds; int32_t nq, n;
    float velocity[16], lastTcw[16], K[4];
    float th; int32_t minMatches, checkOri;
};

int motionref_sizes(int i) { return i == 0 ? (int)sizeof(Key) : i == 1 ? (int)sizeof(Result) : i == 2 ? (int)sizeof(Branches) : (int)sizeof(MotionRefArgs); }

// one job; the counters are ADDED to br.  Returns 0, or -1 for what the device refuses behind its kernels
int motionref_run(const MotionRefArgs* a, Result* out, int32_t* ids_out, uint8_t* outlier_out, int32_t* assign_out, uint8_t* status, Branches* br)
{
    const Pool P = {a->pos, a->flags, a->cap};
    Frame F;
    F.keys = a->keys; F.desc = a->desc; F.nKeys = a->nKeys; F.grid = a->grid;
    for (int i = 0; i < 4; i++) F.bounds[i] = a->bounds[i];
    const Last last = {a->lastKeys, a->lastDesc, a->nLastKeys};
    const Levels L = {a->invSigma2, a->sf, a->nlevels};
    return trackWithMotionModel(P, F, last, L, a->lastIds, a->nq, a->n, a->velocity, a->lastTcw, a->K, a->th, a->minMatches, a->checkOri, *out,
                                ids_out, outlier_out, assign_out, status, *br);
}

void motionref_pose_product(const float* V, const float* T, float* out) { poseProduct(V, T, out); }

}  // extern "C"
