// C shim over tools/reloc_ref.hpp for the Python checkers (tests/reloc_cases.py; built by tests/ref_shim.py).
#include "../../tools/reloc_ref.hpp"

using namespace reloc_ref;

extern "C" {

// everything a job reads, as ctypes fills it (tests/reloc_cases.py: RelocRefArgs)
struct RelocRefArgs {
    const float* pos; const float* minD; const float* maxD; const uint8_t* flags; const uint8_t* pdesc; int32_t cap;
    const Key* keys; const uint8_t* desc; int32_t nKeys;
    Grid grid; float bounds[4];
    const int32_t* entries; int32_t nEntries, stride; const float* angles; int32_t nAngles;
    const float* invSigma2; const float* sf; const float* breaks; int32_t nlevels;
    const int32_t* ids; int32_t n;
    float Tcw[16]; float K[4];
    int32_t checkOri;
};

int relocref_sizes(int i) { return i == 0 ? (int)sizeof(Key) : i == 1 ? (int)sizeof(Result) : i == 2 ? (int)sizeof(Branches) : (int)sizeof(RelocRefArgs); }

// one job; the counters are ADDED to br.  Returns 0, or -1 for what the device refuses behind its kernels
int relocref_run(const RelocRefArgs* a, Result* out, int32_t* ids_out, uint8_t* outlier_out, uint8_t* status, Branches* br)
{
    const Pool P = {a->pos, a->minD, a->maxD, a->flags, a->pdesc, a->cap};
    Frame F;
    F.keys = a->keys; F.desc = a->desc; F.nKeys = a->nKeys; F.grid = a->grid;
    for (int i = 0; i < 4; i++) F.bounds[i] = a->bounds[i];
    const KeyFrame kf = {a->entries, a->nEntries, a->stride, a->angles, a->nAngles};
    const Levels L = {a->invSigma2, a->sf, a->breaks, a->nlevels};
    return relocalize(P, F, kf, L, a->ids, a->n, a->Tcw, a->K, a->checkOri, *out, ids_out, outlier_out, status, *br);
}

int relocref_n_good(const Result* r) { return nGoodAtExit(*r); }
int relocref_verdict(const Result* r) { return verdict(*r) ? 1 : 0; }

}  // extern "C"
