// newpoints_ref_capi.cpp -- C entry points over the CreateNewMapPoints restatement (tools/newpoints_ref.hpp) for the tests
// and tools/newpoints_bench.py (ctypes); built with g++ -ffp-contract=off through tests/ref_shim.py.
#include "../../tools/newpoints_ref.hpp"

using namespace newpoints_ref;

extern "C" {

void npref_compute_f12(const KeyFrame* k1, const KeyFrame* k2, float* F12, float* epipole) { computeF12(*k1, *k2, F12, epipole); }
int npref_baseline_too_short(const KeyFrame* k1, const KeyFrame* k2) { return baselineTooShort(*k1, *k2) ? 1 : 0; }
// one pair: the status code; on ACCEPTED out holds pos, normal and the distances; dbg (9 floats, may be null): the gates' quantities
int npref_pair(const KeyFrame* k1, const KeyFrame* k2, const KeyPt* kp1, const KeyPt* kp2, const float* scaleFactors, const float* levelSigma2,
               int nlevels, float scaleFactor, NewPoint* out, float* dbg)
{
    return pair(*k1, *k2, *kp1, *kp2, scaleFactors, levelSigma2, nlevels, 1.5f * scaleFactor, *out, dbg);
}
// one pass of the serial neighbour loop (skip1 is updated); returns the number of points appended to out
int npref_neighbour(int k, const KeyFrame* k1, const KeyFrame* k2, const KeyPt* keys1, int n1, const KeyPt* keys2, const int32_t* m12,
                    uint8_t* skip1, const float* scaleFactors, const float* levelSigma2, int nlevels, float scaleFactor, NewPoint* out,
                    uint8_t* statusRow)
{
    return neighbour(k, *k1, *k2, keys1, n1, keys2, m12, skip1, scaleFactors, levelSigma2, nlevels, scaleFactor, out, statusRow);
}
int npref_sizes(int what) { return what == 0 ? (int)sizeof(KeyFrame) : what == 1 ? (int)sizeof(NewPoint) : (int)sizeof(KeyPt); }

}  // extern "C"
