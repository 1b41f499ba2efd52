// C entry points over tools/correct_ref.hpp for the tests and tools/correct_bench.py (built by tests/ref_shim.py).
#include "../../tools/correct_ref.hpp"

using namespace correct_ref;

extern "C" {

int cor_kf_size(void) { return (int)sizeof(KeyFrameOut); }
int cor_point_size(void) { return (int)sizeof(PointOut); }

// the loop over the world's arrays, which it OVERWRITES (positions, normals, bounds, centres): the caller passes copies.
// outKf[K] in the caller's order, outPts[poolCap]; branches: kBranchInts ints added to, or null.  Returns the moved points
int cor_correct(World* w, const Args* a, KeyFrameOut* outKf, PointOut* outPts, int32_t* branches)
{
    Branches br = Branches();
    const refresh_ref::Observations obs(viewOf(*w));
    const int n = correctLoop(*w, obs, *a, outKf, outPts, branches ? &br : 0);
    if (branches) { int32_t b[kBranchInts]; std::memcpy(b, &br, sizeof b); for (int q = 0; q < kBranchInts; q++) branches[q] += b[q]; }
    return n;
}

// the same over an observation index built once (the entries and the set flags must not change behind it): what a caller
// whose MapPoints carry their mObservations pays, for tools/correct_bench.py
void* cor_index(const World* w) { return new refresh_ref::Observations(viewOf(*w)); }
void cor_index_free(void* idx) { delete (refresh_ref::Observations*)idx; }
int cor_correct_indexed(World* w, const void* idx, const Args* a, KeyFrameOut* outKf, PointOut* outPts)
{
    return correctLoop(*w, *(const refresh_ref::Observations*)idx, *a, outKf, outPts, 0);
}

}
static_assert(sizeof(Branches) == kBranchInts * sizeof(int32_t), "the branch counters are kBranchInts ints");
static_assert(sizeof(KeyFrameOut) == 192 && sizeof(PointOut) == 52, "OrbeKeyFrame's and OrbePoint's layouts");
