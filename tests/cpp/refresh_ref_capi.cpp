// C entry points over tools/refresh_ref.hpp for the tests and tools/refresh_bench.py (built by tests/ref_shim.py).
#include "../../tools/refresh_ref.hpp"

using namespace refresh_ref;

struct RefreshHandle {
    Store s;
    Observations obs;
    explicit RefreshHandle(const Store& st) : s(st), obs(st) {}
};

extern "C" {

// the arrays must outlive the handle; the observation index is built here, once
void* rfr_open(const Store* s) { return new RefreshHandle(*s); }
void rfr_close(void* h) { delete (RefreshHandle*)h; }
int rfr_point_size(void) { return (int)sizeof(Point); }

// out[n] Point records (OrbrPoint's layout).  newPos: 3 n floats or null.  branches: kBranchInts ints added to, or null
void rfr_refresh(void* hv, const int32_t* ids, const int32_t* refKf, const float* newPos, int n, int what, const float* sf, int nlevels, Point* out,
                 int32_t* branches)
{
    RefreshHandle* h = (RefreshHandle*)hv;
    Branches br = Branches();
    for (int i = 0; i < n; i++) refreshPoint(h->s, h->obs, ids[i], refKf[i], newPos ? newPos + 3 * (size_t)i : 0, what, sf, nlevels, out[i], branches ? &br : 0);
    if (branches) { int32_t b[kBranchInts]; std::memcpy(b, &br, sizeof b); for (int q = 0; q < kBranchInts; q++) branches[q] += b[q]; }
}

}
static_assert(sizeof(Branches) == kBranchInts * sizeof(int32_t), "the branch counters are kBranchInts ints");
static_assert(sizeof(Point) == 84, "OrbrPoint's layout");
