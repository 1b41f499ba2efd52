// C entry points over tools/covis_ref.hpp for the tests and tools/covis_bench.py (built by tests/ref_shim.py).
#include "../../tools/covis_ref.hpp"

#include <cstring>

using namespace covis_ref;

struct CovHandle {
    Store s;
    Observations obs;
    explicit CovHandle(const Store& st) : s(st), obs(st) {}
};

extern "C" {

// the arrays must outlive the handle; the observation index is built here, once
void* cov_open(const Store* s) { return new CovHandle(*s); }
void cov_close(void* h) { delete (CovHandle*)h; }

// rows of at most `cap` pairs in all; returns 0, or -1 when they do not fit.  branches: kBranchInts ints added to, or null
int cov_connections(void* hv, const int32_t* targets, int K, int th, int32_t* status, int32_t* kfMax, int32_t* nMax, int32_t* cntStart, int32_t* cntKf,
                    int32_t* cntW, int32_t* ordStart, int32_t* ordKf, int32_t* ordW, int cap, int32_t* branches)
{
    CovHandle* h = (CovHandle*)hv;
    Branches br = Branches();
    int nc = 0, no = 0;
    cntStart[0] = 0; ordStart[0] = 0;
    for (int t = 0; t < K; t++) {
        const Connections r = updateConnections(h->s, h->obs, targets[t], th, branches ? &br : 0);
        if (nc + (int)r.counter.size() > cap || no + (int)r.ordered.size() > cap) return -1;
        status[t] = r.empty ? 1 : 0; kfMax[t] = r.kfMax; nMax[t] = r.nMax;
        for (size_t q = 0; q < r.counter.size(); q++) { cntKf[nc] = r.counter[q].first; cntW[nc] = r.counter[q].second; nc++; }
        for (size_t q = 0; q < r.ordered.size(); q++) { ordKf[no] = r.ordered[q].first; ordW[no] = r.ordered[q].second; no++; }
        cntStart[t + 1] = nc; ordStart[t + 1] = no;
    }
    if (branches) { int32_t b[kBranchInts]; std::memcpy(b, &br, sizeof b); for (int q = 0; q < kBranchInts; q++) branches[q] += b[q]; }
    return 0;
}

void cov_culling(void* hv, const int32_t* targets, int K, int thObs, int32_t* nMps, int32_t* nRedundant, uint8_t* redundant, int32_t* branches)
{
    CovHandle* h = (CovHandle*)hv;
    Branches br = Branches();
    for (int t = 0; t < K; t++) {
        const Culling r = cullingCounts(h->s, h->obs, targets[t], thObs, branches ? &br : 0);
        nMps[t] = r.nMPs; nRedundant[t] = r.nRedundant; redundant[t] = r.redundant ? 1 : 0;
    }
    if (branches) { int32_t b[kBranchInts]; std::memcpy(b, &br, sizeof b); for (int q = 0; q < kBranchInts; q++) branches[q] += b[q]; }
}

}
static_assert(sizeof(Branches) == kBranchInts * sizeof(int32_t), "the branch counters are kBranchInts ints");
