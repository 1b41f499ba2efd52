// C shim over tools/computesim3_ref.hpp for the Python checkers (tests/computesim3_cases.py; built by tests/ref_shim.py).
#include "../../tools/computesim3_ref.hpp"

using namespace computesim3_ref;

extern "C" {

int computesim3ref_sizes(int i)
{
    return i == 0 ? (int)sizeof(Key) : i == 1 ? (int)sizeof(Grid) : i == 2 ? (int)sizeof(sim3opt_ref::Problem) : i == 3 ? (int)sizeof(Result) : (int)sizeof(Counters);
}

// One job.  kf arrays come in pairs, pKF1's first: keys, desc, n, entries, n_entries, bounds (4 floats each), scale factors, break
// tables, sigma tables.  The counters are added to.
void computesim3ref_run(const float* pos, const float* min_d, const float* max_d, const uint8_t* flags, const uint8_t* pdesc, int cap,
                        const Key* keys1, const uint8_t* desc1, int n1, const int32_t* entries1, int n_entries1, const float* bounds1,
                        const Key* keys2, const uint8_t* desc2, int n2, const int32_t* entries2, int n_entries2, const float* bounds2,
                        const float* sf1, const float* sf2, const float* breaks1, const float* breaks2, const float* sig1, const float* sig2, int nlevels,
                        const Grid* grid, const sim3opt_ref::Problem* prob, const float* R12, const float* t12, float s12, float th,
                        const int32_t* m12_id, const int32_t* m12_idx2, Result* res, int32_t* match_out, int32_t* ids_out, uint8_t* removed,
                        uint8_t* status, int32_t* vn, Counters* br)
{
    const Pool pool = {pos, min_d, max_d, flags, pdesc, cap};
    KeyFrame a = {keys1, desc1, n1, entries1, n_entries1, {bounds1[0], bounds1[1], bounds1[2], bounds1[3]}, sf1, breaks1, sig1};
    KeyFrame b = {keys2, desc2, n2, entries2, n_entries2, {bounds2[0], bounds2[1], bounds2[2], bounds2[3]}, sf2, breaks2, sig2};
    computeSim3(pool, a, b, *grid, *prob, R12, t12, s12, th, nlevels, m12_id, m12_idx2, *res, match_out, ids_out, removed, status, vn, *br);
}

int computesim3ref_verdict(int n_inliers) { return verdict(n_inliers) ? 1 : 0; }

}  // extern "C"
