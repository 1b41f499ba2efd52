// C shim over tools/trackref_ref.hpp for the Python checkers (tests/trackref_cases.py; built by tests/ref_shim.py).
#include "../../tools/trackref_ref.hpp"

using namespace trackref_ref;

extern "C" {

int trackrefref_sizes(int i) { return i == 0 ? (int)sizeof(trackpose_ref::Key) : i == 1 ? (int)sizeof(Result) : (int)sizeof(Branches); }

// valid[n_features] by the rule of ORBmatcher.cc:191-197; the validity counters are ADDED to br
void trackrefref_validity(const int32_t* entries, int n_entries, int stride, int n_features, const uint8_t* flags, int cap, uint8_t* valid, Branches* br)
{
    const trackpose_ref::Pool P = {nullptr, flags, cap};
    const KeyFrame kf = {entries, n_entries, stride, n_features};
    validity(P, kf, valid, *br);
}

// one job behind the search; the counters are ADDED to br.  Returns 0, or -1 for what the device refuses behind its kernel
int trackrefref_run(const int32_t* entries, int n_entries, int stride, int n_features, const int32_t* match, const trackpose_ref::Key* keys, int n,
                    int solve, int min_matches, const float* Tcw, const float* K, const float* pos, const uint8_t* flags, int cap,
                    const float* inv_level_sigma2, int nlevels, Result* out, int32_t* ids_out, uint8_t* outlier_out, Branches* br)
{
    const trackpose_ref::Pool P = {pos, flags, cap};
    const KeyFrame kf = {entries, n_entries, stride, n_features};
    poseopt_ref::Frame F;
    for (int i = 0; i < 16; i++) F.Tcw[i] = Tcw[i];
    for (int i = 0; i < 4; i++) F.K[i] = K[i];
    return trackReference(P, kf, match, keys, n, solve, min_matches, F, inv_level_sigma2, nlevels, *out, ids_out, outlier_out, br);
}

int trackrefref_verdict(int status, int n_matches_map) { return referenceVerdict(status, n_matches_map) ? 1 : 0; }

}  // extern "C"
