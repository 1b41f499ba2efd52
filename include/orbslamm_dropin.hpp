// orbslamm_dropin.hpp -- what the solver drop-ins (Initializer_hip.hpp, Sim3Solver_hip.hpp, PnPsolver_hip.hpp,
// LocalMapping_hip.hpp) share.  Header-only, C++11; installed next to them and included by relative name.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_hip.h"

namespace iORB_SLAM {
namespace detail {

const int kCV_32F = 5;

// an error of the C ABI as the drop-ins throw it: who ("Sim3Solver(HIP): ") and the library's text
inline void check(int rc, const char* who)
{
    if (rc != ORBX_OK) throw std::runtime_error(std::string(who) + orbx_last_error());
}

// `count` more RANSAC sets of k behind `sets`, drawn as the Sim3Solver's and the PnPsolver's iterate draw them
// (Sim3Solver.cc:163-177, PnPsolver.cc:191-201): Random::RandomInt over the process's rand(), one call per index;
// vAvailableIndices[idx] is indexed by the drawn VALUE as in the reference (its write can land past the live part: here
// the vector keeps its N slots)
template <class Random>
void draw_sets(int N, int k, int count, std::vector<int32_t>& sets)
{
    std::vector<size_t> vAvailableIndices((size_t)N);
    size_t at = sets.size();
    sets.resize(at + (size_t)count * k, 0);
    for (int it = 0; it < count; it++) {
        for (int i = 0; i < N; i++) vAvailableIndices[i] = (size_t)i;
        int live = N;
        for (short i = 0; i < k; ++i) {
            const int randi = Random::RandomInt(0, live - 1);
            const int idx = (int)vAvailableIndices[randi];
            sets[at++] = idx;
            vAvailableIndices[idx] = vAvailableIndices[live - 1];
            live--;
        }
    }
}

// the first n flags of a mask as the reference's vector<bool>
inline std::vector<bool> mask_bools(const std::vector<uint8_t>& mask, int n)
{
    std::vector<bool> out((size_t)n, false);
    for (int i = 0; i < n; i++) if (mask[i]) out[i] = true;
    return out;
}

// a row-major float array as Mat(rows, cols, CV_32F)
template <class Mat>
Mat mat32f(const float* a, int rows, int cols)
{
    Mat m(rows, cols, kCV_32F);
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) m.template at<float>(r, c) = a[cols * r + c];
    return m;
}

}  // namespace detail
}  // namespace iORB_SLAM
