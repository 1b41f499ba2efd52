// sim3_ref_capi.cpp -- C entry points over the Sim3Solver restatement (tools/sim3_ref.hpp) for the tests (ctypes);
// built with g++ -ffp-contract=off by tests/sim3_cases.py.
#include <cstring>
#include <vector>

#include "../../tools/sim3_ref.hpp"

using sim3_ref::Sim3Solver;

extern "C" {

// cv::eigen on a symmetric 4x4 CV_32F: eigenvalues descending, eigenvectors as rows
void sim3ref_eigen(const float* a, float* w, float* v) { sim3_ref::eigenSym(a, 4, w, v); }

// cv::Rodrigues, vector to matrix
void sim3ref_rodrigues(const float* v, float* R) { sim3_ref::rodrigues(v, R); }

// iterate's set drawing (Sim3Solver.cc:163-177) over the process's rand()
void sim3ref_draw_sets(int n, int iters, int32_t* out)
{
    const std::vector<int32_t> s = sim3_ref::drawSets(n, iters);
    std::memcpy(out, s.data(), s.size() * sizeof(int32_t));
}

void* sim3ref_create(int n1, const int32_t* idx1, int n, const float* X1w, const float* X2w, const float* Rcw1, const float* tcw1,
                     const float* Rcw2, const float* tcw2, const float* K1, const float* K2, const float* s1, const float* s2, int fix)
{
    return new Sim3Solver(n1, idx1, n, X1w, X2w, Rcw1, tcw1, Rcw2, tcw2, K1, K2, s1, s2, fix != 0);
}
void sim3ref_destroy(void* s) { delete (Sim3Solver*)s; }
// SetRansacParameters; returns mRansacMaxIts
int sim3ref_set_ransac(void* s, double p, int minInliers, int maxIts)
{
    ((Sim3Solver*)s)->SetRansacParameters(p, minInliers, maxIts);
    return ((Sim3Solver*)s)->maxIterations();
}
int sim3ref_max_iterations(void* s) { return ((Sim3Solver*)s)->maxIterations(); }
// iterate(n) over the sets given (mRansacMaxIts x 3); hyp (mRansacMaxIts records, may be null) receives every hypothesis evaluated
void sim3ref_iterate(void* s, int n, const int32_t* sets, sim3_ref::Result* res, uint8_t* inliers, sim3_ref::Hypothesis* hyp)
{
    ((Sim3Solver*)s)->iterate(n, sets, *res, inliers, hyp);
}
void sim3ref_thresholds(void* s, float* e1, float* e2)
{
    Sim3Solver* S = (Sim3Solver*)s;
    for (int i = 0; i < S->size(); i++) { e1[i] = S->maxError1(i); e2[i] = S->maxError2(i); }
}
// ComputeSim3 alone on two 3x3 matrices (one point per column): out = T12 (16), T21 (16), R (9), t (3), s (1), quaternion (4)
void sim3ref_compute(const float* P1, const float* P2, int fix, float* out)
{
    const int32_t i0 = 0;
    const float z3[3] = {0, 0, 1}, I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0}, K[4] = {1, 1, 0, 0}, s = 1;
    Sim3Solver S(1, &i0, 1, z3, z3, I, z, I, z, K, K, &s, &s, fix != 0);
    S.ComputeSim3(P1, P2);
    std::memcpy(out, S.T12i(), 64); std::memcpy(out + 16, S.T21i(), 64); std::memcpy(out + 32, S.R12i(), 36);
    std::memcpy(out + 41, S.t12i(), 12); out[44] = S.s12i(); std::memcpy(out + 45, S.quat(), 16);
}

}  // extern "C"
