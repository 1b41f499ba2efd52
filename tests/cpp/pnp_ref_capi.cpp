// pnp_ref_capi.cpp -- C entry points over the PnPsolver restatement (tools/pnp_ref.hpp) for the tests and
// tools/pnp_bench.py (ctypes); built with g++ -ffp-contract=off through tests/ref_shim.py.
#include <cstring>
#include <vector>

#include "../../tools/pnp_ref.hpp"

using pnp_ref::PnPsolver;

extern "C" {

// cvSVD of a row-major m x n matrix (m >= n): w (n), ut (n x m, rows = left vectors), vt (n x n)
void pnpref_svd(const double* A, int m, int n, double* w, double* ut, double* vt) { pnp_ref::svd(A, m, n, w, ut, vt); }
// cvSolve(A, b, x, CV_SVD)
void pnpref_solve_svd(const double* A, int m, int n, const double* b, double* x) { pnp_ref::solveSVD(A, m, n, b, x); }
// cvInvert(A, Ainv, CV_SVD), 3x3
void pnpref_invert3(const double* A, double* Ainv) { pnp_ref::invert3(A, Ainv); }
// qr_solve on a 6x4 system (A and b are overwritten); returns 0 on the singular branch
int pnpref_qr_solve(double* A, double* b, double* x) { return pnp_ref::qrSolve(A, b, x) ? 1 : 0; }
// cvMulTransposed(src, dst, 1)
void pnpref_mul_transposed(const double* src, int rows, int cols, double* dst) { pnp_ref::mulTransposed(src, rows, cols, dst); }

// iterate's set drawing (PnPsolver.cc:191-201) over the process's rand()
void pnpref_draw_sets(int n, int iters, int32_t* out)
{
    const std::vector<int32_t> s = pnp_ref::drawSets(n, iters);
    std::memcpy(out, s.data(), s.size() * sizeof(int32_t));
}

void* pnpref_create(int nAll, const int32_t* idx, int n, const float* P2D, const float* sigma2, const float* P3Dw, const float* K)
{
    return new PnPsolver(nAll, idx, n, P2D, sigma2, P3Dw, K);
}
void pnpref_destroy(void* s) { delete (PnPsolver*)s; }
int pnpref_set_ransac(void* s, double p, int minInliers, int maxIts, int minSet, float eps, float th2)
{
    return ((PnPsolver*)s)->SetRansacParameters(p, minInliers, maxIts, minSet, eps, th2);
}
int pnpref_max_iterations(void* s) { return ((PnPsolver*)s)->maxIterations(); }
int pnpref_min_inliers(void* s) { return ((PnPsolver*)s)->minInliers(); }
int pnpref_iterations(void* s) { return ((PnPsolver*)s)->iterations(); }
float pnpref_epsilon(void* s) { return ((PnPsolver*)s)->epsilon(); }
void pnpref_thresholds(void* s, float* e)
{
    PnPsolver* S = (PnPsolver*)s;
    for (int i = 0; i < S->size(); i++) e[i] = S->maxError(i);
}
// iterate(n) over nSets sets of 4; hyp (nSets records, may be null) receives every hypothesis evaluated
int pnpref_iterate(void* s, int n, const int32_t* sets, int nSets, pnp_ref::Result* res, uint8_t* inliers, pnp_ref::Hypothesis* hyp, int stopOnRefine)
{
    return ((PnPsolver*)s)->iterate(n, sets, nSets, *res, inliers, hyp, stopOnRefine != 0);
}
// compute_pose on n of the solver's correspondences; returns the reprojection error
double pnpref_compute_pose(void* s, const int32_t* set, int n, double* R, double* t) { return ((PnPsolver*)s)->computePose(set, n, R, t); }

}  // extern "C"
