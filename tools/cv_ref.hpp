// cv_ref.hpp -- the OpenCV 3.0 arithmetic that the restatements (init_ref, sim3_ref, newpoints_ref, pnp_ref) call, and
// DUtils::Random's integer draw, stated once.  Restated from the published 3.0 source, UNPINNED: no
// OpenCV exists to compare against.  Standard headers only: like its includers it shares nothing with the library it
// checks, and is built with g++ -ffp-contract=off (every operation one IEEE operation).
//
// What stays with its restatement, because the copies are not the same sequence of operations: the Jacobi SVDs (init_ref's
// float m x n completes zero singular values, newpoints_ref's 4x4 does not, pnp_ref's is binary64 with another epsilon),
// sim3_ref's eigenSym, and the transposed gemm branches (the generic kernel, written per shape where it is used).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace cv_ref {

// gemm(A, B, alpha, C, beta) with flags == 0 and len == 3 (matmul.cpp's small-matrix branch), one element: a is a row of A,
// b a column of B with stride bstep; the three products summed in float, left to right, then d = (float)(t*alpha + c*beta)
// in double.  C absent: c = 0, beta = 0 (so -0 becomes +0).
inline float gemmElem(const float* a, const float* b, int bstep, double alpha, float c, double beta)
{
    const float t = a[0] * b[0] + a[1] * b[bstep] + a[2] * b[2 * bstep];
    return (float)((double)t * alpha + (double)c * beta);
}
// a MatExpr `alpha*A` (or A/s, -A) assigned to a Mat (MatOp_AddEx::assign): alpha 1 -> add(A, 0), alpha -1 ->
// subtract(0, A), else convertTo with a double scale
inline float exprScale(float x, double alpha)
{
    if (alpha == 1.0) return x + 0.f;
    if (alpha == -1.0) return 0.f - x;
    return (float)((double)x * alpha);
}
// cv::scaleAdd(a, alpha, b) on CV_32F: the scale converted to float, a float product, a float sum
inline float scaleAdd(float a, double alpha, float b) { const float fa = (float)alpha; return a * fa + b; }
// cv::norm (normL2_<float, double>) and Mat::dot on CV_32F: double accumulation in element order
inline double norm(const float* a, int n) { double s = 0; for (int i = 0; i < n; i++) s += (double)a[i] * (double)a[i]; return std::sqrt(s); }
inline double dot(const float* a, const float* b, int n) { double s = 0; for (int i = 0; i < n; i++) s += (double)a[i] * (double)b[i]; return s; }
// determinant / invert of a 3x3 row-major CV_32F (lapack.cpp: det3 in double; invert's n == 3 branch, the cofactors in
// double, zeros when singular)
inline double det3(const float* S)
{
    return S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) +
           S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
}
inline void inv33(const float* S, float* D)
{
    double d = det3(S);
    if (d == 0.) { for (int i = 0; i < 9; i++) D[i] = 0.f; return; }
    d = 1. / d;
    const double t[9] = {((double)S[4] * S[8] - (double)S[5] * S[7]) * d, ((double)S[2] * S[7] - (double)S[1] * S[8]) * d,
                         ((double)S[1] * S[5] - (double)S[2] * S[4]) * d, ((double)S[5] * S[6] - (double)S[3] * S[8]) * d,
                         ((double)S[0] * S[8] - (double)S[2] * S[6]) * d, ((double)S[2] * S[3] - (double)S[0] * S[5]) * d,
                         ((double)S[3] * S[7] - (double)S[4] * S[6]) * d, ((double)S[1] * S[6] - (double)S[0] * S[7]) * d,
                         ((double)S[0] * S[4] - (double)S[1] * S[3]) * d};
    for (int i = 0; i < 9; i++) D[i] = (float)t[i];
}
// lapack.cpp's hypot, a template there too: binary64 inside the Jacobi SVDs, float inside cv::eigen (the 1 converts to T,
// std::sqrt is T's overload)
template <class T> inline T hypotCv(T a, T b)
{
    a = std::abs(a);
    b = std::abs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
}

// DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp) over the process's rand()
inline int randomInt(int min, int max) { const int d = max - min + 1; return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min; }
// The set draw of Sim3Solver::iterate (:163-177, k = 3) and PnPsolver::iterate (:191-201, k = 4), `iterations` sets
// flattened: vAvailableIndices[idx] = back() with idx the drawn VALUE, as the reference has it, so a set can repeat a
// point; on a plain array of N with a live length (the reference's write past the live part lands inside the vector's
// capacity and is never read back: the live length only shrinks)
inline std::vector<int32_t> drawSets(int N, int iterations, int k)
{
    std::vector<int32_t> sets((size_t)iterations * k, 0), avail((size_t)N);
    for (int it = 0; it < iterations; it++) {
        for (int i = 0; i < N; i++) avail[i] = i;
        int live = N;
        for (int j = 0; j < k; j++) {
            const int randi = randomInt(0, live - 1);
            const int idx = avail[randi];
            sets[(size_t)it * k + j] = idx;
            avail[idx] = avail[live - 1];
            live--;
        }
    }
    return sets;
}

}  // namespace cv_ref
