// orbx_cvmath.hpp -- the pieces of OpenCV 3.0's arithmetic that more than one solver family restates: the 3x3 float
// algebra (the Initializer, orbi_kernels.hip; the Sim3Solver, orbs_kernels.hip and orbs_host.inc; CreateNewMapPoints,
// orbl_kernels.hip) and the one Jacobi SVD (the Initializer and CreateNewMapPoints in float, the PnPsolver,
// orbp_kernels.hip, in double).  Part of the library's one translation unit.  3x3 matrices are row-major CV_32F.  One IEEE operation per source operation (the library is built
// with -ffp-contract=off, host and device alike); each function names the OpenCV source branch it follows, and its
// rounding is what keeps the device bit-equal with the reference.  (The checkers under tools/ restate the same branches
// on their own and share nothing with this file.)
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace cvm {

// gemm's small-matrix branch (flags 0, len 3) for one output: t = a0*b0 + a1*b1 + a2*b2 in float, products summed left to
// right, d = (float)(t*alpha + c*beta); without a C: c = 0.f, beta = 0.0
__host__ __device__ __forceinline__ float gemm3_elem(float a0, float a1, float a2, float b0, float b1, float b2, double alpha, float c, double beta)
{
    const float t = a0 * b0 + a1 * b1 + a2 * b2;
    return (float)((double)t * alpha + (double)c * beta);
}
// the same branch with len 4 (a 4x4 pose product): four float products summed left to right
__host__ __device__ __forceinline__ float gemm4_elem(float a0, float a1, float a2, float a3, float b0, float b1, float b2, float b3, double alpha, float c, double beta)
{
    const float t = a0 * b0 + a1 * b1 + a2 * b2 + a3 * b3;
    return (float)((double)t * alpha + (double)c * beta);
}
__host__ __device__ inline void mm3(const float* A, const float* B, float* D, double alpha = 1.0)
{
    float o[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o[3 * i + j] = gemm3_elem(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j], alpha, 0.f, 0.0);
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = o[k];
}
__host__ __device__ inline void mv3(const float* A, const float* b, float* d)
{
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = gemm3_elem(A[3 * i], A[3 * i + 1], A[3 * i + 2], b[0], b[1], b[2], 1.0, 0.f, 0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = o[i];
}
// GEMM_1_T / GEMM_2_T: GEMMSingleMul<float, double>, double sums in k order
__host__ __device__ inline void mm3_t1(const float* A, const float* B, float* D)   // A.t()*B
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)A[3 * k + i] * (double)B[3 * k + j];
            D[3 * i + j] = (float)(s * 1.0);
        }
}
__host__ __device__ inline void mm3_t2(const float* A, const float* B, float* D)   // A*B.t()
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)A[3 * i + k] * (double)B[3 * j + k];
            D[3 * i + j] = (float)(s * 1.0);
        }
}
// MatOp_AddEx::assign of alpha*A: 1 -> A + 0, -1 -> 0 - A, else convertTo with a double scale
__host__ __device__ __forceinline__ float expr_scale(float x, double alpha)
{
    if (alpha == 1.0) return x + 0.f;
    if (alpha == -1.0) return 0.f - x;
    return (float)((double)x * alpha);
}
// cv::norm (NORM_L2) of a 3-vector: double sum of squares in order
__host__ __device__ __forceinline__ double norm3(const float* v)
{
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) s += (double)v[i] * (double)v[i];
    return sqrt(s);
}
// cv::determinant's 3x3 branch (the det3 macro: float products in double)
__host__ __device__ __forceinline__ double det3(const float* m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}
// cv::invert's 3x3 branch: the cofactors in double times 1/det, zeros for a zero determinant
__host__ __device__ inline void inv3(const float* S, float* D)
{
    double d = det3(S);
    if (d == 0.) {
#pragma unroll
        for (int k = 0; k < 9; k++) D[k] = 0.f;
        return;
    }
    d = 1. / d;
    const double t0 = ((double)S[4] * S[8] - (double)S[5] * S[7]) * d, t1 = ((double)S[2] * S[7] - (double)S[1] * S[8]) * d,
                 t2 = ((double)S[1] * S[5] - (double)S[2] * S[4]) * d, t3 = ((double)S[5] * S[6] - (double)S[3] * S[8]) * d,
                 t4 = ((double)S[0] * S[8] - (double)S[2] * S[6]) * d, t5 = ((double)S[2] * S[3] - (double)S[0] * S[5]) * d,
                 t6 = ((double)S[3] * S[7] - (double)S[4] * S[6]) * d, t7 = ((double)S[1] * S[6] - (double)S[0] * S[7]) * d,
                 t8 = ((double)S[0] * S[4] - (double)S[1] * S[3]) * d;
    D[0] = (float)t0; D[1] = (float)t1; D[2] = (float)t2; D[3] = (float)t3; D[4] = (float)t4;
    D[5] = (float)t5; D[6] = (float)t6; D[7] = (float)t7; D[8] = (float)t8;
}
// lapack.cpp's hypot<_Tp>, written out in T's own precision (a defined choice: not libm's).  JacobiSVDImpl_ calls it in
// binary64, JacobiImpl_<float> in binary32: fabs / sqrt are T's overloads and 1 + b*b stays a T expression.
template <class T>
__host__ __device__ __forceinline__ T hypot_cv(T a, T b)
{
    a = fabs(a);
    b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

// JacobiSVDImpl_<T>(At, .., W, Vt, .., m, n, n1, minval, eps) of lapack.cpp, T = float (FLT_MIN, FLT_EPSILON*2) or double
// (DBL_MIN, DBL_EPSILON*10), on arrays in LDS.  Device code only.  S threads interleave their arrays: element (i, k) of At
// at At[(i*m + k)*S], of Vt at Vt[(i*n + k)*S], W[i] at W[i*S] (double; on return the sorted singular values, still
// double).  As in the template, T is the precision of c, s, the rotated elements, val0, asum and the completion's products;
// every sum of squares and the dot products are double.  trackV: Vt's rotations are kept (callers that read only At skip
// them and may pass no Vt).  complete: run the random completion of rows [0, n1) of At (callers that read only Vt skip it).
template <class T, int S>
__device__ void jacobi_svd(T* At, double* W, T* Vt, int m, int n, int n1, bool trackV, bool complete)
{
#define A_(i, k) At[((i) * m + (k)) * S]
#define V_(i, k) Vt[((i) * n + (k)) * S]
    constexpr bool kFloat = sizeof(T) == sizeof(float);
    const double minval = kFloat ? (double)FLT_MIN : DBL_MIN;
    const T eps = kFloat ? (T)(FLT_EPSILON * 2) : (T)(DBL_EPSILON * 10);
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const T t = A_(i, k); sd += (double)t * t; }
        W[i * S] = sd;
        if (trackV) { for (int k = 0; k < n; k++) V_(i, k) = 0; V_(i, i) = 1; }
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double a = W[i * S], p = 0, b = W[j * S];
                for (int k = 0; k < m; k++) p += (double)A_(i, k) * A_(j, k);
                if (fabs(p) <= eps * sqrt((double)a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot_cv(p, beta);
                T c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (T)sqrt(delta / gamma);
                    c = (T)(p / (gamma * s * 2));
                } else {
                    c = (T)sqrt((gamma + beta) / (gamma * 2));
                    s = (T)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const T ai = A_(i, k), aj = A_(j, k);
                    const T t0 = c * ai + s * aj;
                    const T t1 = -s * ai + c * aj;
                    A_(i, k) = t0; A_(j, k) = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i * S] = a; W[j * S] = b;
                changed = true;
                if (trackV)
                    for (int k = 0; k < n; k++) {
                        const T vi = V_(i, k), vj = V_(j, k);
                        V_(i, k) = c * vi + s * vj;
                        V_(j, k) = -s * vi + c * vj;
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const T t = A_(i, k); sd += (double)t * t; }
        W[i * S] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j * S] < W[k * S]) j = k;
        if (i != j) {
            const double tw = W[i * S]; W[i * S] = W[j * S]; W[j * S] = tw;
            for (int k = 0; k < m; k++) { const T t = A_(i, k); A_(i, k) = A_(j, k); A_(j, k) = t; }
            if (trackV) for (int k = 0; k < n; k++) { const T t = V_(i, k); V_(i, k) = V_(j, k); V_(j, k) = t; }
        }
    }
    if (!complete) return;
    uint64_t state = 0x12345678;   // cv::RNG(0x12345678)
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? W[i * S] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const T val0 = (T)(1. / m);
            for (int k = 0; k < m; k++) {
                state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
                A_(i, k) = ((unsigned)state & 256) != 0 ? val0 : -val0;
            }
            for (int it = 0; it < 2; it++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += A_(i, k) * A_(j, k);   // T products, double sum
                    T asum = 0;
                    for (int k = 0; k < m; k++) {
                        const T t = (T)(A_(i, k) - sd * A_(j, k));
                        A_(i, k) = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) A_(i, k) *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const T t = A_(i, k); sd += (double)t * t; }
            sd = sqrt(sd);
        }
        const T s = (T)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < m; k++) A_(i, k) *= s;
    }
#undef A_
#undef V_
}

}  // namespace cvm
