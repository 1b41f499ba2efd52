// orbi_kernels.hip -- the device Initializer (src/Initializer.cc of both scenarios).  Part of the
// library's one translation unit (orbslamm_hip.hip); host side: orbi_host.inc.
//
// One Initialize is one chain on the handle's stream and one copy down:
//   k_init_normalize   Normalize (:764-811) of a frame: its float sums in key order, one ordered chain per frame (the
//                      block stages keys in LDS, thread 0 adds them in lane order)
//   k_init_fit<H>      one hypothesis per thread: the 8-point matrix, JacobiSVDImpl_<float> on arrays in LDS, ComputeH21 /
//                      ComputeF21, the de-normalisation (and H's inverse)
//   k_init_score<H>    one block per hypothesis: CheckHomography / CheckFundamental's chi-square terms in parallel, their
//                      sum by one lane in match order
//   k_init_pick        one lane: the RANSAC winners (the first currentScore > score from 0), RH and the model, the pose
//                      candidates (DecomposeE, or ReconstructH's eight)
//   k_init_checkrt     candidates x matches: the winner's inlier flag, Triangulate (a 4x4 SVD per thread in LDS) and
//                      CheckRT's tests; nGood by integer atomics
//   k_init_winner      one block: the winning candidate from integers alone, the 51st-smallest cosParallax of every
//                      candidate (radix select: order-free), the winner's vP3D / vbTriangulated
// Arithmetic: one IEEE operation per source operation (the library is built with -ffp-contract=off), float and double
// division and sqrt correctly rounded.  OpenCV's pieces follow its 3.0 source and are unpinned.
#pragma once

#include <cfloat>

namespace orbi {

constexpr int kMaxIterations = 4096;
constexpr int kMaxFeatures = 65535;
constexpr int kNormThreads = 256;
constexpr int kFitThreads = 32;
constexpr int kScoreThreads = 256;
constexpr int kRtThreads = 128;
constexpr int kWinThreads = 256;

struct Key { float x, y, size, angle, response; int32_t octave, class_id; };   // cv::KeyPoint's layout
struct Norm { float meanX, meanY, sX, sY; };
struct Pair { int32_t i1, i2; };

// what the chain leaves for the host
struct Hdr {
    float SH, SF, RH;
    int32_t itH, itF, reconH, nCand;
    int32_t status;                   // 0: candidates ran; 1: ReconstructH's singular-value test failed; 2: the model's best score stayed 0
    float H21[9], H12[9], F21[9];
    float R[8][9], t[8][3];
    int32_t nInliers, nInliersH, nInliersF;
    int32_t nGood[8];
    float kthCos[8];
    int32_t best;
    int32_t pad[3];
};

// OpenCV 3.0 arithmetic (3x3 row-major, CV_32F): orbx_cvmath.hpp
using cvm::det3; using cvm::expr_scale; using cvm::gemm3_elem; using cvm::inv3; using cvm::jacobi_svd; using cvm::mm3; using cvm::mm3_t1;
using cvm::mm3_t2; using cvm::mv3; using cvm::norm3;

// cv::SVD::compute(src 3x3, w, u, vt) for one lane: arrays in LDS (stride 1)
__device__ inline void svd3_lane(const float* src, float* At, float* Vt, double* W, float* U, float* w, float* vt)
{
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) At[i * 3 + k] = src[3 * k + i];   // !at: temp_a = src.t()
    jacobi_svd<float, 1>(At, W, Vt, 3, 3, 3, true, true);
    for (int i = 0; i < 3; i++) w[i] = (float)W[i];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { U[3 * r + c] = At[c * 3 + r]; vt[3 * r + c] = Vt[3 * r + c]; }
}

// ------------------------------------------------------------------ Normalize
// blockIdx.x: frame (keys[f], n[f]); out[f] = (meanX, meanY, sX, sY)
__global__ __launch_bounds__(kNormThreads) void k_init_normalize(const Key* __restrict__ k0, int n0, const Key* __restrict__ k1, int n1, Norm* __restrict__ out)
{
    const Key* keys = blockIdx.x == 0 ? k0 : k1;
    const int n = blockIdx.x == 0 ? n0 : n1;
    __shared__ float sx[kNormThreads], sy[kNormThreads];
    __shared__ float sMean[2];
    float accX = 0, accY = 0;
    for (int base = 0; base < n; base += kNormThreads) {
        const int i = base + threadIdx.x;
        if (i < n) { sx[threadIdx.x] = keys[i].x; sy[threadIdx.x] = keys[i].y; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(kNormThreads, n - base);
            for (int k = 0; k < cnt; k++) { accX += sx[k]; accY += sy[k]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sMean[0] = accX / n; sMean[1] = accY / n; }
    __syncthreads();
    const float meanX = sMean[0], meanY = sMean[1];
    float devX = 0, devY = 0;
    for (int base = 0; base < n; base += kNormThreads) {
        const int i = base + threadIdx.x;
        if (i < n) { sx[threadIdx.x] = fabsf(keys[i].x - meanX); sy[threadIdx.x] = fabsf(keys[i].y - meanY); }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(kNormThreads, n - base);
            for (int k = 0; k < cnt; k++) { devX += sx[k]; devY += sy[k]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        devX = devX / n;
        devY = devY / n;
        Norm r;
        r.meanX = meanX; r.meanY = meanY;
        r.sX = (float)(1.0 / (double)devX);
        r.sY = (float)(1.0 / (double)devY);
        out[blockIdx.x] = r;
    }
}

__device__ __forceinline__ void norm_T(const Norm& q, float* T)
{
    T[0] = q.sX; T[1] = 0.f; T[2] = -q.meanX * q.sX;
    T[3] = 0.f; T[4] = q.sY; T[5] = -q.meanY * q.sY;
    T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// ------------------------------------------------------------------ hypotheses
// H: out[h*18 ..] = H21, H12; F: out[h*9 ..] = F21
template <bool H>
__global__ __launch_bounds__(kFitThreads) void k_init_fit(const Key* __restrict__ k1, const Key* __restrict__ k2, const Norm* __restrict__ nrm,
                                                          const Pair* __restrict__ pairs, const int32_t* __restrict__ sets, int iters,
                                                          float* __restrict__ out)
{
    // H: A is 16x9 -> not transposed, At 9 x 16, Vt 9 x 9 read (row 8).  F: A is 8x9 -> transposed, At 8 x 9 plus the
    // completed row 8 (u of the transposed problem = vt), then the 3x3 SVD of Fpre.
    constexpr int M = H ? 16 : 9, N = H ? 9 : 8, ROWS = 9;
    __shared__ float sA[ROWS * M * kFitThreads];
    __shared__ float sV[(H ? 81 : 9) * kFitThreads];
    __shared__ double sW[N * kFitThreads];
    __shared__ float sA3[H ? 1 : 9 * kFitThreads];
    const int t = threadIdx.x, h = blockIdx.x * kFitThreads + t;
    if (h >= iters) return;   // (no barrier below)
    float* A = sA + t;
    double* W = sW + t;
    const Norm n1 = nrm[0], n2 = nrm[1];
    for (int j = 0; j < 8; j++) {
        const Pair p = pairs[sets[h * 8 + j]];
        const float u1 = (k1[p.i1].x - n1.meanX) * n1.sX, v1 = (k1[p.i1].y - n1.meanY) * n1.sY;
        const float u2 = (k2[p.i2].x - n2.meanX) * n2.sX, v2 = (k2[p.i2].y - n2.meanY) * n2.sY;
        if (H) {
            // rows 2j, 2j+1 of A are columns 2j, 2j+1 of At (At(c, r) = A(r, c), row length 16)
            const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
            for (int c = 0; c < 9; c++) { A[(c * M + 2 * j) * kFitThreads] = r0[c]; A[(c * M + 2 * j + 1) * kFitThreads] = r1[c]; }
        } else {
            const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
#pragma unroll
            for (int c = 0; c < 9; c++) A[(j * M + c) * kFitThreads] = r[c];
        }
    }
    float T1[9], T2[9];
    norm_T(n1, T1);
    norm_T(n2, T2);
    if (H) {
        jacobi_svd<float, kFitThreads>(A, W, sV + t, M, N, 16, true, false);
        float Hn[9], T2inv[9], X[9], H21[9], H12[9];
        for (int k = 0; k < 9; k++) Hn[k] = sV[t + (8 * N + k) * kFitThreads];
        inv3(T2, T2inv);
        mm3(T2inv, Hn, X);
        mm3(X, T1, H21);
        inv3(H21, H12);
        float* o = out + (size_t)h * 18;
        for (int k = 0; k < 9; k++) { o[k] = H21[k]; o[9 + k] = H12[k]; }
    } else {
        jacobi_svd<float, kFitThreads>(A, W, nullptr, M, N, 9, false, true);
        float Fpre[9];
        for (int k = 0; k < 9; k++) Fpre[k] = A[(8 * M + k) * kFitThreads];
        // SVDecomp(Fpre, w, u, vt, FULL_UV): 3x3, not transposed
        float* A3 = sA3 + t;
        float* V3 = sV + t;
        double* W3 = W;   // (the 8x9 decomposition's W is no longer read)
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) A3[(i * 3 + k) * kFitThreads] = Fpre[3 * k + i];
        jacobi_svd<float, kFitThreads>(A3, W3, V3, 3, 3, 3, true, true);
        float u[9], vt[9], D[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) { u[3 * r + c] = A3[(c * 3 + r) * kFitThreads]; vt[3 * r + c] = V3[(r * 3 + c) * kFitThreads]; }
        D[0] = (float)W3[0];
        D[4] = (float)W3[kFitThreads];
        D[8] = 0.f;   // w.at<float>(2) = 0
        float X[9], Fn[9], T2t[9], F21[9];
        mm3(u, D, X);
        mm3(X, vt, Fn);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) T2t[3 * r + c] = T2[3 * c + r];
        mm3(T2t, Fn, X);
        mm3(X, T1, F21);
        float* o = out + (size_t)h * 9;
        for (int k = 0; k < 9; k++) o[k] = F21[k];
    }
}

// CheckHomography / CheckFundamental for one match: the two chi-square values
__device__ __forceinline__ void chi_h(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare, float& chi1, float& chi2)
{
    const float w2in1inv = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]);
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * invSigmaSquare;
    const float w1in2inv = 1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8]);
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * invSigmaSquare;
}
__device__ __forceinline__ void chi_f(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float& chi1, float& chi2)
{
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * invSigmaSquare;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * invSigmaSquare;
}
__device__ __forceinline__ float th_h() { return (float)5.991; }
__device__ __forceinline__ float th_f() { return (float)3.841; }
__device__ __forceinline__ float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// blockIdx.x: hypothesis; score[h] = its score, summed by one lane in match order
template <bool H>
__global__ __launch_bounds__(kScoreThreads) void k_init_score(const Key* __restrict__ k1, const Key* __restrict__ k2, const Pair* __restrict__ pairs, int N,
                                                              const float* __restrict__ hyp, float sigma, float* __restrict__ score)
{
    __shared__ float sT0[kScoreThreads], sT1[kScoreThreads];
    __shared__ uint8_t sIn0[kScoreThreads], sIn1[kScoreThreads];
    const float* Hm = hyp + (size_t)blockIdx.x * (H ? 18 : 9);
    float M[18];
    for (int k = 0; k < (H ? 18 : 9); k++) M[k] = Hm[k];
    const float invS = inv_sigma_square(sigma);
    const float th = H ? th_h() : th_f(), thScore = th_h();
    float acc = 0;
    for (int base = 0; base < N; base += kScoreThreads) {
        const int i = base + threadIdx.x;
        if (i < N) {
            const Pair p = pairs[i];
            float c1, c2;
            if (H) chi_h(M, M + 9, k1[p.i1].x, k1[p.i1].y, k2[p.i2].x, k2[p.i2].y, invS, c1, c2);
            else chi_f(M, k1[p.i1].x, k1[p.i1].y, k2[p.i2].x, k2[p.i2].y, invS, c1, c2);
            sIn0[threadIdx.x] = !(c1 > th);
            sIn1[threadIdx.x] = !(c2 > th);
            sT0[threadIdx.x] = thScore - c1;
            sT1[threadIdx.x] = thScore - c2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(kScoreThreads, N - base);
            for (int k = 0; k < cnt; k++) {
                if (sIn0[k]) acc += sT0[k];
                if (sIn1[k]) acc += sT1[k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) score[blockIdx.x] = acc;
}

// ------------------------------------------------------------------ the winners and the pose candidates (one lane)
__global__ __launch_bounds__(64) void k_init_pick(const float* __restrict__ hypF, const float* __restrict__ scoreF, const float* __restrict__ hypH,
                                                  const float* __restrict__ scoreH, int iters, int hf, float fx, float fy, float cx, float cy, Hdr* hdr)
{
    __shared__ float sAt[9], sVt[9];
    __shared__ double sW[3];
    if (threadIdx.x != 0) return;
    float SF = 0.0f, SH = 0.0f;
    int itF = -1, itH = -1;
    for (int it = 0; it < iters; it++) if (scoreF[it] > SF) { SF = scoreF[it]; itF = it; }
    if (hf) for (int it = 0; it < iters; it++) if (scoreH[it] > SH) { SH = scoreH[it]; itH = it; }
    hdr->SF = SF; hdr->SH = SH; hdr->itF = itF; hdr->itH = itH;
    float F21[9], H21[9], H12[9];
    for (int k = 0; k < 9; k++) {
        F21[k] = itF >= 0 ? hypF[(size_t)itF * 9 + k] : 0.f;
        H21[k] = itH >= 0 ? hypH[(size_t)itH * 18 + k] : 0.f;
        H12[k] = itH >= 0 ? hypH[(size_t)itH * 18 + 9 + k] : 0.f;
        hdr->F21[k] = F21[k]; hdr->H21[k] = H21[k]; hdr->H12[k] = H12[k];
    }
    int reconH = 0;
    if (hf) {
        const float RH = SH / (SH + SF);
        hdr->RH = RH;
        reconH = RH > 0.45;
    } else
        hdr->RH = 0.f;
    hdr->reconH = reconH;
    const float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    float U[9], w[3], Vt[9], X[9];
    if (reconH) {
        // ReconstructH (:587-702)
        float invK[9], A[9];
        inv3(K, invK);
        mm3(invK, H21, X);
        mm3(X, K, A);
        svd3_lane(A, sAt, sVt, sW, U, w, Vt);
        const float s = det3(U) * det3(Vt);
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) { hdr->nCand = 0; hdr->status = 1; return; }
        const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
        const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
        const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
        const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
        const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
        const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
        for (int c = 0; c < 8; c++) {
            // x1 = {aux1, aux1, -aux1, -aux1}, x3 = {aux3, -aux3, aux3, -aux3}, stheta / sphi = {aux, -aux, -aux, aux}
            const int i = c & 3;
            const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
            const float sth = (i == 0 || i == 3) ? aux_stheta : -aux_stheta, sph = (i == 0 || i == 3) ? aux_sphi : -aux_sphi;
            float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3];
            double sc;
            if (c < 4) {
                Rp[0] = ctheta; Rp[2] = -sth; Rp[6] = sth; Rp[8] = ctheta;
                tp[0] = x1; tp[1] = 0.f; tp[2] = -x3;
                sc = (double)(d1 - d3);
            } else {
                Rp[0] = cphi; Rp[2] = sph; Rp[4] = -1.f; Rp[6] = sph; Rp[8] = -cphi;
                tp[0] = x1; tp[1] = 0.f; tp[2] = x3;
                sc = (double)(d1 + d3);
            }
            mm3(U, Rp, X, (double)s);
            mm3(X, Vt, hdr->R[c]);
            if (sc != 1.0) for (int k = 0; k < 3; k++) tp[k] = (float)((double)tp[k] * sc);   // tp *= d1 -+ d3
            float tv[3];
            mv3(U, tp, tv);
            const double a = 1. / norm3(tv);
            for (int k = 0; k < 3; k++) hdr->t[c][k] = expr_scale(tv[k], a);
        }
        hdr->nCand = 8;
        hdr->status = 0;
        return;
    }
    if (itF < 0) { hdr->nCand = 0; hdr->status = 2; return; }   // no hypothesis beat 0: false (a defined choice)
    // ReconstructF (:485-512): E21 = K.t()*F21*K, DecomposeE (:924-946)
    float E[9];
    mm3_t1(K, F21, X);
    mm3(X, K, E);
    svd3_lane(E, sAt, sVt, sW, U, w, Vt);
    float t[3] = {U[2], U[5], U[8]};
    const double a = 1. / norm3(t);
    for (int k = 0; k < 3; k++) t[k] = expr_scale(t[k], a);
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float R1[9], R2[9];
    mm3(U, Wm, X);
    mm3(X, Vt, R1);
    if (det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = expr_scale(R1[k], -1.0);
    mm3_t2(U, Wm, X);
    mm3(X, Vt, R2);
    if (det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = expr_scale(R2[k], -1.0);
    for (int k = 0; k < 9; k++) { hdr->R[0][k] = R1[k]; hdr->R[1][k] = R2[k]; hdr->R[2][k] = R1[k]; hdr->R[3][k] = R2[k]; }
    for (int k = 0; k < 3; k++) {
        const float t2 = expr_scale(t[k], -1.0);
        hdr->t[0][k] = t[k]; hdr->t[1][k] = t[k]; hdr->t[2][k] = t2; hdr->t[3][k] = t2;
    }
    hdr->nCand = 4;
    hdr->status = 0;
}

// ------------------------------------------------------------------ CheckRT: candidates x matches
// grid (ceil(N / kRtThreads), 8): blockIdx.y = candidate.  Per (candidate, match): flag 0 (not good), 1 (good, counted,
// cosParallax >= 0.99998: stored, not flagged) or 2 (good and flagged); rec = (x, y, z, cosParallax)
__global__ __launch_bounds__(kRtThreads) void k_init_checkrt(const Key* __restrict__ k1, const Key* __restrict__ k2, const Pair* __restrict__ pairs, int N,
                                                             float fx, float fy, float cx, float cy, float sigma, int hf, Hdr* hdr,
                                                             float4* __restrict__ rec, uint8_t* __restrict__ flag)
{
    __shared__ float sA[16 * kRtThreads], sV[16 * kRtThreads];
    __shared__ double sW[4 * kRtThreads];
    const int i = blockIdx.x * kRtThreads + threadIdx.x, c = blockIdx.y;
    if (i >= N) return;   // (no barrier below)
    const Pair p = pairs[i];
    const Key kp1 = k1[p.i1], kp2 = k2[p.i2];
    const float invS = inv_sigma_square(sigma);
    // the reference's vbMatchesInliersF / H: the winner's flags, recomputed
    float c1, c2;
    bool inF = false, inH = false;
    if (hdr->itF >= 0) { chi_f(hdr->F21, kp1.x, kp1.y, kp2.x, kp2.y, invS, c1, c2); inF = !(c1 > th_f()) && !(c2 > th_f()); }
    if (hf && hdr->itH >= 0) { chi_h(hdr->H21, hdr->H12, kp1.x, kp1.y, kp2.x, kp2.y, invS, c1, c2); inH = !(c1 > th_h()) && !(c2 > th_h()); }
    const bool in = hdr->reconH ? inH : inF;
    if (c == 0) {
        if (inF) atomicAdd(&hdr->nInliersF, 1);
        if (inH) atomicAdd(&hdr->nInliersH, 1);
        if (in) atomicAdd(&hdr->nInliers, 1);
    }
    if (c >= hdr->nCand) return;
    const size_t o = (size_t)c * N + i;
    if (!in) { flag[o] = 0; return; }
    float R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = hdr->R[c][k];
    for (int k = 0; k < 3; k++) t[k] = hdr->t[c][k];
    const float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    // P1 = K[I|0], P2 = K*[R|t] (gemm 3x3 * 3x4), O2 = -R.t()*t (GEMM_1_T, alpha -1)
    float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f}, P2[12], Rt[12], O2[3];
    for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) Rt[4 * r + k] = R[3 * r + k]; Rt[4 * r + 3] = t[r]; }
    for (int r = 0; r < 3; r++)
        for (int j = 0; j < 4; j++) P2[4 * r + j] = gemm3_elem(K[3 * r], K[3 * r + 1], K[3 * r + 2], Rt[j], Rt[4 + j], Rt[8 + j], 1.0, 0.f, 0.0);
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)R[3 * k + r] * (double)t[k];
        O2[r] = (float)(s * -1.0);
    }
    // Triangulate (:749-762): A.row(r) = x*P.row(2) - P.row(0|1) (addWeighted in double; x == 1: subtract), SVD 4x4
    float* At = sA + threadIdx.x;
    float* Vt = sV + threadIdx.x;
    double* W = sW + threadIdx.x;
    const float xs[4] = {kp1.x, kp1.y, kp2.x, kp2.y};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float* P = r < 2 ? P1 : P2;
        const int pr = r & 1;
        const float x = xs[r];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float v = x == 1.f ? P[8 + k] - P[4 * pr + k] : (float)((double)P[8 + k] * (double)x + (double)P[4 * pr + k] * -1.0 + 0.0);
            At[(k * 4 + r) * kRtThreads] = v;   // !at: temp_a = A.t()
        }
    }
    jacobi_svd<float, kRtThreads>(At, W, Vt, 4, 4, 4, true, false);
    const double alpha = 1. / (double)Vt[15 * kRtThreads];
    float X[3];
    for (int k = 0; k < 3; k++) X[k] = expr_scale(Vt[(12 + k) * kRtThreads], alpha);
    flag[o] = 0;
    if (!__builtin_isfinite(X[0]) || !__builtin_isfinite(X[1]) || !__builtin_isfinite(X[2])) return;
    float n1[3], n2[3];
    for (int k = 0; k < 3; k++) { n1[k] = X[k] - 0.f; n2[k] = X[k] - O2[k]; }
    const float dist1 = norm3(n1), dist2 = norm3(n2);
    double dt = 0;
    for (int k = 0; k < 3; k++) dt += (double)n1[k] * (double)n2[k];
    const float cosParallax = dt / (dist1 * dist2);
    if (X[2] <= 0 && cosParallax < 0.99998) return;
    float X2[3];
    for (int r = 0; r < 3; r++) X2[r] = gemm3_elem(R[3 * r], R[3 * r + 1], R[3 * r + 2], X[0], X[1], X[2], 1.0, t[r], 1.0);   // R*X + t: gemm with C
    if (X2[2] <= 0 && cosParallax < 0.99998) return;
    const float th2 = 4.0 * (double)(sigma * sigma);
    const float invZ1 = 1.0 / X[2];
    const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
    if ((im1x - kp1.x) * (im1x - kp1.x) + (im1y - kp1.y) * (im1y - kp1.y) > th2) return;
    const float invZ2 = 1.0 / X2[2];
    const float im2x = fx * X2[0] * invZ2 + cx, im2y = fy * X2[1] * invZ2 + cy;
    if ((im2x - kp2.x) * (im2x - kp2.x) + (im2y - kp2.y) * (im2y - kp2.y) > th2) return;
    rec[o] = make_float4(X[0], X[1], X[2], cosParallax);
    flag[o] = cosParallax < 0.99998 ? 2 : 1;
    atomicAdd(&hdr->nGood[c], 1);
}

// ------------------------------------------------------------------ the winning candidate, the parallax values, vP3D
__device__ __forceinline__ uint32_t ord_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_val(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// one block: kthCos[c] = the min(50, nGood - 1)-th smallest cosParallax of candidate c (radix select, 8 bits a pass);
// best = ReconstructF's first maxGood / ReconstructH's first strictly greater nGood; out = the winner's vP3D (n1 x 3)
// and vbTriangulated (n1), zeros elsewhere
__global__ __launch_bounds__(kWinThreads) void k_init_winner(Hdr* hdr, int N, int n1, const Pair* __restrict__ pairs, const float4* __restrict__ rec,
                                                             const uint8_t* __restrict__ flag, float* __restrict__ outP3D, uint8_t* __restrict__ outTri)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sPrefix, sMask;
    __shared__ int sK;
    const int nc = hdr->nCand;
    for (int c = 0; c < nc; c++) {
        const int g = hdr->nGood[c];
        if (g == 0) continue;
        if (threadIdx.x == 0) { sPrefix = 0; sMask = 0; sK = g - 1 < 50 ? g - 1 : 50; }
        __syncthreads();
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[threadIdx.x] = 0;
            __syncthreads();
            const uint32_t prefix = sPrefix, mask = sMask;
            for (int i = threadIdx.x; i < N; i += kWinThreads)
                if (flag[(size_t)c * N + i]) {
                    const uint32_t key = ord_key(rec[(size_t)c * N + i].w);
                    if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t acc = 0;
                for (uint32_t b = 0; b < 256; b++) {
                    if ((uint32_t)sK < acc + hist[b]) { sPrefix = prefix | (b << shift); sMask = mask | (255u << shift); sK -= (int)acc; break; }
                    acc += hist[b];
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) hdr->kthCos[c] = ord_val(sPrefix);
        __syncthreads();
    }
    int best = -1;
    if (nc == 4) {
        int mx = hdr->nGood[0];
        for (int c = 1; c < 4; c++) mx = max(mx, hdr->nGood[c]);
        for (int c = 0; c < 4 && best < 0; c++) if (hdr->nGood[c] == mx) best = c;
    } else if (nc == 8) {
        int bg = 0;
        for (int c = 0; c < 8; c++) if (hdr->nGood[c] > bg) { bg = hdr->nGood[c]; best = c; }
    }
    if (threadIdx.x == 0) hdr->best = best;
    for (int i = threadIdx.x; i < n1; i += kWinThreads) { outP3D[3 * i] = 0.f; outP3D[3 * i + 1] = 0.f; outP3D[3 * i + 2] = 0.f; outTri[i] = 0; }
    __syncthreads();
    if (best < 0) return;
    for (int i = threadIdx.x; i < N; i += kWinThreads) {
        const uint8_t f = flag[(size_t)best * N + i];
        if (!f) continue;
        const float4 r = rec[(size_t)best * N + i];
        const int j = pairs[i].i1;
        outP3D[3 * j] = r.x; outP3D[3 * j + 1] = r.y; outP3D[3 * j + 2] = r.z;
        outTri[j] = f == 2;
    }
}

}  // namespace orbi
