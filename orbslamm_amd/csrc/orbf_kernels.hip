// orbf_kernels.hip -- the device pieces that the two batched ORBmatcher::Fuse searches share (part of orbslamm_hip.hip;
// DESIGN.md §8n): k_fuse_batch (orbl_kernels.hip, SearchInNeighbors, §8l) and k_loopfuse_search (orbc_kernels.hip,
// SearchAndFuse, §8m).  Host side: orbf_host.inc.
//   FuseTgt, FusePt, FST_*   a target keyframe and a map point as both kernels read them, and the status byte of a pair
//   project_gates            the five projection gates and PredictScale of ONE (target, point) pair (ORBmatcher.cc:855-892
//                            and :1010-1051: the same statements)
//   sim3_gates               the gates of ONE point in one direction of SearchBySim3 (:1160-1191, :1240-1271; orby_kernels.hip)
//   predict_level            PredictScale through the break table, under both gate sets
//   window_best<Lpp>         the window walk of ONE survivor by Lpp lanes without the chi-square test (:1053-1081);
//                            k_fuse_batch keeps its own walk with the test (:894-951), see there
//   block_rank<Threads>      the rank of a flag inside a workgroup by ballot and wave counts
// A kernel keeps its tiling, its LDS arrays, its output record and its early exit.
// Arithmetic: one IEEE operation per source operation (the library is built with -ffp-contract=off); OpenCV's pieces are
// orbx_cvmath.hpp's.
#pragma once

namespace orbf {

// the status codes of include/orbslamm_fuse.h (ORBL_FUSE_ST_*)
enum : uint8_t { FST_DEPTH = 0, FST_OUTSIDE_IMAGE, FST_DISTANCE, FST_VIEW_ANGLE, FST_LEVEL_RANGE, FST_NO_CANDIDATE, FST_FOUND };

struct FuseTgt {
    const orbm::KeyDev* keys; const uint8_t* desc; const int32_t* cellStart; const int32_t* cellIdx;
    orbm::GridDev grid;
    float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, minX, maxX, minY, maxY;
    int32_t n;
};
struct FusePt { float pos[3], normal[3], minDistance, maxDistance; uint32_t desc[8]; };       // OrblFusePoint

// PredictScale (MapPoint.cc:385-394) through the break table: the breaks below ratio = maxDistance / dist3D (a NaN ratio is above
// none).  True: the level lies inside [0, nlevels).
__device__ __forceinline__ bool predict_level(float maxDistance, float dist3D, int nlevels, const float* breaks, int& level)
{
    const float ratio = __fdiv_rn(maxDistance, dist3D);
    int c = 0;
    for (int j = 0; j <= nlevels; j++) c += ratio > breaks[j] ? 1 : 0;
    level = c - 1;
    return c >= 1 && c <= nlevels;
}

// The projection gates of one pair.  True: the pair reaches the window search at (u, v) and `level`.  False: `st` names
// the gate that ended it (u, v set once the depth gate is passed, level once PredictScale has run).
__device__ __forceinline__ bool project_gates(const FuseTgt& T, const FusePt& P, int nlevels, const float* breaks, float& u, float& v,
                                              int& level, uint8_t& st)
{
    u = 0.f; v = 0.f; level = -1; st = FST_DEPTH;
    const float X[3] = {P.pos[0], P.pos[1], P.pos[2]};
    float pc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) pc[i] = cvm::gemm3_elem(T.Rcw[3 * i], T.Rcw[3 * i + 1], T.Rcw[3 * i + 2], X[0], X[1], X[2], 1.0, T.tcw[i], 1.0);
    if (pc[2] < 0.0f) return false;
    const float invz = __fdiv_rn(1.f, pc[2]);   // (float)(1.0 / (double)z) of :1021: the same bits (orbslamm_loopfuse.h)
    const float x = pc[0] * invz, y = pc[1] * invz;
    u = T.fx * x + T.cx; v = T.fy * y + T.cy;
    st = FST_OUTSIDE_IMAGE;
    if (!(u >= T.minX && u < T.maxX && v >= T.minY && v < T.maxY)) return false;
    const float maxDistance = 1.2f * P.maxDistance, minDistance = 0.8f * P.minDistance;
    const float PO[3] = {X[0] - T.Ow[0], X[1] - T.Ow[1], X[2] - T.Ow[2]};
    const float dist3D = (float)cvm::norm3(PO);
    st = FST_DISTANCE;
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    double dt = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) dt += (double)PO[i] * (double)P.normal[i];
    st = FST_VIEW_ANGLE;
    if (dt < 0.5 * (double)dist3D) return false;
    st = FST_LEVEL_RANGE;
    return predict_level(P.maxDistance, dist3D, nlevels, breaks, level);
}

// The gates of one point in one direction of SearchBySim3 (ORBmatcher.cc:1160-1191 and :1240-1271: the same statements): X, the
// point in the camera frame of the keyframe it comes FROM, moved by (sR, t) into the keyframe searched; K1 = pKF1's fx fy cx cy in
// both directions (:1107-1110, sic); bounds = mnMinX, mnMaxX, mnMinY, mnMaxY of the keyframe searched (KeyFrame::IsInImage: >= min,
// < max); minD, maxD the point's raw mfMinDistance, mfMaxDistance.  No viewing-angle gate.  `failed` counts the gates passed before
// the one that ended it: 0 depth, 1 image, 2 distance, 3 level; true: (u, v) and level stand.
__device__ __forceinline__ bool sim3_gates(const float* sR, const float* t, const float* X, const float* K1, const float* bounds, float minD,
                                           float maxD, int nlevels, const float* breaks, float& u, float& v, int& level, int& failed)
{
    u = 0.f; v = 0.f; level = -1; failed = 0;
    float pt[3];
#pragma unroll
    for (int i = 0; i < 3; i++) pt[i] = cvm::gemm3_elem(sR[3 * i], sR[3 * i + 1], sR[3 * i + 2], X[0], X[1], X[2], 1.0, t[i], 1.0);
    if (pt[2] < 0.0f) return false;
    const float invz = (float)(1.0 / (double)pt[2]);   // :1168
    const float x = pt[0] * invz, y = pt[1] * invz;
    u = K1[0] * x + K1[2]; v = K1[1] * y + K1[3];
    failed = 1;
    if (!(u >= bounds[0] && u < bounds[1] && v >= bounds[2] && v < bounds[3])) return false;
    const float maxDistance = 1.2f * maxD, minDistance = 0.8f * minD;
    const float dist3D = (float)cvm::norm3(pt);
    failed = 2;
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    failed = 3;
    return predict_level(maxD, dist3D, nlevels, breaks, level);
}

// The window walk of one survivor in GetFeaturesInArea's order, levels pred - 1..pred, no chi-square test (:1053-1081).
// Lane `sub` of the survivor's Lpp holds 32 / Lpp bytes of the point's descriptor `qdesc` and reads that share of a
// candidate's (one 32-byte line per candidate and group instead of a 32-byte gather per lane); the partial popcounts are
// summed across the group, and every lane keeps the same (bestDist, bestIdx) under the strict `<` of k_window_best.  ALL
// Lpp lanes of a group must call it with the same u, v and pred: then they take the same path through the walk and the
// shuffle partners are active.  k_fuse_batch's walk (the same with the 5.99 test of :905-917) is written out in that
// kernel: a fix to one is a fix to the other.
template <int Lpp>
__device__ __forceinline__ void window_best(const FuseTgt& T, const orbm::GridDev& grid, const uint32_t* qdesc, int sub, float u, float v, int pred,
                                            float radius, int& bestDist, int& bestIdx)
{
    constexpr int W = 8 / Lpp;
    uint32_t qw[W];
    const uint32_t* qp = qdesc + sub * W;
#pragma unroll
    for (int i = 0; i < W; i++) qw[i] = qp[i];
    int bd = 256, bi = -1;
    orbm::for_each_in_area(grid, T.keys, T.cellStart, T.cellIdx, u, v, radius, -1, -1, [&](int idx) {
        const orbm::KeyDev& kp = T.keys[idx];
        const int kpLevel = kp.octave;
        if (kpLevel < pred - 1 || kpLevel > pred) return;
        const uint32_t* tp = (const uint32_t*)(T.desc + (int64_t)idx * 32) + sub * W;
        int d = 0;
#pragma unroll
        for (int i = 0; i < W; i++) d += __popc(qw[i] ^ tp[i]);
#pragma unroll
        for (int k = Lpp / 2; k >= 1; k >>= 1) d += __shfl_xor(d, k);
        if (d < bd) { bd = d; bi = idx; }
    });
    bestDist = bd; bestIdx = bi;
}

// the set lanes of `flag` in front of this thread in a workgroup of Threads, and in all of it.  sWave: Threads / 64 ints in
// LDS; a caller that ranks again through the same sWave puts a __syncthreads() in front of the call (the earlier reads).
template <int Threads>
__device__ __forceinline__ int block_rank(bool flag, int* sWave, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) sWave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < Threads / 64; w++) { const int c = sWave[w]; all += c; if (w < wave) before += c; }
    total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

}  // namespace orbf
