// orbc_kernels.hip -- device side of SearchAndFuse (part of orbslamm_hip.hip; host side: orbc_host.inc, ABI:
// include/orbslamm_loopfuse.h): the searches of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (ORBmatcher.cc:1010-1081, monocular) of every point against every target, T x P pairs, in three launches however many
// targets there are.
//   k_loopfuse_search   one workgroup per (target, tile of kTile consecutive points).  One lane per pair for the five
//                       projection gates in orbx_cvmath.hpp's forms, the level from the break table; the survivors are
//                       compacted by ballot into LDS in point order; kLpp lanes per survivor walk its window together in
//                       GetFeaturesInArea's order (for_each_in_area), each lane holding 32 / kLpp bytes of the point's
//                       descriptor, with the strict `<` of :1076.  NO chi-square test.  A pair with bestIdx >= 0 &&
//                       bestDist <= maxDist is a hit: its word (bestDist << 16 | bestIdx) goes to pair[k * P + i], every
//                       other pair's word is kNoHit, and the tile's hits are counted.  A tile without a survivor (most
//                       tiles of a keyframe that looks away) writes its zero count and nothing else.
//   k_scan_small        (orbm) the exclusive scan of the tile counts: a tile's place in the hit list.
//   k_loopfuse_compact  one workgroup per tile with hits: the tile's words, ranked by ballot, written as OrbcHit records
//                       behind the earlier tiles' (target-major, points ascending), and hit_start.
// No atomics: every word and record is written by exactly one lane, at a place the counts alone decide.
// kTile and kLpp are build-time choices (-DORBC_TILE=128|256|512, -DORBC_LPP=1|2|4|8) so that tools/loopfuse_bench.py can A/B
// them; 512 x 1 measured best: with a launch full of survivors the lanes of a group only repeat each other's walk
// (docs/experiments.md, "k_loopfuse_search, tile and lanes per survivor").
#pragma once

namespace orbc {

#ifndef ORBC_TILE
#define ORBC_TILE 512
#endif
#ifndef ORBC_LPP
#define ORBC_LPP 1
#endif
constexpr int kTile = ORBC_TILE;
constexpr int kLpp = ORBC_LPP;
static_assert(kTile == 128 || kTile == 256 || kTile == 512, "points per tile");
static_assert(kLpp == 1 || kLpp == 2 || kLpp == 4 || kLpp == 8, "lanes per survivor");
constexpr uint32_t kNoHit = 0xFFFFFFFFu;

struct Hit { int32_t target, point, bestIdx, bestDist; };   // OrbcHit
struct Args {
    const orbl::FuseTgt* tgt; const orbl::FusePt* pts;
    uint32_t* pair;        // T * P words between the search and the compaction (only the tiles with a survivor are written)
    int32_t* tileCnt;      // nTiles
    const int32_t* tileOff;  // nTiles + 1: the scan of tileCnt
    int32_t* hitStart;     // T + 1
    Hit* hits;             // capacity records
    uint8_t* status;       // T * P, or null
    int32_t nTargets, nPoints, tilesPerTarget, nTiles, capacity, maxDist, nlevels;
    float th;
    float sf[16], breaks[17];
};

// the set lanes of `flag` in front of this thread in the workgroup, and in all of it
__device__ __forceinline__ int tile_rank(bool flag, int* sWave, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) sWave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kTile / 64; w++) { const int c = sWave[w]; all += c; if (w < wave) before += c; }
    total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kTile) void k_loopfuse_search(Args a)
{
    __shared__ float sU[kTile], sV[kTile];
    __shared__ int32_t sLocal[kTile], sLevel[kTile];
    __shared__ uint32_t sWord[kTile];
    __shared__ int sWave[kTile / 64], sWave2[kTile / 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int k = tile / a.tilesPerTarget;
    const int p = (tile - k * a.tilesPerTarget) * kTile + tid;
    const bool inRange = p < a.nPoints;
    const orbl::FuseTgt& T = a.tgt[k];
    const orbm::GridDev grid = T.grid;
    // 1. the projection gates (:1010-1051), one lane per pair
    bool alive = false;
    uint8_t st = orbl::FST_DEPTH;
    float u = 0.f, v = 0.f;
    int level = -1;
    if (inRange) {
        const orbl::FusePt& P = a.pts[p];
        const float X[3] = {P.pos[0], P.pos[1], P.pos[2]};
        float pc[3];
#pragma unroll
        for (int i = 0; i < 3; i++) pc[i] = cvm::gemm3_elem(T.Rcw[3 * i], T.Rcw[3 * i + 1], T.Rcw[3 * i + 2], X[0], X[1], X[2], 1.0, T.tcw[i], 1.0);
        if (!(pc[2] < 0.0f)) {
            const float invz = __fdiv_rn(1.f, pc[2]);   // (float)(1.0 / (double)z): the same bits (orbslamm_loopfuse.h)
            const float x = pc[0] * invz, y = pc[1] * invz;
            u = T.fx * x + T.cx; v = T.fy * y + T.cy;
            st = orbl::FST_OUTSIDE_IMAGE;
            if (u >= T.minX && u < T.maxX && v >= T.minY && v < T.maxY) {
                const float maxDistance = 1.2f * P.maxDistance, minDistance = 0.8f * P.minDistance;
                const float PO[3] = {X[0] - T.Ow[0], X[1] - T.Ow[1], X[2] - T.Ow[2]};
                const float dist3D = (float)cvm::norm3(PO);
                st = orbl::FST_DISTANCE;
                if (!(dist3D < minDistance || dist3D > maxDistance)) {
                    double dt = 0;
#pragma unroll
                    for (int i = 0; i < 3; i++) dt += (double)PO[i] * (double)P.normal[i];
                    st = orbl::FST_VIEW_ANGLE;
                    if (!(dt < 0.5 * (double)dist3D)) {
                        // PredictScale: the breaks below ratio (a NaN ratio is above none)
                        const float ratio = __fdiv_rn(P.maxDistance, dist3D);
                        int c = 0;
                        for (int j = 0; j <= a.nlevels; j++) c += ratio > a.breaks[j] ? 1 : 0;
                        level = c - 1;
                        st = orbl::FST_LEVEL_RANGE;
                        alive = c >= 1 && c <= a.nlevels;
                    }
                }
            }
        }
        if (a.status && !alive) a.status[(int64_t)k * a.nPoints + p] = st;
    }
    sWord[tid] = kNoHit;
    // the survivors, in point order
    int nSurv;
    const int s0 = tile_rank(alive, sWave, nSurv);
    if (nSurv == 0) {   // (the whole workgroup: nSurv is one value)
        if (tid == 0) a.tileCnt[tile] = 0;
        return;
    }
    if (alive) { sU[s0] = u; sV[s0] = v; sLocal[s0] = tid; sLevel[s0] = level; }
    __syncthreads();
    // 2. kLpp lanes per survivor: :1053-1081
    constexpr int W = 8 / kLpp;
    const int sub = tid % kLpp;
    for (int s = tid / kLpp; s < nSurv; s += kTile / kLpp) {
        const float su = sU[s], sv = sV[s];
        const int pred = sLevel[s], local = sLocal[s];
        const float radius = a.th * a.sf[pred];
        uint32_t qw[W];
        const uint32_t* qp = a.pts[p - tid + local].desc + sub * W;
#pragma unroll
        for (int i = 0; i < W; i++) qw[i] = qp[i];
        int bestDist = 256, bestIdx = -1;
        orbm::for_each_in_area(grid, T.keys, T.cellStart, T.cellIdx, su, sv, radius, -1, -1, [&](int idx) {
            const int kpLevel = T.keys[idx].octave;
            if (kpLevel < pred - 1 || kpLevel > pred) return;
            const uint32_t* tp = (const uint32_t*)(T.desc + (int64_t)idx * 32) + sub * W;
            int d = 0;
#pragma unroll
            for (int i = 0; i < W; i++) d += __popc(qw[i] ^ tp[i]);
            // (the lanes of a survivor take the same path through the walk: their partners are active here)
#pragma unroll
            for (int j = kLpp / 2; j >= 1; j >>= 1) d += __shfl_xor(d, j);
            if (d < bestDist) { bestDist = d; bestIdx = idx; }
        });
        if (sub == 0) {
            if (bestIdx >= 0 && bestDist <= a.maxDist) sWord[local] = ((uint32_t)bestDist << 16) | (uint32_t)bestIdx;   // (bestIdx < 65536)
            if (a.status) a.status[(int64_t)k * a.nPoints + (p - tid + local)] = bestIdx >= 0 ? orbl::FST_FOUND : orbl::FST_NO_CANDIDATE;
        }
    }
    __syncthreads();
    const uint32_t word = sWord[tid];
    if (inRange) a.pair[(int64_t)k * a.nPoints + p] = word;
    int nHit;
    (void)tile_rank(word != kNoHit, sWave2, nHit);
    if (tid == 0) a.tileCnt[tile] = nHit;
}

__global__ __launch_bounds__(kTile) void k_loopfuse_compact(Args a)
{
    __shared__ int sWave[kTile / 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int k = tile / a.tilesPerTarget;
    const int first = tile - k * a.tilesPerTarget;
    const int base = a.tileOff[tile], cnt = a.tileOff[tile + 1] - base;
    if (tid == 0) {
        if (first == 0) a.hitStart[k] = base;
        if (tile == a.nTiles - 1) a.hitStart[a.nTargets] = base + cnt;
    }
    if (cnt == 0) return;
    const int p = first * kTile + tid;
    const uint32_t word = p < a.nPoints ? a.pair[(int64_t)k * a.nPoints + p] : kNoHit;
    int all;
    const int r = tile_rank(word != kNoHit, sWave, all);
    if (word != kNoHit && base + r < a.capacity) {   // (more hits than the capacity: the host reports the count and copies nothing)
        Hit h;
        h.target = k; h.point = p; h.bestIdx = (int32_t)(word & 0xFFFFu); h.bestDist = (int32_t)(word >> 16);
        a.hits[base + r] = h;
    }
}

}  // namespace orbc
