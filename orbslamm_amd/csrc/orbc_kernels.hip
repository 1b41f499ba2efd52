// orbc_kernels.hip -- device side of SearchAndFuse (part of orbslamm_hip.hip; host side: orbc_host.inc, ABI:
// include/orbslamm_loopfuse.h): the searches of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (ORBmatcher.cc:1010-1081, monocular) of every point against every target, T x P pairs, in three launches however many
// targets there are.
//   k_loopfuse_search   one workgroup per (target, tile of kTile consecutive points).  One lane per pair for the projection
//                       gates (orbf::project_gates, orbf_kernels.hip); the survivors are compacted by ballot
//                       into LDS in point order; kLpp lanes per survivor walk its window together (orbf::window_best:
//                       no chi-square test, :1053-1081, the strict `<` of :1076).  A pair with bestIdx >= 0 &&
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
    const orbf::FuseTgt* tgt; const orbf::FusePt* pts;
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
    const orbf::FuseTgt& T = a.tgt[k];
    const orbm::GridDev grid = T.grid;
    // 1. the projection gates (:1010-1051), one lane per pair
    bool alive = false;
    float u = 0.f, v = 0.f;
    int level = -1;
    if (inRange) {
        uint8_t st;
        alive = orbf::project_gates(T, a.pts[p], a.nlevels, a.breaks, u, v, level, st);
        if (a.status && !alive) a.status[(int64_t)k * a.nPoints + p] = st;
    }
    sWord[tid] = kNoHit;
    // the survivors, in point order
    int nSurv;
    const int s0 = orbf::block_rank<kTile>(alive, sWave, nSurv);
    if (nSurv == 0) {   // (the whole workgroup: nSurv is one value)
        if (tid == 0) a.tileCnt[tile] = 0;
        return;
    }
    if (alive) { sU[s0] = u; sV[s0] = v; sLocal[s0] = tid; sLevel[s0] = level; }
    __syncthreads();
    // 2. kLpp lanes per survivor: :1053-1081
    const int sub = tid % kLpp;
    for (int s = tid / kLpp; s < nSurv; s += kTile / kLpp) {
        // (the lanes of a survivor read the same s: the same u, v and level, as window_best asks)
        const int pred = sLevel[s], local = sLocal[s];
        int bestDist, bestIdx;
        orbf::window_best<kLpp>(T, grid, a.pts[p - tid + local].desc, sub, sU[s], sV[s], pred, a.th * a.sf[pred], bestDist, bestIdx);
        if (sub == 0) {
            if (bestIdx >= 0 && bestDist <= a.maxDist) sWord[local] = ((uint32_t)bestDist << 16) | (uint32_t)bestIdx;   // (bestIdx < 65536)
            if (a.status) a.status[(int64_t)k * a.nPoints + (p - tid + local)] = bestIdx >= 0 ? orbf::FST_FOUND : orbf::FST_NO_CANDIDATE;
        }
    }
    __syncthreads();
    const uint32_t word = sWord[tid];
    if (inRange) a.pair[(int64_t)k * a.nPoints + p] = word;
    int nHit;
    (void)orbf::block_rank<kTile>(word != kNoHit, sWave2, nHit);
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
    const int r = orbf::block_rank<kTile>(word != kNoHit, sWave, all);
    if (word != kNoHit && base + r < a.capacity) {   // (more hits than the capacity: the host reports the count and copies nothing)
        Hit h;
        h.target = k; h.point = p; h.bestIdx = (int32_t)(word & 0xFFFFu); h.bestDist = (int32_t)(word >> 16);
        a.hits[base + r] = h;
    }
}

}  // namespace orbc
