// orbn_kernels.hip -- the device side of KeyFrame::UpdateConnections' counting and ordering and of KeyFrameCulling's counts
// (part of orbslamm_hip.hip; ABI: include/orbslamm_covis.h; host side: orbn_host.inc).  Integers only.
// The targets are taken kChunk at a time; a chunk is one pass over the store, whatever the number of its targets:
//   k_mark          one workgroup per target: bit c of mark[p] for every point p of target c, under the chunk's generation tag;
//                   a second sighting of p in the same target sets kDupBit; (culling) clears p's histogram
//   k_conn_walk     one wave per keyframe slot j: its row once in 16-byte reads; per target bit the popcount of the ballot
//                   into lane c's sum; the column counter[.][j] is written by this wave alone, zeros included
//   k_conn_select   one workgroup per target: the row compacted in ascending slot, the maximum, the members >= th, and the
//                   ordered list by ranking every member against tiles of kSortTile keys in LDS
//   k_hist_walk     one wave per keyframe slot: the octave histogram of the observations of every marked point
//   k_cull          one workgroup per target: n_mps and n_redundant from the histograms' prefixes
// mark[p] = (tag << 32) | bits, as orbu's stamp: a max with (tag << 32) brings a stale word to this chunk's zero, then an or
// sets the bit; the or's return tells a thread that the bit was there already, which happens for exactly m - 1 of the m
// slots a point fills, in any order.  The atomics are max, or and add of integers: no result depends on their order.
// A point that fills two slots of one target is rare (the reference never makes one on purpose), so kDupBit sends the two
// walks onto a slow path that counts the target's row again; the fast path then needs one bit per target and point only.
#pragma once

namespace orbn {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 31;                    // targets per pass: bits 0 .. 30 of the mark
constexpr uint32_t kDupBit = 1u << 31;
constexpr int kBins = 16;                     // distinct octave values a store may hold (ORBN_MAX_OCTAVE_VALUES)
constexpr int kSortTile = 256;
constexpr int kNoVote = orbu::kNoVote;
enum { C_NCNT = 0, C_NORD, C_KFMAX, C_NMAX, C_STATUS, C_INTS = 8 };

struct Dev {
    unsigned long long* mark;    // [poolCap]
    uint32_t* hist;              // [poolCap * kBins], or null before the first culling call
    int32_t* cnt;                // [kChunk * kfcap]: counter[c][j]
    unsigned long long* keys;    // [kChunk * kfcap]: (weight << 32) | slot of the members >= th, ascending slot
    const uint8_t* oct;          // [kfcap * pitch], or null
    const uint32_t* poolFlags;
    int32_t poolCap;
    uint32_t gen;
};
// a chunk's rows, in the store's pinned block: row c at c * kfcap
struct ChunkOut { int32_t* hdr; int32_t* cntKf; int32_t* cntW; int32_t* ordKf; int32_t* ordW; };

__device__ __forceinline__ bool point_live(const Dev& d, int id) { return id >= 0 && id < d.poolCap && !(d.poolFlags[id] & 1); }
__device__ __forceinline__ uint32_t mark_bits(const Dev& d, int id)
{
    const unsigned long long w = d.mark[id];
    return (uint32_t)(w >> 32) == d.gen ? (uint32_t)w : 0u;
}

__global__ __launch_bounds__(kThreads) void k_mark(orbu::StoreDev s, Dev d, const int32_t* __restrict__ tg, int withHist)
{
    const int c = blockIdx.x;
    const int k = tg[c];
    if (k < 0 || k >= s.kfcap) return;
    const int4* row = (const int4*)(s.entries + (size_t)k * s.pitch);
    for (int e = threadIdx.x; e < s.pitch / 4; e += kThreads) {
        const int4 v = row[e];
        const int raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int id = raw[j] & ~kNoVote;
            if (raw[j] < 0 || !point_live(d, id)) continue;
            atomicMax(&d.mark[id], (unsigned long long)d.gen << 32);
            const unsigned long long old = atomicOr(&d.mark[id], 1ull << c);
            if ((old >> c) & 1) atomicOr(&d.mark[id], (unsigned long long)kDupBit);
            if (withHist) {   // (every target that holds the point stores the same zeros; the adds come in a later kernel)
                uint4* h = (uint4*)(d.hist + (size_t)id * kBins);
#pragma unroll
                for (int q = 0; q < kBins / 4; q++) h[q] = make_uint4(0, 0, 0, 0);
            }
        }
    }
}

// the slots of target row k that hold point id (bit 30 aside)
__device__ __forceinline__ int row_multiplicity(const orbu::StoreDev& s, int k, int id)
{
    int m = 0;
    if (k < 0 || k >= s.kfcap) return 0;
    const int32_t* row = s.entries + (size_t)k * s.pitch;
    for (int e = 0; e < s.pitch; e++) { const int v = row[e]; m += (v >= 0 && (v & ~kNoVote) == id) ? 1 : 0; }
    return m;
}

__global__ __launch_bounds__(kThreads) void k_conn_walk(orbu::StoreDev s, Dev d, const int32_t* __restrict__ tg, int nC, int hi)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= hi) return;   // (a whole wave)
    int acc = 0;           // lane c: counter[c][j] before the self test
    if (s.flags[j] & 2) {
        const int4* row = (const int4*)(s.entries + (size_t)j * s.pitch);
        const int n4 = s.pitch / 4;
        for (int e0 = 0; e0 < n4; e0 += 64) {
            const int4 v = e0 + lane < n4 ? row[e0 + lane] : make_int4(-1, -1, -1, -1);
            const int raw[4] = {v.x, v.y, v.z, v.w};
            uint32_t bits[4];
            uint32_t any = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {   // a voting entry: an observation (j, .) of its point
                bits[q] = (raw[q] >= 0 && !(raw[q] & kNoVote) && raw[q] < d.poolCap) ? mark_bits(d, raw[q]) : 0u;
                any |= bits[q];
            }
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) any |= (uint32_t)__shfl_xor((int)any, sh);
            uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)any);
            const bool dup = u & kDupBit;
            u &= ~kDupBit;
            while (u) {   // at most kChunk turns
                const int c = __ffs((int)u) - 1;
                u &= u - 1;
                int n = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) n += __popcll(__ballot((bits[q] >> c) & 1));
                if (lane == c) acc += n;
            }
            if (dup) {   // a point that fills m > 1 slots of a target counts m times: m - 1 more
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    unsigned long long m = __ballot((bits[q] & kDupBit) != 0);
                    while (m) {   // at most 64 turns
                        const int l = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const int id = __shfl(raw[q], l);
                        const uint32_t b = (uint32_t)__shfl((int)bits[q], l);
                        if (lane < nC && ((b >> lane) & 1)) acc += row_multiplicity(s, tg[lane], id) - 1;
                    }
                }
            }
        }
    }
    if (lane < nC) d.cnt[(size_t)lane * s.kfcap + j] = tg[lane] == j ? 0 : acc;   // :327 mit->first->mnId == mnId
}

__global__ __launch_bounds__(kThreads) void k_conn_select(orbu::StoreDev s, Dev d, int hi, int th, ChunkOut o)
{
    __shared__ int waveCnt[2][kWaves];
    __shared__ unsigned long long waveBest[kWaves];
    __shared__ unsigned long long tile[kSortTile];
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t r0 = (size_t)c * s.kfcap;
    // :345-357 in ascending slot: the row, the members >= th, the first with strictly the largest weight
    int nCnt = 0, nOrd = 0;
    unsigned long long best = 0;   // (weight << 32) | ~slot
    for (int base = 0; base < hi; base += kThreads) {
        const int k = base + t;
        const int w = k < hi ? d.cnt[r0 + k] : 0;
        const bool nz = w > 0, ge = nz && w >= th;
        const unsigned long long m1 = __ballot(nz), m2 = __ballot(ge);
        if (lane == 0) { waveCnt[0][wave] = __popcll(m1); waveCnt[1][wave] = __popcll(m2); }
        __syncthreads();
        int off1 = nCnt, off2 = nOrd, tot1 = 0, tot2 = 0;
        for (int q = 0; q < kWaves; q++) {
            if (q < wave) { off1 += waveCnt[0][q]; off2 += waveCnt[1][q]; }
            tot1 += waveCnt[0][q]; tot2 += waveCnt[1][q];
        }
        const unsigned long long below = (1ull << lane) - 1;
        if (nz) {
            const int pos = off1 + __popcll(m1 & below);
            o.cntKf[r0 + pos] = k; o.cntW[r0 + pos] = w;
            const unsigned long long key = ((unsigned long long)(uint32_t)w << 32) | (uint32_t)~(uint32_t)k;
            best = key > best ? key : best;
        }
        if (ge) d.keys[r0 + off2 + __popcll(m2 & below)] = ((unsigned long long)(uint32_t)w << 32) | (uint32_t)k;
        nCnt += tot1; nOrd += tot2;
        __syncthreads();
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_down((long long)best, sh);
        best = other > best ? other : best;
    }
    if (lane == 0) waveBest[wave] = best;
    __threadfence_block();
    __syncthreads();
    best = waveBest[0];
    for (int q = 1; q < kWaves; q++) best = waveBest[q] > best ? waveBest[q] : best;
    const int nMax = (int)(best >> 32), kfMax = nCnt ? (int)~(uint32_t)best : -1;
    int32_t* hdr = o.hdr + c * C_INTS;
    if (nCnt && !nOrd) {   // :359-363 the single maximum
        if (t == 0) { o.ordKf[r0] = kfMax; o.ordW[r0] = nMax; }
        nOrd = 1;
    } else {
        // :365-372 weight descending, slot descending: a key's place is the number of larger keys (the keys are distinct)
        for (int base = 0; base < nOrd; base += kThreads) {
            const int i = base + t;
            const unsigned long long mine = i < nOrd ? d.keys[r0 + i] : 0;
            int rank = 0;
            for (int t0 = 0; t0 < nOrd; t0 += kSortTile) {
                tile[t] = t0 + t < nOrd ? d.keys[r0 + t0 + t] : 0;
                __syncthreads();
                const int lim = min(kSortTile, nOrd - t0);
                for (int q = 0; q < lim; q++) rank += tile[q] > mine ? 1 : 0;
                __syncthreads();
            }
            if (i < nOrd) { o.ordKf[r0 + rank] = (int32_t)(uint32_t)mine; o.ordW[r0 + rank] = (int32_t)(mine >> 32); }
        }
    }
    if (t == 0) { hdr[C_NCNT] = nCnt; hdr[C_NORD] = nOrd; hdr[C_KFMAX] = kfMax; hdr[C_NMAX] = nMax; hdr[C_STATUS] = nCnt ? 0 : 1; }
}

// bin[256]: the rank of an octave byte among the values the store holds
__global__ __launch_bounds__(kThreads) void k_hist_walk(orbu::StoreDev s, Dev d, const uint8_t* __restrict__ bin, int hi)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= hi || !(s.flags[j] & 2)) return;
    const int4* row = (const int4*)(s.entries + (size_t)j * s.pitch);
    const uchar4* orow = (const uchar4*)(d.oct + (size_t)j * s.pitch);
    for (int e = lane; e < s.pitch / 4; e += 64) {
        const int4 v = row[e];
        const int raw[4] = {v.x, v.y, v.z, v.w};
        const uchar4 ov = orow[e];
        const uint8_t o[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (raw[q] >= 0 && !(raw[q] & kNoVote) && raw[q] < d.poolCap && mark_bits(d, raw[q]))
                atomicAdd(&d.hist[(size_t)raw[q] * kBins + min((int)bin[o[q]], kBins - 1)], 1u);
    }
}

// upto[257]: the largest rank whose value is <= t, or -1.  counts: n_mps, n_redundant per target of the whole call
__global__ __launch_bounds__(kThreads) void k_cull(orbu::StoreDev s, Dev d, const int32_t* __restrict__ tg, int thObs, const int8_t* __restrict__ upto,
                                                   int32_t* __restrict__ nMps, int32_t* __restrict__ nRed)
{
    __shared__ int tot[2];
    const int c = blockIdx.x, t = threadIdx.x;
    const int k = tg[c];
    if (t == 0) { tot[0] = 0; tot[1] = 0; }
    __syncthreads();
    int nm = 0, nr = 0;
    if (k >= 0 && k < s.kfcap) {
        const int32_t* row = s.entries + (size_t)k * s.pitch;
        const uint8_t* orow = d.oct + (size_t)k * s.pitch;
        for (int e = t; e < s.pitch; e += kThreads) {
            const int raw = row[e];
            const int id = raw & ~kNoVote;
            if (raw < 0 || !point_live(d, id)) continue;   // :656, :658
            nm++;                                          // :666
            const uint4* hp = (const uint4*)(d.hist + (size_t)id * kBins);
            uint32_t h[kBins];
#pragma unroll
            for (int q = 0; q < kBins / 4; q++) { const uint4 x = hp[q]; h[4 * q] = x.x; h[4 * q + 1] = x.y; h[4 * q + 2] = x.z; h[4 * q + 3] = x.w; }
            const int lvl = (int)orow[e] + 1;              // :679 scaleLevel + 1
            const int r = upto[lvl];
            uint32_t all = 0, le = 0;
#pragma unroll
            for (int q = 0; q < kBins; q++) { all += h[q]; le += q <= r ? h[q] : 0u; }
            if ((long long)all <= (long long)thObs) continue;   // :667 Observations() > thObs
            // :675 pKFi == pKF: the target's own observations of the point at or below the level
            int own;
            if (mark_bits(d, id) & kDupBit) {
                own = 0;
                for (int e2 = 0; e2 < s.pitch; e2++) own += (row[e2] == id && (int)orow[e2] <= lvl) ? 1 : 0;
            } else
                own = (raw & kNoVote) ? 0 : 1;
            if ((long long)le - own >= (long long)thObs) nr++;   // :686
        }
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) { nm += __shfl_down(nm, sh); nr += __shfl_down(nr, sh); }
    if ((t & 63) == 0) { atomicAdd(&tot[0], nm); atomicAdd(&tot[1], nr); }
    __syncthreads();
    if (t == 0) { nMps[c] = tot[0]; nRed[c] = tot[1]; }
}

}  // namespace orbn
