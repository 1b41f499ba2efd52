// orbr_kernels.hip -- the device side of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth over the
// keyframe store, refreshing the pool's records in place (part of orbslamm_hip.hip; ABI: include/orbslamm_refresh.h, DESIGN.md
// §8w; host side: orbr_host.inc).
//   k_desc_scatter / k_centre_scatter   the setters' staged rows into the store's descriptor block and centres
//   k_pool_gather     orbw_debug_pool_get: pool records into the pinned staging
//   k_mark            mark[id] = (tag << 32) | position in ids, under the store's generation tag; the per-point counters cleared
//   k_walk            one wave per keyframe slot, its entry row once in 16-byte reads: pass 0 counts the voting entries of
//                     every marked point, pass 1 claims a place in the point's segment and leaves the key (slot << 13) | q
//   k_segments        one thread per listed point: its segment's start, the error word for more than kMaxObs observations, and
//                     the two work lists (at most kGroup observations / more)
//   k_refresh_short   kGroup lanes a point, four points a wave; k_refresh_long one workgroup a point, up to kMaxObs observations
//   k_commit          one thread per listed point scatters the record into the pool's arrays
// The atomics are integer adds (counts, the claim of a place, a segment's start, a list's next place) and one LDS minimum:
// both refresh kernels sort a segment by key before they read it, so the order of the observations is ascending (slot, q)
// whatever the placement was, and a point's record depends on nothing but its own segment's content.
// Arithmetic: one IEEE operation per source operation (-ffp-contract=off); OpenCV's pieces are orbx_cvmath.hpp's.
#pragma once

namespace orbr {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroup = 16;                       // lanes a point on the short path
constexpr int kGroups = kThreads / kGroup;       // points a workgroup
constexpr int kMaxObs = 1024;                    // ORBR_MAX_OBS
constexpr int kQBits = 13;                       // ORBU_MAX_STRIDE = 1 << 13: a key is (slot << 13) | q, below 2^30
constexpr int kNoVote = orbu::kNoVote;
constexpr int kRecWords = 21;                    // OrbrPoint as 32-bit words
enum : uint32_t { ST_NOT_ASKED = 0, ST_DONE, ST_BAD, ST_NO_OBSERVATION, ST_ALL_KF_BAD, ST_NO_REF, ST_LEVEL_RANGE };
enum { H_TOTAL = 0, H_NSHORT, H_NLONG, H_ERR, H_INTS = 4 };
enum { R_POS = 0, R_NORMAL = 3, R_MIN = 6, R_MAX = 7, R_DESC = 8, R_NOBS = 16, R_NDESC = 17, R_BESTKF = 18, R_BESTIDX = 19, R_STATUS = 20 };

struct Dev {
    unsigned long long* mark;   // [poolCap]
    int32_t* cnt;               // [n] observations of listed point i
    int32_t* start;             // [n] its segment in keys
    int32_t* fill;              // [n] places claimed so far
    int32_t* listShort;         // [n]
    int32_t* listLong;          // [n]
    int32_t* hdr;               // [H_INTS]
    uint32_t* keys;             // [keysCap]
    uint32_t* res;              // [n * kRecWords]
    const uint8_t* desc;        // the store's descriptor block [kfcap * pitch * 32], or null
    const float* ctr;           // [kfcap * 3], or null
    const uint8_t* oct;         // [kfcap * pitch], or null
    orbw::PoolDev pool;
    int32_t keysCap;
    uint32_t gen;
};
// a call's arguments where the host staged them (pinned memory, read where it lies)
struct Call {
    const int32_t* ids; const int32_t* ref; const float* newPos; const float* sf;
    int32_t n, what, nlevels;
};

__global__ __launch_bounds__(kThreads) void k_desc_scatter(uint8_t* __restrict__ dst, const uint4* __restrict__ staged, int n16)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n16) ((uint4*)dst)[i] = staged[i];
}

// staged: {slot, x, y, z} as four words; slots are distinct within a launch and inside the store (checked on the host)
__global__ __launch_bounds__(kThreads) void k_centre_scatter(float* __restrict__ ctr, int kfcap, const uint4* __restrict__ staged, int n)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint4 r = staged[i];
    if (r.x >= (uint32_t)kfcap) return;
    ctr[3 * (size_t)r.x] = __uint_as_float(r.y); ctr[3 * (size_t)r.x + 1] = __uint_as_float(r.z); ctr[3 * (size_t)r.x + 2] = __uint_as_float(r.w);
}

// a record as k_pool_scatter takes it: five 16-byte pieces; an id outside the pool (never: checked on the host) gives zeros
__global__ __launch_bounds__(kThreads) void k_pool_gather(orbw::PoolDev pool, const int32_t* __restrict__ ids, int n, uint4* __restrict__ out)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    uint4* o = out + 5 * (size_t)i;
    if (id < 0 || id >= pool.cap) {
        const uint4 zero = make_uint4(0, 0, 0, 0);
        o[0] = zero; o[1] = zero; o[2] = zero; o[3] = zero; o[4] = make_uint4(0u, (uint32_t)id, 0u, 0u);
        return;
    }
    const float4 a = pool.a[id], b = pool.b[id];
    o[0] = make_uint4(__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(a.z), __float_as_uint(a.w));
    o[1] = make_uint4(__float_as_uint(b.x), __float_as_uint(b.y), __float_as_uint(b.z), __float_as_uint(b.w));
    o[2] = pool.desc[2 * (size_t)id];
    o[3] = pool.desc[2 * (size_t)id + 1];
    o[4] = make_uint4(pool.flags[id], (uint32_t)id, 0u, 0u);
}

__global__ __launch_bounds__(kThreads) void k_mark(Dev d, Call c)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) { d.hdr[H_TOTAL] = 0; d.hdr[H_NSHORT] = 0; d.hdr[H_NLONG] = 0; d.hdr[H_ERR] = 0; }
    if (i >= c.n) return;
    const int id = c.ids[i];
    if (id >= 0 && id < d.pool.cap) d.mark[id] = ((unsigned long long)d.gen << 32) | (uint32_t)i;   // (ids are distinct within a call)
    d.cnt[i] = 0; d.fill[i] = 0;
}

__global__ __launch_bounds__(kThreads) void k_walk(orbu::StoreDev s, Dev d, int n, int hi, int place)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= hi || !(s.flags[j] & 2)) return;   // (a whole wave)
    const int4* row = (const int4*)(s.entries + (size_t)j * s.pitch);
    const int n4 = s.pitch / 4;
    for (int e = lane; e < n4; e += 64) {
        const int4 v = row[e];
        const int raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {   // a voting entry: an observation (j, 4 e + q) of its point
            const int r = raw[q];
            if (r < 0 || (r & kNoVote) || r >= d.pool.cap) continue;
            const unsigned long long w = d.mark[r];
            if ((uint32_t)(w >> 32) != d.gen) continue;
            const int pos = (int)(uint32_t)w;
            if (pos >= n) continue;
            if (!place) { atomicAdd(&d.cnt[pos], 1); continue; }
            const int k = atomicAdd(&d.fill[pos], 1);
            const long long at = (long long)d.start[pos] + k;
            if (k < d.cnt[pos] && at >= 0 && at < d.keysCap) d.keys[at] = ((uint32_t)j << kQBits) | (uint32_t)(4 * e + q);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_segments(Dev d, int n)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = d.cnt[i];
    d.start[i] = atomicAdd(&d.hdr[H_TOTAL], c);
    if (c > kMaxObs) atomicOr(&d.hdr[H_ERR], 1);
    else if (c <= kGroup) d.listShort[atomicAdd(&d.hdr[H_NSHORT], 1)] = i;
    else d.listLong[atomicAdd(&d.hdr[H_NLONG], 1)] = i;
}

__device__ __forceinline__ int hamming8(const uint32_t* a, const uint32_t* b)
{
    int s = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) s += __popc(a[w] ^ b[w]);
    return s;
}

// one observation's term of the normal's sum: (P - Ow) * (float)(1. / cv::norm(P - Ow)), MapPoint.cc:354-355
__device__ __forceinline__ void normal_term(const float* P, const float* Ow, float* t)
{
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = P[c] - Ow[c];
    const double nd = cvm::norm3(v);
    const float a = (float)(1. / nd);
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = v[c] * a;
}

// what one thread per point writes behind the two halves: everything of the record but the descriptor words
struct Verdict {
    float P[3], normal[3], minD, maxD;   // the pool's, or the half's
    int nObs, nDesc, bestKf, bestIdx;
    uint32_t stD, stN;
};

// the statuses and the depth bounds (MapPoint.cc:251-269, :338-345, :359-368).  refQ: the reference keyframe's feature, or -1
__device__ __forceinline__ void verdict(const orbu::StoreDev& s, const Dev& d, const Call& c, int id, int ref, int refQ, const float* normal, uint32_t bestKey, Verdict& v)
{
    const float4 A = d.pool.a[id], B = d.pool.b[id];
    const bool bad = d.pool.flags[id] & 1;
    v.normal[0] = B.x; v.normal[1] = B.y; v.normal[2] = B.z; v.minD = A.w; v.maxD = B.w;
    v.bestKf = -1; v.bestIdx = -1;
    v.stD = !(c.what & 1) ? ST_NOT_ASKED : bad ? ST_BAD : v.nObs == 0 ? ST_NO_OBSERVATION : v.nDesc == 0 ? ST_ALL_KF_BAD : ST_DONE;
    if (v.stD == ST_DONE) { v.bestKf = (int)(bestKey >> kQBits); v.bestIdx = (int)(bestKey & ((1u << kQBits) - 1)); }
    v.stN = !(c.what & 2) ? ST_NOT_ASKED : bad ? ST_BAD : v.nObs == 0 ? ST_NO_OBSERVATION : refQ < 0 ? ST_NO_REF : ST_DONE;
    if (v.stN == ST_DONE) {
        const int level = d.oct[(size_t)ref * s.pitch + refQ];
        if (level >= c.nlevels) v.stN = ST_LEVEL_RANGE;
        else {
            float pc[3];
#pragma unroll
            for (int k = 0; k < 3; k++) pc[k] = v.P[k] - d.ctr[3 * (size_t)ref + k];
            const float dist = (float)cvm::norm3(pc);
            v.maxD = dist * c.sf[level];
            v.minD = v.maxD / c.sf[c.nlevels - 1];
#pragma unroll
            for (int k = 0; k < 3; k++) v.normal[k] = normal[k];
        }
    }
}

__device__ __forceinline__ void write_verdict(uint32_t* r, const Verdict& v)
{
#pragma unroll
    for (int k = 0; k < 3; k++) { r[R_POS + k] = __float_as_uint(v.P[k]); r[R_NORMAL + k] = __float_as_uint(v.normal[k]); }
    r[R_MIN] = __float_as_uint(v.minD); r[R_MAX] = __float_as_uint(v.maxD);
    r[R_NOBS] = (uint32_t)v.nObs; r[R_NDESC] = (uint32_t)v.nDesc; r[R_BESTKF] = (uint32_t)v.bestKf; r[R_BESTIDX] = (uint32_t)v.bestIdx;
    r[R_STATUS] = v.stD | (v.stN << 8);
}

__device__ __forceinline__ void point_position(const Dev& d, const Call& c, int i, int id, float* P)
{
    if (c.newPos) { P[0] = c.newPos[3 * (size_t)i]; P[1] = c.newPos[3 * (size_t)i + 1]; P[2] = c.newPos[3 * (size_t)i + 2]; }
    else { const float4 A = d.pool.a[id]; P[0] = A.x; P[1] = A.y; P[2] = A.z; }
}

// kGroup lanes a point with at most kGroup observations; lane j of a group is observation j once the keys are ranked
__global__ __launch_bounds__(kThreads) void k_refresh_short(orbu::StoreDev s, Dev d, Call c)
{
    __shared__ uint32_t sKey[kGroups][kGroup];
    __shared__ uint32_t sDesc[kGroups][kGroup][8];
    __shared__ float sTerm[kGroups][kGroup][3];
    const int t = threadIdx.x, lane = t & 63, g = t / kGroup, j = t % kGroup, gshift = lane - j;
    const unsigned long long gmask = ((1ull << kGroup) - 1) << gshift;
    const int nShort = min(d.hdr[H_NSHORT], c.n);
    for (int base = blockIdx.x * kGroups; base < nShort; base += gridDim.x * kGroups) {   // (the same turns for the whole workgroup)
        bool live = base + g < nShort;
        int i = live ? d.listShort[base + g] : 0;
        live = live && i >= 0 && i < c.n;
        const int id = live ? c.ids[i] : -1;
        live = live && id >= 0 && id < d.pool.cap;
        int N = live ? d.cnt[i] : 0;
        const int st = live ? d.start[i] : 0;
        if (N < 0 || N > kGroup || st < 0 || (long long)st + N > d.keysCap) N = 0;   // (never: the list holds the short points)
        bool has = j < N;
        uint32_t key = has ? d.keys[st + j] : 0xffffffffu;
        if (has && ((int)(key >> kQBits) >= s.kfcap || (int)(key & ((1u << kQBits) - 1)) >= s.pitch)) { has = false; key = 0xffffffffu; }   // (never: k_walk made the key)
        int rank = 0;
#pragma unroll
        for (int k = 0; k < kGroup; k++) rank += (uint32_t)__shfl((int)key, gshift + k) < key ? 1 : 0;   // (the keys of a point are distinct)
        if (has) {
            sKey[g][rank] = key;
            if (c.what & 1) {
                const uint4* p = (const uint4*)(d.desc + ((size_t)(key >> kQBits) * s.pitch + (key & ((1u << kQBits) - 1))) * 32);
                const uint4 a = p[0], b = p[1];
                uint32_t* o = sDesc[g][rank];
                o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
            }
        }
        __syncthreads();
        // from here lane j is the observation of rank j
        const uint32_t myKey = j < N ? sKey[g][j] : 0u;
        const int mySlot = (int)(myKey >> kQBits), myQ = (int)(myKey & ((1u << kQBits) - 1));
        has = j < N && mySlot < s.kfcap;
        const bool good = has && !(s.flags[mySlot] & 1);   // MapPoint.cc:265 !pKF->isBad()
        const int nDesc = __popcll(__ballot(good) & gmask);
        float P[3] = {0.f, 0.f, 0.f};
        if (live) point_position(d, c, i, id, P);
        // ---- ComputeDistinctiveDescriptors: row i's median by a counting select over [0, 256], the first strictly smallest
        int best = 0x7fffffff, bestI = 0;
        if (c.what & 1) {
            uint32_t md[8];
#pragma unroll
            for (int w = 0; w < 8; w++) md[w] = good ? sDesc[g][j][w] : 0u;
            const int k1 = ((nDesc - 1) >> 1) + 1;   // the element of rank (N - 1) / 2: the smallest v with k1 distances <= v
            for (int r = 0; r < kGroup; r++) {
                if (!__ballot(r < N)) break;   // (the whole wave)
                const bool rowGood = __shfl((int)good, gshift + r) != 0;
                const int dd = hamming8(md, sDesc[g][r]);
                int lo = 0, hiV = 256;
#pragma unroll
                for (int step = 0; step < 9; step++) {
                    const int mid = (lo + hiV) >> 1;
                    const int le = __popcll(__ballot(good && dd <= mid) & gmask);
                    if (lo < hiV) { if (le >= k1) hiV = mid; else lo = mid + 1; }
                }
                if (rowGood && lo < best) { best = lo; bestI = r; }   // :296
            }
        }
        // ---- UpdateNormalAndDepth: the terms in parallel, the sum in order on one lane per component
        float acc = 0.f;
        if (c.what & 2) {
            if (has) normal_term(P, d.ctr + 3 * (size_t)mySlot, sTerm[g][j]);
            __syncthreads();
            if (j < 3 && N > 0) {
                for (int k = 0; k < N; k++) acc = sTerm[g][k][j] + acc;   // :355
                acc = cvm::expr_scale(acc, 1. / N);                       // :369
            }
        }
        float normal[3];
#pragma unroll
        for (int k = 0; k < 3; k++) normal[k] = __shfl(acc, gshift + k);
        const int ref = live ? c.ref[i] : -1;
        const unsigned long long refMask = __ballot(has && ref >= 0 && mySlot == ref) & gmask;
        const int refLane = refMask ? __ffsll((long long)refMask) - 1 : lane;
        const int refQ0 = __shfl(myQ, refLane);
        const int refQ = refMask ? refQ0 : -1;
        Verdict v;
        if (live) {
            v.P[0] = P[0]; v.P[1] = P[1]; v.P[2] = P[2];
            v.nObs = N; v.nDesc = nDesc;
            verdict(s, d, c, id, ref, refQ, normal, (c.what & 1) && nDesc ? sKey[g][bestI] : 0u, v);
            uint32_t* r = d.res + (size_t)i * kRecWords;
            if (j == 0) write_verdict(r, v);
            if (j < 8) r[R_DESC + j] = v.stD == ST_DONE ? sDesc[g][bestI][j] : ((const uint32_t*)d.pool.desc)[8 * (size_t)id + j];
        }
        __syncthreads();   // (the LDS rows are the next turn's)
    }
}

// one workgroup a point with kGroup < N <= kMaxObs observations; descriptors transposed in LDS (word w of observation x at [w][x])
__global__ __launch_bounds__(kThreads) void k_refresh_long(orbu::StoreDev s, Dev d, Call c)
{
    __shared__ uint32_t sRaw[kMaxObs];
    __shared__ uint32_t sKey[kMaxObs];
    __shared__ uint32_t sDesc[8][kMaxObs];
    __shared__ float sTerm[kMaxObs][3];
    __shared__ uint16_t sRow[kWaves][kMaxObs];
    __shared__ uint8_t sGood[kMaxObs];
    __shared__ unsigned long long sBest[kWaves];
    __shared__ int sCnt[kWaves];
    __shared__ int sRef;
    __shared__ float sNormal[3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nLong = min(d.hdr[H_NLONG], c.n);
    for (int w0 = blockIdx.x; w0 < nLong; w0 += gridDim.x) {
        const int i = d.listLong[w0];
        if (i < 0 || i >= c.n) continue;   // (never; the whole workgroup)
        const int id = c.ids[i];
        int N = d.cnt[i];
        const int st = d.start[i];
        if (id < 0 || id >= d.pool.cap || N < 0 || N > kMaxObs || st < 0 || (long long)st + N > d.keysCap) continue;   // (never)
        const int ref = c.ref[i];
        float P[3];
        point_position(d, c, i, id, P);
        for (int x = t; x < N; x += kThreads) sRaw[x] = d.keys[st + x];
        if (t == 0) sRef = 0x7fffffff;
        __syncthreads();
        for (int x = t; x < N; x += kThreads) {
            const uint32_t key = sRaw[x];
            int rank = 0;
            for (int y = 0; y < N; y++) rank += sRaw[y] < key ? 1 : 0;   // (the keys of a point are distinct)
            const int slot = min((int)(key >> kQBits), s.kfcap - 1), q = min((int)(key & ((1u << kQBits) - 1)), s.pitch - 1);   // (k_walk made the key: within both)
            sKey[rank] = key;
            sGood[rank] = (s.flags[slot] & 1) ? 0 : 1;   // MapPoint.cc:265
            if (c.what & 1) {
                const uint4* p = (const uint4*)(d.desc + ((size_t)slot * s.pitch + q) * 32);
                const uint4 a = p[0], b = p[1];
                sDesc[0][rank] = a.x; sDesc[1][rank] = a.y; sDesc[2][rank] = a.z; sDesc[3][rank] = a.w;
                sDesc[4][rank] = b.x; sDesc[5][rank] = b.y; sDesc[6][rank] = b.z; sDesc[7][rank] = b.w;
            }
            if (c.what & 2) normal_term(P, d.ctr + 3 * (size_t)slot, sTerm[rank]);
            if (ref >= 0 && slot == ref) atomicMin(&sRef, rank);
        }
        __syncthreads();
        int cntGood = 0;
        for (int b0 = 0; b0 < N; b0 += kThreads) cntGood += __popcll(__ballot(b0 + t < N && sGood[b0 + t]));
        if (lane == 0) sCnt[wave] = cntGood;
        __syncthreads();
        int nDesc = 0;
        for (int k = 0; k < kWaves; k++) nDesc += sCnt[k];
        // ---- ComputeDistinctiveDescriptors: a wave a row, rows wave, wave + kWaves, ..
        unsigned long long best = ~0ull;   // (median << 32) | row: the minimum is the first strictly smallest median
        if ((c.what & 1) && nDesc) {
            const int k1 = ((nDesc - 1) >> 1) + 1, nch = (N + 63) / 64;
            for (int r = wave; r < N; r += kWaves) {
                if (!sGood[r]) continue;   // (the whole wave)
                for (int ch = 0; ch < nch; ch++) {
                    const int x = ch * 64 + lane;
                    int dd = 0xffff;
                    if (x < N && sGood[x]) {
                        dd = 0;
#pragma unroll
                        for (int w = 0; w < 8; w++) dd += __popc(sDesc[w][x] ^ sDesc[w][r]);
                    }
                    sRow[wave][x] = (uint16_t)dd;   // (read back by this lane alone)
                }
                int lo = 0, hiV = 256;
#pragma unroll 1
                for (int step = 0; step < 9; step++) {
                    const int mid = (lo + hiV) >> 1;
                    int le = 0;
                    for (int ch = 0; ch < nch; ch++) le += __popcll(__ballot((int)sRow[wave][ch * 64 + lane] <= mid));
                    if (lo < hiV) { if (le >= k1) hiV = mid; else lo = mid + 1; }
                }
                const unsigned long long cand = ((unsigned long long)(uint32_t)lo << 32) | (uint32_t)r;
                best = cand < best ? cand : best;
            }
        }
        if (lane == 0) sBest[wave] = best;
        // ---- UpdateNormalAndDepth: the sum in order on one thread per component
        if ((c.what & 2) && t < 3) {
            float acc = 0.f;
            for (int k = 0; k < N; k++) acc = sTerm[k][t] + acc;   // :355
            sNormal[t] = cvm::expr_scale(acc, 1. / N);              // :369
        }
        __syncthreads();
        for (int k = 0; k < kWaves; k++) best = sBest[k] < best ? sBest[k] : best;
        const int bestI = nDesc && (c.what & 1) ? (int)(uint32_t)best : 0;
        uint32_t* r = d.res + (size_t)i * kRecWords;
        Verdict v;
        v.P[0] = P[0]; v.P[1] = P[1]; v.P[2] = P[2];
        v.nObs = N; v.nDesc = nDesc;
        const float normal[3] = {(c.what & 2) ? sNormal[0] : 0.f, (c.what & 2) ? sNormal[1] : 0.f, (c.what & 2) ? sNormal[2] : 0.f};
        const int refRank = sRef;
        verdict(s, d, c, id, ref, refRank < N ? (int)(sKey[refRank] & ((1u << kQBits) - 1)) : -1, normal, sKey[bestI], v);
        if (t == 0) write_verdict(r, v);
        if (t < 8) r[R_DESC + t] = v.stD == ST_DONE ? sDesc[t][bestI] : ((const uint32_t*)d.pool.desc)[8 * (size_t)id + t];
        __syncthreads();   // (the LDS arrays are the next point's)
    }
}

// a half that is not DONE left the pool's own values in the record and is not written; with new positions the position of every
// listed id is (SetWorldPos has no gate); the flags word is never touched
__global__ __launch_bounds__(kThreads) void k_commit(Dev d, Call c)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= c.n) return;
    const int id = c.ids[i];
    if (id < 0 || id >= d.pool.cap) return;
    const uint32_t* r = d.res + (size_t)i * kRecWords;
    const uint32_t st = r[R_STATUS];
    if (c.newPos || ((st >> 8) & 0xff) == ST_DONE) {
        d.pool.a[id] = make_float4(__uint_as_float(r[R_POS]), __uint_as_float(r[R_POS + 1]), __uint_as_float(r[R_POS + 2]), __uint_as_float(r[R_MIN]));
        d.pool.b[id] = make_float4(__uint_as_float(r[R_NORMAL]), __uint_as_float(r[R_NORMAL + 1]), __uint_as_float(r[R_NORMAL + 2]), __uint_as_float(r[R_MAX]));
    }
    if ((st & 0xff) == ST_DONE) {
        d.pool.desc[2 * (size_t)id] = make_uint4(r[R_DESC], r[R_DESC + 1], r[R_DESC + 2], r[R_DESC + 3]);
        d.pool.desc[2 * (size_t)id + 1] = make_uint4(r[R_DESC + 4], r[R_DESC + 5], r[R_DESC + 6], r[R_DESC + 7]);
    }
}

}  // namespace orbr
