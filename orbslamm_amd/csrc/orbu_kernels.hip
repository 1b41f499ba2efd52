// orbu_kernels.hip -- the device side of Tracking::UpdateLocalMap (part of orbslamm_hip.hip; ABI: include/orbslamm_localmap.h,
// DESIGN.md §8r; host side: orbu_host.inc).  Integers only.
//   k_kf_scatter      a setter's staged keyframe records (header, children, entries) into the store's arrays
//   k_pair_scatter    single match slots of one keyframe, or flag bytes
//   k_stamp           the frame's pool ids -> a count per point under this call's generation tag
//   k_vote            one wave per set keyframe: the sum of its voting entries' counts (Tracking.cc:1293-1309)
//   k_select          one workgroup: the voted keyframes in ascending slot, kf_max, and in ONE wave the expansion (:1311-1397)
//   k_points_mark     first sighting of every point of the local keyframes: a 64-bit atomic min of (tag, position)
//   k_points_count / k_points_scan / k_points_write   the ordered compaction of the first sightings into L, seen and S
// The pool-sized scratch is never cleared per call.  stamp[id] = (tag << 32) | count: a max with (tag << 32) brings a stale
// word to this call's zero and leaves a live one alone, then the add counts; both are integer atomics whose result does not
// depend on order.  first[id] = (~tag << 32) | position: a later call's tag gives a smaller word than any stale one, so the
// min needs no clear either.  The host clears both once when the tag wraps.
// The compaction works in chunks of kChunk positions (list position * pitch + entry index; the pitch is the stride rounded
// up to 4, so a thread's 16-byte read stays within one row); a fixed grid walks the chunks, whose number only the device knows.
#pragma once

namespace orbu {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = kThreads * 4;
constexpr int kNoVote = 1 << 30;
constexpr int kGraphInts = 12;     // neigh[10], parent, nchildren
constexpr int kRecHead = 16;       // a staged record's header: slot, flags, the graph record, two pads
constexpr int kMaxKeyFrames = 1 << 17;
enum { H_STATUS = 0, H_KFMAX, H_NKF, H_NL, H_NS, H_INTS = 16 };

struct StoreDev {
    int32_t* entries;    // [kfcap * pitch]
    uint8_t* flags;      // [kfcap]
    int32_t* graph;      // [kfcap * kGraphInts]
    int32_t* children;   // [kfcap * maxc]
    int32_t kfcap, pitch, maxc;
};
struct Scratch {
    unsigned long long* stamp;   // [poolCap]
    unsigned long long* first;   // [poolCap]
    const uint32_t* poolFlags;
    int32_t poolCap;
    uint32_t gen;
};
// what a call writes: the device copies the kernels read, and the pinned copies the host reads after the stream's end
struct Out {
    int32_t* hdr; int32_t* list; int32_t* votes; uint2* chunk;
    int32_t* L; int32_t* S;
    int32_t* hHdr; int32_t* hList; int32_t* hVotes; int32_t* hL; uint8_t* hSeen;
    int32_t maxL;
};

// staged: nrec records of recInts ints: header | maxcP children | (mode 0) pitch entries.  mode 0 writes everything, mode 1
// the graph record and the children.  Slots are distinct within a launch and inside the store (checked on the host).
__global__ __launch_bounds__(kThreads) void k_kf_scatter(StoreDev s, const int32_t* __restrict__ staged, int recInts, int maxcP, int mode)
{
    const int32_t* rec = staged + (size_t)blockIdx.x * recInts;
    const int k = rec[0];
    if (k < 0 || k >= s.kfcap) return;
    const int t = threadIdx.x;
    if (t < kGraphInts) s.graph[(size_t)k * kGraphInts + t] = rec[2 + t];
    if (t == 0 && mode == 0) s.flags[k] = (uint8_t)rec[1];
    for (int c = t; c < s.maxc; c += kThreads) s.children[(size_t)k * s.maxc + c] = rec[kRecHead + c];
    if (mode == 0) {
        const int4* src = (const int4*)(rec + kRecHead + maxcP);
        int4* dst = (int4*)(s.entries + (size_t)k * s.pitch);
        for (int e = t; e < s.pitch / 4; e += kThreads) dst[e] = src[e];
    }
}

// mode 0: {idx, val} pairs -> entries of keyframe `slot`.  mode 1: {slot, flags} pairs -> the flags
__global__ __launch_bounds__(kThreads) void k_pair_scatter(StoreDev s, const int2* __restrict__ staged, int n, int slot, int mode)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int2 p = staged[i];
    if (mode == 0) {
        if (p.x >= 0 && p.x < s.pitch && slot >= 0 && slot < s.kfcap) s.entries[(size_t)slot * s.pitch + p.x] = p.y;
    } else if (p.x >= 0 && p.x < s.kfcap)
        s.flags[p.x] = (uint8_t)p.y;
}

__device__ __forceinline__ bool point_live(const Scratch& c, int id) { return id >= 0 && id < c.poolCap && !(c.poolFlags[id] & 1); }
__device__ __forceinline__ uint32_t stamped_count(const Scratch& c, int id)
{
    const unsigned long long w = c.stamp[id];
    return (uint32_t)(w >> 32) == c.gen ? (uint32_t)w : 0u;
}

// ids[n]: the frame's pool ids or -1 (pinned host memory).  givenList (orbu_local_points): the caller's keyframe list, copied
// to where k_select would have left it, with the header
__global__ __launch_bounds__(kThreads) void k_stamp(Scratch c, const int32_t* __restrict__ ids, int n, const int32_t* __restrict__ givenList, int nGiven, Out o)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        const int id = ids[i];
        if (point_live(c, id)) {
            atomicMax(&c.stamp[id], (unsigned long long)c.gen << 32);
            atomicAdd(&c.stamp[id], 1ull);
        }
    }
    if (givenList) {
        if (i < nGiven) { const int k = givenList[i]; o.list[i] = k; o.hList[i] = k; }
        if (i == 0) {
            o.hdr[H_STATUS] = 0; o.hdr[H_KFMAX] = -1; o.hdr[H_NKF] = nGiven;
            o.hHdr[H_STATUS] = 0; o.hHdr[H_KFMAX] = -1; o.hHdr[H_NKF] = nGiven;
        }
    }
}

// one wave per keyframe slot below hi (the highest set slot + 1): 16-byte reads of the entry row, a gather of the counts
__global__ __launch_bounds__(kThreads) void k_vote(StoreDev s, Scratch c, int hi, Out o)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (k >= hi) return;
    uint32_t sum = 0;
    if (s.flags[k] & 2) {
        const int4* row = (const int4*)(s.entries + (size_t)k * s.pitch);
        for (int e = lane; e < s.pitch / 4; e += 64) {
            const int4 v = row[e];
            const int id[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (id[j] >= 0 && !(id[j] & kNoVote) && id[j] < c.poolCap) sum += stamped_count(c, id[j]);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += (uint32_t)__shfl_down((int)sum, d);
    if (lane == 0) { o.votes[k] = (int32_t)sum; o.hVotes[k] = (int32_t)sum; }
}

// Tracking.cc:1311-1397.  All kThreads threads build the voted group; wave 0 runs the expansion, the `included` marks
// (mnTrackReferenceForFrame == mCurrentFrame.mnId) as a bitmap in LDS.
__global__ __launch_bounds__(kThreads) void k_select(StoreDev s, int hi, int maxKf, Out o)
{
    __shared__ uint32_t inc[kMaxKeyFrames / 32];
    __shared__ int waveCnt[kWaves];
    __shared__ unsigned long long waveBest[kWaves];
    __shared__ int anyVote;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int w = t; w < (s.kfcap + 31) / 32; w += kThreads) inc[w] = 0;
    if (t == 0) anyVote = 0;
    __syncthreads();
    // :1321-1336 in ascending slot: the voted keyframes that are not bad join the list; the first with strictly the most votes
    int G = 0;
    bool any = false;
    unsigned long long best = 0;   // (votes << 32) | ~slot: the maximum is the most votes, then the lowest slot
    for (int base = 0; base < hi; base += kThreads) {
        const int k = base + t;
        const int v = k < hi ? o.votes[k] : 0;
        any |= v > 0;
        const bool take = v > 0 && !(s.flags[k] & 1);
        const unsigned long long m = __ballot(take);
        if (lane == 0) waveCnt[wave] = __popcll(m);
        __syncthreads();
        int off = G, tot = 0;
        for (int w = 0; w < kWaves; w++) { if (w < wave) off += waveCnt[w]; tot += waveCnt[w]; }
        if (take) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1));
            o.list[pos] = k; o.hList[pos] = k;
            atomicOr(&inc[k >> 5], 1u << (k & 31));
            const unsigned long long key = ((unsigned long long)(uint32_t)v << 32) | (uint32_t)~(uint32_t)k;
            best = key > best ? key : best;
        }
        G += tot;
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_down((long long)best, d);
        best = other > best ? other : best;
    }
    if (lane == 0) waveBest[wave] = best;
    if (any) anyVote = 1;   // (every writer stores the same value)
    __threadfence_block();
    __syncthreads();
    if (wave != 0) return;
    if (!anyVote) {   // :1311 keyframeCounter.empty(): the old lists stay
        if (lane == 0) {
            o.hdr[H_STATUS] = 1; o.hdr[H_KFMAX] = -1; o.hdr[H_NKF] = 0;
            o.hHdr[H_STATUS] = 1; o.hHdr[H_KFMAX] = -1; o.hHdr[H_NKF] = 0;
        }
        return;
    }
    for (int w = 1; w < kWaves; w++) best = waveBest[w] > best ? waveBest[w] : best;
    best = waveBest[0] > best ? waveBest[0] : best;
    const int kfMax = G > 0 ? (int)~(uint32_t)best : -1;
    volatile uint32_t* vinc = inc;
    int size = G;
    for (int i = 0; i < G; i++) {   // :1340: the end iterator is taken before the loop
        if (size > maxKf) break;   // :1343
        const int k = o.list[i];
        {   // :1348-1362 the first neighbour that is neither bad nor included
            const int nb = lane < 10 ? s.graph[(size_t)k * kGraphInts + lane] : -1;
            const bool ok = nb >= 0 && nb < s.kfcap && !(s.flags[nb] & 1) && !((vinc[nb >> 5] >> (nb & 31)) & 1);
            const unsigned long long m = __ballot(ok);
            if (m) {
                const int pick = __shfl(nb, __ffsll((long long)m) - 1);
                if (lane == 0) { o.list[size] = pick; o.hList[size] = pick; vinc[pick >> 5] |= 1u << (pick & 31); }
                size++;
            }
        }
        __builtin_amdgcn_wave_barrier();
        {   // :1364-1377 the first such child
            const int nc = min(max(s.graph[(size_t)k * kGraphInts + 11], 0), s.maxc);
            for (int c0 = 0; c0 < nc; c0 += 64) {
                const int ch = c0 + lane < nc ? s.children[(size_t)k * s.maxc + c0 + lane] : -1;
                const bool ok = ch >= 0 && ch < s.kfcap && !(s.flags[ch] & 1) && !((vinc[ch >> 5] >> (ch & 31)) & 1);
                const unsigned long long m = __ballot(ok);
                if (m) {
                    const int pick = __shfl(ch, __ffsll((long long)m) - 1);
                    if (lane == 0) { o.list[size] = pick; o.hList[size] = pick; vinc[pick >> 5] |= 1u << (pick & 31); }
                    size++;
                    break;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // :1379-1388 the parent, not tested for bad; the break at :1386 leaves the OUTER loop
        const int par = s.graph[(size_t)k * kGraphInts + 10];
        if (par >= 0 && par < s.kfcap && !((vinc[par >> 5] >> (par & 31)) & 1)) {
            if (lane == 0) { o.list[size] = par; o.hList[size] = par; }
            size++;
            break;
        }
    }
    if (lane == 0) {
        o.hdr[H_STATUS] = 0; o.hdr[H_KFMAX] = kfMax; o.hdr[H_NKF] = size;
        o.hHdr[H_STATUS] = 0; o.hHdr[H_KFMAX] = kfMax; o.hHdr[H_NKF] = size;
    }
}

// a thread's four entries at positions pos .. pos + 3 of the walk over the local keyframes (-1 behind the walk's end)
__device__ __forceinline__ int4 walk_entries(const StoreDev& s, const int32_t* list, long long total, int pos)
{
    if (pos >= total) return make_int4(-1, -1, -1, -1);
    const int j = pos / s.pitch, e = pos - j * s.pitch;
    const int k = list[j];
    if (k < 0 || k >= s.kfcap) return make_int4(-1, -1, -1, -1);
    return *(const int4*)(s.entries + (size_t)k * s.pitch + e);
}
__device__ __forceinline__ unsigned long long first_key(const Scratch& c, int pos) { return ((unsigned long long)~c.gen << 32) | (uint32_t)pos; }

// :1272-1283, the part that does not depend on order: per point that is not bad, the smallest position at which it is met
__global__ __launch_bounds__(kThreads) void k_points_mark(StoreDev s, Scratch c, Out o)
{
    const long long total = (long long)o.hdr[H_NKF] * s.pitch;
    for (long long c0 = (long long)blockIdx.x * kChunk; c0 < total; c0 += (long long)gridDim.x * kChunk) {
        const int pos = (int)c0 + threadIdx.x * 4;
        const int4 v = walk_entries(s, o.list, total, pos);
        const int raw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int id = raw[j] & ~kNoVote;
            if (raw[j] >= 0 && point_live(c, id)) atomicMin(&c.first[id], first_key(c, pos + j));
        }
    }
}

// the four flags of a thread: bit j = position pos + j is its point's first sighting, bit 4 + j = and the point is not stamped
__device__ __forceinline__ uint32_t first_flags(const StoreDev& s, const Scratch& c, const int32_t* list, long long total, int pos, int* ids)
{
    const int4 v = walk_entries(s, list, total, pos);
    const int raw[4] = {v.x, v.y, v.z, v.w};
    uint32_t f = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int id = raw[j] & ~kNoVote;
        ids[j] = id;
        if (raw[j] >= 0 && point_live(c, id) && c.first[id] == first_key(c, pos + j)) f |= (stamped_count(c, id) ? 1u : 0x11u) << j;
    }
    return f;
}

__global__ __launch_bounds__(kThreads) void k_points_count(StoreDev s, Scratch c, Out o)
{
    __shared__ int cnt[2];
    const long long total = (long long)o.hdr[H_NKF] * s.pitch;
    for (long long c0 = (long long)blockIdx.x * kChunk; c0 < total; c0 += (long long)gridDim.x * kChunk) {
        if (threadIdx.x == 0) { cnt[0] = 0; cnt[1] = 0; }
        __syncthreads();
        int ids[4];
        const uint32_t f = first_flags(s, c, o.list, total, (int)c0 + threadIdx.x * 4, ids);
        int nl = __popc(f & 15u), ns = __popc(f >> 4);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { nl += __shfl_down(nl, d); ns += __shfl_down(ns, d); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&cnt[0], nl); atomicAdd(&cnt[1], ns); }
        __syncthreads();
        if (threadIdx.x == 0) o.chunk[c0 / kChunk] = make_uint2((uint32_t)cnt[0], (uint32_t)cnt[1]);
        __syncthreads();
    }
}

// one workgroup: the chunks' counts -> their exclusive offsets, in place; the totals into the header
__global__ __launch_bounds__(kThreads) void k_points_scan(StoreDev s, Out o)
{
    __shared__ uint2 waveTot[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long total = (long long)o.hdr[H_NKF] * s.pitch;
    const int nchunks = (int)((total + kChunk - 1) / kChunk);
    uint2 run = make_uint2(0, 0);
    for (int base = 0; base < nchunks; base += kThreads) {
        const int i = base + t;
        const uint2 v = i < nchunks ? o.chunk[i] : make_uint2(0, 0);
        uint2 inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t a = (uint32_t)__shfl_up((int)inc.x, d), b = (uint32_t)__shfl_up((int)inc.y, d);
            if (lane >= d) { inc.x += a; inc.y += b; }
        }
        if (lane == 63) waveTot[wave] = inc;
        __syncthreads();
        uint2 off = run, tot = make_uint2(0, 0);
        for (int w = 0; w < kWaves; w++) {
            if (w < wave) { off.x += waveTot[w].x; off.y += waveTot[w].y; }
            tot.x += waveTot[w].x; tot.y += waveTot[w].y;
        }
        if (i < nchunks) o.chunk[i] = make_uint2(off.x + inc.x - v.x, off.y + inc.y - v.y);
        run.x += tot.x; run.y += tot.y;
        __syncthreads();
    }
    if (t == 0) {
        o.hdr[H_NL] = (int32_t)run.x; o.hdr[H_NS] = (int32_t)run.y;
        o.hHdr[H_NL] = (int32_t)run.x; o.hHdr[H_NS] = (int32_t)run.y;
    }
}

// L, seen and S in walk order.  More than maxL: nothing is written (the host reports the count)
__global__ __launch_bounds__(kThreads) void k_points_write(StoreDev s, Scratch c, Out o)
{
    __shared__ uint2 waveTot[kWaves];
    if (o.hdr[H_NL] > o.maxL) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long total = (long long)o.hdr[H_NKF] * s.pitch;
    for (long long c0 = (long long)blockIdx.x * kChunk; c0 < total; c0 += (long long)gridDim.x * kChunk) {
        int ids[4];
        const uint32_t f = first_flags(s, c, o.list, total, (int)c0 + t * 4, ids);
        const uint32_t nl = __popc(f & 15u), ns = __popc(f >> 4);
        uint2 inc = make_uint2(nl, ns);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t a = (uint32_t)__shfl_up((int)inc.x, d), b = (uint32_t)__shfl_up((int)inc.y, d);
            if (lane >= d) { inc.x += a; inc.y += b; }
        }
        if (lane == 63) waveTot[wave] = inc;
        __syncthreads();
        const uint2 base = o.chunk[c0 / kChunk];
        uint32_t l = base.x + inc.x - nl, q = base.y + inc.y - ns;
        for (int w = 0; w < wave; w++) { l += waveTot[w].x; q += waveTot[w].y; }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if ((f >> j) & 1) {
                const bool unseen = (f >> (4 + j)) & 1;
                if (l < (uint32_t)o.maxL) { o.L[l] = ids[j]; o.hL[l] = ids[j]; o.hSeen[l] = unseen ? 0 : 1; }
                l++;
                if (unseen) { if (q < (uint32_t)o.maxL) o.S[q] = ids[j]; q++; }
            }
        __syncthreads();
    }
}

}  // namespace orbu
