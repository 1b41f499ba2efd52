// orbk_kernels.hip -- the keyframe database's queries on gfx950.
//
// Reference: SingleRobotScenario/src/KeyFrameDatabase.cc (identical in the multi-robot tree)
//   DetectRelocalizationCandidates :211-303, DetectLoopCandidates :97-209
// and DBoW2's L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp).
//
// No inverted file lives on the device.  A database keeps, per member keyframe (pool slot), how many live copies it holds
// and the insertion sequence of the earliest one; the lists of the reference hold every copy of a keyframe under every
// word of its BowVector in insertion order and erase() removes the first occurrence per word, so the walk of
// lKFsSharingWords meets a keyframe first at (its smallest word shared with the query, its earliest live copy), and it
// meets it copies * shared-words times in all.  One wave per member walks the member's own BowVector against a dense
// word table of the query: shared-word count, first-encounter key, the state update, and later the score.
//
// Per query (one stream, no host step in between for the batch):
//   k_kf_prepare   query words -> dense table (epoch-tagged), connected slots -> marks, counters cleared
//   k_kf_count     wave per member: hits, state update / push decision, max of the pushed word counts
//   k_kf_score     wave per pushed member above minCommonWords: exact L1 score, the ordered double sum wave-uniform
//   k_kf_rank      the scored list in first-encounter order (rank of each key among the scored)
//   k_kf_acc       covisibility accumulation per scored entry
//   k_kf_finalize  one workgroup: bestAccScore, 0.75f threshold, pBestKF dedup on first occurrence, ordered compaction
// Integer and fp64 add/sub only; every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbk {

constexpr int kNeigh = 10;             // GetBestCovisibilityKeyFrames(10)
constexpr int kFinThreads = 1024;
constexpr uint64_t kNoKey = ~0ull;

struct PoolDev {
    const int32_t* bowOff;   // [slots] first entry of the slot's BowVector in the arena
    const int32_t* bowLen;   // [slots]
    const uint32_t* ids;     // arena: word ids ascending per slot
    const double* vals;      // arena: word values
    uint64_t* relocQ; int32_t* relocW; float* relocS;   // mnRelocQuery, mnRelocWords, mRelocScore
    uint64_t* loopQ; int32_t* loopW; float* loopS;      // mnLoopQuery, mnLoopWords, mLoopScore
    const int32_t* cov; const int32_t* covN;            // [slots][kNeigh], [slots]: GetBestCovisibilityKeyFrames(10)
    int32_t* connMark;       // [slots] epoch of the loop query whose connected set holds the slot
    int32_t* firstIdx;       // [slots] INT_MAX at rest: the finalize's dedup
    int32_t* wEpoch;         // [words] epoch of the query that holds the word
    int32_t* wIdx;           // [words] the word's index in that query's BowVector
};

struct Member { int32_t slot, copies; uint32_t seq; int32_t pad; };

struct Counters {
    int32_t maxWords;   // maxCommonWords over the pushed keyframes
    int32_t nSel;       // entries of lScoreAndMatch
    int32_t nOut;       // candidates
    float minScore;     // loop: the query's minScore
};

// One query of a sequence.  The query's BowVector is either a pool slot (qSlot) or a buffer whose length is read on the
// device (qIds / qVals / qLen: a frame-set slot copied device to device).
struct Query {
    const int32_t* qSlot; const uint32_t* qIds; const double* qVals; const int32_t* qLen;
    const uint64_t* qid;                 // [q]
    const int32_t* connStart; const int32_t* connIdx;   // CSR [q] (loop)
    Counters* cnt;                       // [q]
    int32_t q, loop, epoch;
};

struct QView { const uint32_t* ids; const double* vals; int n; };
__device__ __forceinline__ QView query_view(const PoolDev& p, const Query& Q)
{
    if (Q.qSlot) { const int s = Q.qSlot[Q.q]; return {p.ids + p.bowOff[s], p.vals + p.bowOff[s], p.bowLen[s]}; }
    return {Q.qIds, Q.qVals, *Q.qLen};
}

// DBoW2 L1Scoring::score's term for a word both vectors hold (v1 = vi, v2 = wi), in its evaluation order
__device__ __forceinline__ double l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }

// adds the terms of the hit lanes (ballot b) to s in lane order -- the words ascend with the lanes, so this is the
// reference's sequential sum in word order; wave-uniform (v_readlane), every lane holds the same s
__device__ __forceinline__ double add_terms_in_order(double s, double t, uint64_t b)
{
    const long long tb = __double_as_longlong(t);
    const int lo = (int)(tb & 0xFFFFFFFFll), hi = (int)(tb >> 32);
    while (b) {
        const int l = __ffsll((long long)b) - 1;
        b &= b - 1;
        const long long v = ((long long)(uint32_t)__builtin_amdgcn_readlane(lo, l)) | ((long long)__builtin_amdgcn_readlane(hi, l) << 32);
        s += __longlong_as_double(v);
    }
    return s;
}

// ORBVocabulary::score(v1 = a, v2 = b) by a wave: every word of b is looked up in a (binary search), common words in
// ascending id; -score/2.0 as the reference writes it (an empty intersection gives -0.0)
__device__ double l1_score_wave(const uint32_t* __restrict__ aIds, const double* __restrict__ aVals, int na,
                                const uint32_t* __restrict__ bIds, const double* __restrict__ bVals, int nb)
{
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const int j = j0 + lane;
        bool hit = false;
        double t = 0.0;
        if (j < nb && na > 0) {
            const uint32_t w = bIds[j];
            int lo = 0, hi = na;   // first a >= w
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (aIds[mid] < w) lo = mid + 1; else hi = mid; }
            if (lo < na && aIds[lo] == w) { hit = true; t = l1_term(aVals[lo], bVals[j]); }
        }
        const uint64_t b = __ballot(hit);
        if (b) s = add_terms_in_order(s, t, b);
    }
    return -s / 2.0;
}

// score(slot aSlot[i], slot bSlot[i]) narrowed to float, one wave per pair
__global__ __launch_bounds__(256) void k_kf_score_pairs(PoolDev p, const int32_t* __restrict__ aSlot, const int32_t* __restrict__ bSlot, int n,
                                                        float* __restrict__ outF)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int a = aSlot[i], b = bSlot[i];
    const double s = l1_score_wave(p.ids + p.bowOff[a], p.vals + p.bowOff[a], p.bowLen[a], p.ids + p.bowOff[b], p.vals + p.bowOff[b], p.bowLen[b]);
    if ((threadIdx.x & 63) == 0) outF[i] = (float)s;
}

__global__ __launch_bounds__(64) void k_kf_score_one(const uint32_t* __restrict__ aIds, const double* __restrict__ aVals, int na,
                                                     const uint32_t* __restrict__ bIds, const double* __restrict__ bVals, int nb, double* __restrict__ out)
{
    const double s = l1_score_wave(aIds, aVals, na, bIds, bVals, nb);
    if (threadIdx.x == 0) out[0] = s;
}

// LoopClosing / MultiMapper's minScore: 1, then every covisible keyframe's score if lower, in list order; one thread per query
__global__ __launch_bounds__(256) void k_kf_min_score(const float* __restrict__ pairScore, const int32_t* __restrict__ covStart, int n, Counters* __restrict__ cnt)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    float m = 1.f;
    for (int i = covStart[q]; i < covStart[q + 1]; i++) if (pairScore[i] < m) m = pairScore[i];
    cnt[q].minScore = m;
}

// the copy of a frame set slot's BowVector (count on the device) into a buffer: the query buffer or a pool arena range
__global__ __launch_bounds__(256) void k_kf_copy_bow(const uint32_t* __restrict__ srcIds, const double* __restrict__ srcVals, const int32_t* __restrict__ srcCount,
                                                     int cap, uint32_t* __restrict__ dstIds, double* __restrict__ dstVals, int32_t* __restrict__ dstLen)
{
    const int n = min(*srcCount, cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { dstIds[i] = srcIds[i]; dstVals[i] = srcVals[i]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) *dstLen = n;
}

__global__ __launch_bounds__(256) void k_kf_prepare(PoolDev p, Query Q)
{
    const QView v = query_view(p, Q);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    for (int i = tid; i < v.n; i += nt) { const uint32_t w = v.ids[i]; p.wEpoch[w] = Q.epoch; p.wIdx[w] = i; }
    if (Q.loop && Q.connStart)
        for (int i = Q.connStart[Q.q] + tid; i < Q.connStart[Q.q + 1]; i += nt) p.connMark[Q.connIdx[i]] = Q.epoch;
    if (tid == 0) { Counters* c = Q.cnt + Q.q; c->maxWords = 0; c->nSel = 0; c->nOut = 0; }
}

// one wave per database member: how often the walk meets it (copies x shared words), where it meets it first, and what
// the reference does to its state on those hits (:107-121 / :218-231)
__global__ __launch_bounds__(256) void k_kf_count(PoolDev p, Query Q, const Member* __restrict__ mem, int m, uint64_t* __restrict__ key)
{
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= m) return;
    const int lane = threadIdx.x & 63;
    const Member M = mem[w];
    const int s = M.slot, off = p.bowOff[s], len = p.bowLen[s];
    int shared = 0;
    uint32_t minWord = 0;
    bool any = false;
    for (int j0 = 0; j0 < len; j0 += 64) {
        const int j = j0 + lane;
        uint32_t id = 0;
        bool hit = false;
        if (j < len) { id = p.ids[off + j]; hit = p.wEpoch[id] == Q.epoch; }
        const uint64_t b = __ballot(hit);
        if (b && !any) { any = true; minWord = (uint32_t)__builtin_amdgcn_readlane((int)id, __ffsll((long long)b) - 1); }
        shared += __popcll(b);
    }
    if (lane != 0) return;
    uint64_t k = kNoKey;
    if (shared > 0) {
        const int c = shared * M.copies;
        const uint64_t qid = Q.qid[Q.q];
        if (!Q.loop) {
            if (p.relocQ[s] != qid) { p.relocW[s] = c; p.relocQ[s] = qid; k = ((uint64_t)minWord << 32) | M.seq; }
            else p.relocW[s] += c;
        } else {
            if (p.loopQ[s] != qid) {
                if (p.connMark[s] == Q.epoch) p.loopW[s] = 1;   // reset on every hit, then one increment
                else { p.loopW[s] = c; p.loopQ[s] = qid; k = ((uint64_t)minWord << 32) | M.seq; }
            } else p.loopW[s] += c;
        }
        if (k != kNoKey) atomicMax(&Q.cnt[Q.q].maxWords, c);
    }
    key[w] = k;
}

__device__ __forceinline__ int min_common_words(int maxWords) { return (int)((float)maxWords * 0.8f); }

// one wave per pushed member with more than minCommonWords: si = (float)score(query, member), the member's score field,
// and (loop) si >= minScore puts it on the scored list; list order comes from k_kf_rank
__global__ __launch_bounds__(256) void k_kf_score(PoolDev p, Query Q, const Member* __restrict__ mem, int m, const uint64_t* __restrict__ key,
                                                  uint64_t* __restrict__ selKey, int32_t* __restrict__ selSlot, float* __restrict__ selScore)
{
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= m) return;
    const uint64_t k = key[w];
    if (k == kNoKey) return;
    const int s = mem[w].slot;
    Counters* c = Q.cnt + Q.q;
    const int minCommon = min_common_words(c->maxWords);
    if ((Q.loop ? p.loopW[s] : p.relocW[s]) <= minCommon) return;
    const QView v = query_view(p, Q);
    const int lane = threadIdx.x & 63, off = p.bowOff[s], len = p.bowLen[s];
    double sum = 0.0;
    for (int j0 = 0; j0 < len; j0 += 64) {
        const int j = j0 + lane;
        bool hit = false;
        double t = 0.0;
        if (j < len) {
            const uint32_t id = p.ids[off + j];
            if (p.wEpoch[id] == Q.epoch) { hit = true; t = l1_term(v.vals[p.wIdx[id]], p.vals[off + j]); }
        }
        const uint64_t b = __ballot(hit);
        if (b) sum = add_terms_in_order(sum, t, b);
    }
    if (lane != 0) return;
    const float si = (float)(-sum / 2.0);
    if (Q.loop) p.loopS[s] = si; else p.relocS[s] = si;
    if (Q.loop && !(si >= c->minScore)) return;
    const int i = atomicAdd(&c->nSel, 1);
    selKey[i] = k; selSlot[i] = s; selScore[i] = si;
}

// lScoreAndMatch in first-encounter order: each entry's rank among the keys (all distinct: one entry per slot)
__global__ __launch_bounds__(256) void k_kf_rank(Query Q, const uint64_t* __restrict__ selKey, const int32_t* __restrict__ selSlot,
                                                 const float* __restrict__ selScore, int32_t* __restrict__ ordSlot, float* __restrict__ ordScore)
{
    __shared__ uint64_t tile[256];
    const int n = Q.cnt[Q.q].nSel;
    if ((int)(blockIdx.x * 256) >= n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t ki = i < n ? selKey[i] : kNoKey;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
        __syncthreads();
        if (t0 + (int)threadIdx.x < n) tile[threadIdx.x] = selKey[t0 + threadIdx.x];
        __syncthreads();
        const int tn = min(256, n - t0);
        for (int t = 0; t < tn; t++) rank += tile[t] < ki;
    }
    if (i < n) { ordSlot[rank] = selSlot[i]; ordScore[rank] = selScore[i]; }
}

// "accumulate score by covisibility" (:151-173 / :254-279) for entry e of the ordered list; the neighbours come from the
// pool's table (nbStart == nullptr) or from a CSR over the entries the caller filled at this point
__global__ __launch_bounds__(256) void k_kf_acc(PoolDev p, Query Q, const int32_t* __restrict__ ordSlot, const float* __restrict__ ordScore,
                                                const int32_t* __restrict__ nbStart, const int32_t* __restrict__ nbIdx,
                                                float* __restrict__ accOut, int32_t* __restrict__ bestOut)
{
    const Counters* c = Q.cnt + Q.q;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c->nSel) return;
    const uint64_t qid = Q.qid[Q.q];
    const int minCommon = min_common_words(c->maxWords);
    const int s = ordSlot[e];
    float best = ordScore[e], acc = best;
    int pBest = s;
    const int* nb = nbStart ? nbIdx + nbStart[e] : p.cov + (size_t)s * kNeigh;
    const int nn = nbStart ? nbStart[e + 1] - nbStart[e] : p.covN[s];
    for (int i = 0; i < nn; i++) {
        const int k2 = nb[i];
        float sc;
        if (Q.loop) {
            if (!(p.loopQ[k2] == qid && p.loopW[k2] > minCommon)) continue;
            sc = p.loopS[k2];
        } else {
            if (p.relocQ[k2] != qid) continue;
            sc = p.relocS[k2];
        }
        acc += sc;
        if (sc > best) { pBest = k2; best = sc; }
    }
    accOut[e] = acc;
    bestOut[e] = pBest;
}

// block-wide exclusive scan of one int per thread (kFinThreads threads), returns the total in *tot
__device__ int block_excl_scan(int v, int* sh, int* tot)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kFinThreads; d <<= 1) {
        const int x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const int incl = sh[t];
    *tot = sh[kFinThreads - 1];
    __syncthreads();
    return incl - v;
}

// bestAccScore, minScoreToRetain = 0.75f*bestAccScore, and the candidates: pBestKF of every entry above it, first
// occurrence only, in list order (:176-206 / :281-300).  The candidates of query q start at *outTotal (the queries of a
// batch append behind each other); what does not fit cap is counted, not written.
__global__ __launch_bounds__(kFinThreads) void k_kf_finalize(Query Q, const float* __restrict__ acc, const int32_t* __restrict__ best, int32_t* firstIdx,
                                                            int32_t* __restrict__ out, int cap, int32_t* __restrict__ outTotal, int32_t* __restrict__ outStart)
{
    __shared__ float shf[kFinThreads];
    __shared__ int shi[kFinThreads];
    Counters* c = Q.cnt + Q.q;
    const int n = c->nSel, t = threadIdx.x;
    const int base = *outTotal;
    float m = Q.loop ? c->minScore : 0.f;
    for (int e = t; e < n; e += kFinThreads) m = fmaxf(m, acc[e]);
    shf[t] = m;
    __syncthreads();
    for (int d = kFinThreads / 2; d > 0; d >>= 1) { if (t < d) shf[t] = fmaxf(shf[t], shf[t + d]); __syncthreads(); }
    const float thr = 0.75f * shf[0];
    for (int e = t; e < n; e += kFinThreads) if (acc[e] > thr) atomicMin(&firstIdx[best[e]], e);
    __syncthreads();
    __threadfence_block();
    int written = 0;
    for (int e0 = 0; e0 < n; e0 += kFinThreads) {
        const int e = e0 + t;
        const int kept = e < n && acc[e] > thr && __hip_atomic_load(&firstIdx[best[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e;
        int tot;
        const int pos = block_excl_scan(kept, shi, &tot);
        if (kept && base + written + pos < cap) out[base + written + pos] = best[e];
        written += tot;
    }
    __syncthreads();
    for (int e = t; e < n; e += kFinThreads) if (acc[e] > thr) firstIdx[best[e]] = 0x7FFFFFFF;
    if (t == 0) {
        c->nOut = written;
        if (outStart) { outStart[Q.q] = base; outStart[Q.q + 1] = base + written; }
        *outTotal = base + written;
    }
}

}  // namespace orbk
