// refresh_ref.hpp -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth
// (:330-371), monocular, restated over the arrays of a keyframe store and its map-point pool (include/orbslamm_refresh.h,
// DESIGN.md §8w).  Plain C++11, no project header: the side the device kernels are held to, byte for byte.  Build with
// -ffp-contract=off: every float operation below is one IEEE operation.
//
// The arrays: per keyframe slot k < kfcap: entries[k * stride .. + stride) (pool id, -1 empty, bit 30 = in the match slot but
// not in the point's observations), kfFlags[k] (bit 0 isBad(), bit 1 set), octaves[k * stride ..], desc[(k * stride + i) * 32 ..]
// (mDescriptors.row(i)), centres[3 k ..] (GetCameraCenter()).  Per pool id: the OrbwPoint fields as arrays.  Both members go
// through MapPoint::mObservations, built here as an index per pool id of the voting entries in ascending (keyframe, feature):
// the reference's walk, not the device's passes.  map<KeyFrame*,size_t>'s heap-address order is DEFINED as that order.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace refresh_ref {

const int32_t kNoVote = 1 << 30;
enum { kDescriptor = 1, kNormalDepth = 2 };
enum { ST_NOT_ASKED = 0, ST_DONE, ST_BAD, ST_NO_OBSERVATION, ST_ALL_KF_BAD, ST_NO_REF, ST_LEVEL_RANGE };

struct Store {
    int kfcap, stride;
    const int32_t* entries;
    const uint8_t* kfFlags;
    const uint8_t* octaves;
    const uint8_t* desc;
    const float* centres;
    int poolCap;
    const float* pos;        // [3 poolCap]
    const float* normal;     // [3 poolCap]
    const float* minD;
    const float* maxD;
    const uint8_t* ptDesc;   // [32 poolCap]
    const uint8_t* ptFlags;  // bit 0 isBad()
};

// OrbrPoint's layout
struct Point {
    float pos[3], normal[3];
    float minDistance, maxDistance;
    uint8_t desc[32];
    int32_t nObs, nDesc, bestKf, bestIdx;
    uint8_t stDescriptor, stNormalDepth, pad[2];
};

// which branches ran, for the tests that must see each one
struct Branches {
    int badPoint, noObservation, badKfSkipped, allKfBad, n1, n2, nOdd, nEven, tieAtBest, duplicateEntry, noRef, levelRange, singleObserver;
};
const int kBranchInts = 13;

// MapPoint::mObservations of every point: AddObservation(pKF, idx) for every voting entry of every set keyframe
struct Observations {
    std::vector<int32_t> start, kf, idx;
    explicit Observations(const Store& s) : start((size_t)s.poolCap + 1, 0)
    {
        for (int pass = 0; pass < 2; pass++) {
            std::vector<int32_t> fill(start.begin(), start.end() - 1);
            for (int k = 0; k < s.kfcap; k++) {
                if (!(s.kfFlags[k] & 2)) continue;
                for (int i = 0; i < s.stride; i++) {
                    const int32_t v = s.entries[(size_t)k * s.stride + i];
                    if (v < 0 || (v & kNoVote) || v >= s.poolCap) continue;
                    if (pass == 0) start[(size_t)v + 1]++;
                    else { kf[(size_t)fill[v]] = k; idx[(size_t)fill[v]] = i; fill[v]++; }
                }
            }
            if (pass == 0) {
                for (int p = 0; p < s.poolCap; p++) start[(size_t)p + 1] += start[(size_t)p];
                kf.resize((size_t)start[(size_t)s.poolCap]); idx.resize(kf.size());
            }
        }
    }
};

inline int descriptorDistance(const uint8_t* a, const uint8_t* b)   // ORBmatcher::DescriptorDistance: the bits that differ
{
    int d = 0;
    for (int w = 0; w < 8; w++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * w, 4); std::memcpy(&y, b + 4 * w, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

inline double norm3(const float* v)   // cv::norm (NORM_L2) of a CV_32F 3-vector: a double sum of squares in order, sqrt
{
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
    return std::sqrt(s);
}

// MapPoint.cc:242-307.  Returns the status; on ST_DONE out.desc / bestKf / bestIdx are the winner's
inline int computeDistinctiveDescriptors(const Store& s, const Observations& obs, int32_t id, Point& out, Branches& br)
{
    if (s.ptFlags[id] & 1) { br.badPoint++; return ST_BAD; }                        // :251 mbBad
    const int32_t o0 = obs.start[(size_t)id], o1 = obs.start[(size_t)id + 1];       // :253 observations = mObservations
    if (o0 == o1) { br.noObservation++; return ST_NO_OBSERVATION; }                 // :256
    std::vector<int32_t> which;                                                     // :245 vDescriptors, as observation numbers
    for (int32_t o = o0; o < o1; o++) {                                             // :261
        if (o > o0 && obs.kf[(size_t)o] == obs.kf[(size_t)o - 1]) br.duplicateEntry++;
        if (s.kfFlags[obs.kf[(size_t)o]] & 1) { br.badKfSkipped++; continue; }      // :265 !pKF->isBad()
        which.push_back(o);                                                         // :266
    }
    if (which.empty()) { br.allKfBad++; return ST_ALL_KF_BAD; }                     // :269
    const size_t N = which.size();                                                  // :273
    if (N == 1) br.n1++; else if (N == 2) br.n2++; else if (N & 1) br.nOdd++; else br.nEven++;
    std::vector<const uint8_t*> d(N);
    for (size_t i = 0; i < N; i++) d[i] = s.desc + ((size_t)obs.kf[(size_t)which[i]] * s.stride + (size_t)obs.idx[(size_t)which[i]]) * 32;
    std::vector<float> Distances(N * N);                                            // :275
    for (size_t i = 0; i < N; i++) {                                                // :276
        Distances[i * N + i] = 0;                                                   // :278
        for (size_t j = i + 1; j < N; j++) {                                        // :279
            const int distij = descriptorDistance(d[i], d[j]);                      // :281
            Distances[i * N + j] = (float)distij;                                   // :282
            Distances[j * N + i] = (float)distij;                                   // :283
        }
    }
    int BestMedian = INT_MAX;                                                       // :288
    int BestIdx = 0;                                                                // :289
    bool tie = false;
    for (size_t i = 0; i < N; i++) {                                                // :290
        std::vector<int> vDists(Distances.begin() + (ptrdiff_t)(i * N), Distances.begin() + (ptrdiff_t)(i * N + N));   // :292
        std::sort(vDists.begin(), vDists.end());                                    // :293
        const int median = vDists[(size_t)(0.5 * (double)(N - 1))];                 // :294
        if (median == BestMedian) tie = true;
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; tie = false; }   // :296-300
    }
    if (tie) br.tieAtBest++;
    std::memcpy(out.desc, d[(size_t)BestIdx], 32);                                  // :305
    out.bestKf = obs.kf[(size_t)which[(size_t)BestIdx]]; out.bestIdx = obs.idx[(size_t)which[(size_t)BestIdx]];
    return ST_DONE;
}

// MapPoint.cc:330-371.  P: mWorldPos.  On ST_DONE out.normal / minDistance / maxDistance are the member's
inline int updateNormalAndDepth(const Store& s, const Observations& obs, int32_t id, int32_t refKf, const float* P, const float* sf, int nlevels,
                                Point& out, Branches& br)
{
    if (s.ptFlags[id] & 1) { br.badPoint++; return ST_BAD; }                        // :338
    const int32_t o0 = obs.start[(size_t)id], o1 = obs.start[(size_t)id + 1];       // :340
    if (o0 == o1) { br.noObservation++; return ST_NO_OBSERVATION; }                 // :345
    float normal[3] = {0.f, 0.f, 0.f};                                              // :348
    int n = 0;                                                                      // :349
    int32_t refIdx = -1;
    for (int32_t o = o0; o < o1; o++) {                                             // :350
        const float* Owi = s.centres + 3 * (size_t)obs.kf[(size_t)o];               // :353
        float normali[3];
        for (int c = 0; c < 3; c++) normali[c] = P[c] - Owi[c];                     // :354
        const double nd = norm3(normali);
        const float a = (float)(1. / nd);                                           // :355 normali / cv::norm(normali): the scale as a float,
        for (int c = 0; c < 3; c++) { const float t = normali[c] * a; normal[c] = t + normal[c]; }   // a float product, a float sum
        n++;                                                                        // :356
        if (refIdx < 0 && obs.kf[(size_t)o] == refKf) refIdx = obs.idx[(size_t)o];  // observations[pRefKF]: the lowest feature
    }
    if (refKf < 0 || refIdx < 0) { br.noRef++; return ST_NO_REF; }                  // DEFINED: the reference inserts a zero index (:361)
    const int level = s.octaves[(size_t)refKf * s.stride + (size_t)refIdx];         // :361
    if (level < 0 || level >= nlevels) { br.levelRange++; return ST_LEVEL_RANGE; }  // DEFINED: the reference reads out of bounds (:362)
    float PC[3];
    for (int c = 0; c < 3; c++) PC[c] = P[c] - s.centres[3 * (size_t)refKf + c];    // :359
    const float dist = (float)norm3(PC);                                            // :360
    const float levelScaleFactor = sf[level];                                       // :362
    out.maxDistance = dist * levelScaleFactor;                                      // :367
    out.minDistance = out.maxDistance / sf[nlevels - 1];                            // :368
    const double alpha = 1. / n;                                                    // :369 normal / n: MatOp_AddEx with alpha = 1. / n
    if (alpha == 1.) br.singleObserver++;
    for (int c = 0; c < 3; c++) out.normal[c] = alpha == 1. ? normal[c] + 0.f : (float)((double)normal[c] * alpha);
    return ST_DONE;
}

// one point of orbr_refresh_points: the record as it stands after the call
inline void refreshPoint(const Store& s, const Observations& obs, int32_t id, int32_t refKf, const float* newPos, int what, const float* sf, int nlevels,
                         Point& out, Branches* brp)
{
    Branches none = Branches();
    Branches& br = brp ? *brp : none;
    std::memset(&out, 0, sizeof out);
    for (int c = 0; c < 3; c++) { out.pos[c] = newPos ? newPos[c] : s.pos[3 * (size_t)id + c]; out.normal[c] = s.normal[3 * (size_t)id + c]; }   // SetWorldPos first
    out.minDistance = s.minD[id]; out.maxDistance = s.maxD[id];
    std::memcpy(out.desc, s.ptDesc + 32 * (size_t)id, 32);
    out.bestKf = -1; out.bestIdx = -1;
    out.nObs = obs.start[(size_t)id + 1] - obs.start[(size_t)id];
    for (int32_t o = obs.start[(size_t)id]; o < obs.start[(size_t)id + 1]; o++) out.nDesc += (s.kfFlags[obs.kf[(size_t)o]] & 1) ? 0 : 1;
    out.stDescriptor = ST_NOT_ASKED; out.stNormalDepth = ST_NOT_ASKED;
    if (what & kDescriptor) {
        Point t = out;
        out.stDescriptor = (uint8_t)computeDistinctiveDescriptors(s, obs, id, t, br);
        if (out.stDescriptor == ST_DONE) { std::memcpy(out.desc, t.desc, 32); out.bestKf = t.bestKf; out.bestIdx = t.bestIdx; }
    }
    if (what & kNormalDepth) {
        Point t = out;
        out.stNormalDepth = (uint8_t)updateNormalAndDepth(s, obs, id, refKf, out.pos, sf, nlevels, t, br);
        if (out.stNormalDepth == ST_DONE) { for (int c = 0; c < 3; c++) out.normal[c] = t.normal[c]; out.minDistance = t.minDistance; out.maxDistance = t.maxDistance; }
    }
}

}  // namespace refresh_ref
