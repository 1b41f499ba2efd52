// loopfuse_ref.hpp -- a literal C++ restatement of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (src/ORBmatcher.cc:979-1102 of both scenarios, monocular) for a target whose Scw the caller has already decomposed
// (:987-992) into Rcw, tcw and Ow, of LoopClosing::SearchAndFuse (src/LoopClosing.cc:601-627) and MultiMapper::SearchAndFuse
// (src/MultiMapper.cc:668-694) over a small map model, of MapPoint::Replace and MapPoint::ComputeDistinctiveDescriptors
// (MapPoint.cc:177-215, 242-307), of KeyFrame::GetMapPoints (KeyFrame.cc:246-259), of the keyframe grid (Frame.cc:230-245,
// 382-392, KeyFrame.cc:618-657) and of the OpenCV 3.0 pieces :1014-1044 call (gemm's small-matrix branch with C, norm and
// dot on CV_32F).  It is the checker of the device SearchAndFuse (orbslamm_amd/csrc/orbc_kernels.hip): it includes no
// header of the project and is built with g++ -ffp-contract=off (every operation one IEEE op).  The OpenCV pieces are
// restated from the published 3.0 source and are UNPINNED.
//
// Against Fuse(pKF, vpMapPoints, th) (tools/fuse_ref.hpp): invz is `1.0/z` rounded to float (:1021), there is NO chi-square
// test in the window (:1064-1081), a hit is bestDist <= TH_LOW with no Observations() comparison: a feature that holds a
// point goes to vpReplacePoint, and the Replace calls are issued after the loop over the points (LoopClosing.cc:616-625).
// PredictScale is the DIRECT formula, ceil(log(ratio)/logScaleFactor) in float, not a break table.  Defined choices
// (DESIGN.md section 8m), the same on the device:
//   - a level that is NaN or outside [0, nlevels) ends the pair (LEVEL_RANGE; the reference reads mvScaleFactors out of
//     bounds there) and is reported as -1 (below, or NaN) or nlevels (above)
//   - std::map<KeyFrame*, size_t> is walked in pointer order in the reference; the model walks observations in insertion order
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>

namespace loopfuse_ref {

struct KeyPt { float x, y, size, angle, response; int32_t octave, class_id; };   // cv::KeyPoint's layout
struct Grid { float minX, minY, invW, invH; int32_t cols, rows; };
struct Target { float Rcw[9], tcw[3], Ow[3], K[4]; float minX, maxX, minY, maxY; Grid grid; };   // OrblFuseTarget's layout
struct Point { float pos[3], normal[3], minDistance, maxDistance; uint8_t desc[32]; };            // OrblFusePoint's layout
struct Result { int32_t bestIdx, bestDist; float u, v; int8_t level; uint8_t status, pad[2]; };  // OrblFuseResult's layout
struct Gates { float z, dist3D, minDistance, maxDistance, ratio, radius; double dot; };           // what the gates compared
struct Hit { int32_t target, point, bestIdx, bestDist; };                                         // OrbcHit's layout

enum Status : uint8_t { DEPTH = 0, OUTSIDE_IMAGE, DISTANCE, VIEW_ANGLE, LEVEL_RANGE, NO_CANDIDATE, FOUND };
const int TH_LOW = 50;

// :1021 `const float invz = 1.0/p3Dc.at<float>(2);` as written, and the float division a device may use in its place
inline float invzAsWritten(float z) { return (float)(1.0 / (double)z); }
inline float invzFloatDivision(float z) { return 1.0f / z; }

// MapPoint::PredictScale's expression (MapPoint.cc:393) as a float; the caller range-checks before any conversion
inline float predictLevel(float ratio, float logScaleFactor) { return std::ceil(std::log(ratio) / logScaleFactor); }

// :1010-1051 for one pair.  Returns true when the pair reaches the window search; r holds u, v, level and the gate's status
inline bool project(const Target& T, const Point& P, float th, const float* scaleFactors, int nlevels, float logScaleFactor, Result& r,
                    Gates* g = nullptr)
{
    r.bestIdx = -1; r.bestDist = 256; r.u = 0.f; r.v = 0.f; r.level = -1; r.status = DEPTH; r.pad[0] = r.pad[1] = 0;
    if (g) { g->z = g->dist3D = g->minDistance = g->maxDistance = g->ratio = g->radius = NAN; g->dot = NAN; }
    // p3Dc = Rcw*p3Dw + tcw: one gemm(Rcw, p3Dw, 1, tcw, 1), the small-matrix branch: float products summed left to right,
    // then (float)(t*1.0 + c*1.0)
    float pc[3];
    for (int i = 0; i < 3; i++) {
        const float t = T.Rcw[3 * i] * P.pos[0] + T.Rcw[3 * i + 1] * P.pos[1] + T.Rcw[3 * i + 2] * P.pos[2];
        pc[i] = (float)((double)t * 1.0 + (double)T.tcw[i] * 1.0);
    }
    if (g) g->z = pc[2];
    if (pc[2] < 0.0f) return false;
    const float invz = invzAsWritten(pc[2]);
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = T.K[0] * x + T.K[2], v = T.K[1] * y + T.K[3];
    r.u = u; r.v = v;
    r.status = OUTSIDE_IMAGE;
    if (!(u >= T.minX && u < T.maxX && v >= T.minY && v < T.maxY)) return false;   // KeyFrame::IsInImage
    const float maxDistance = 1.2f * P.maxDistance, minDistance = 0.8f * P.minDistance;   // MapPoint.cc:373-383
    float PO[3];
    for (int i = 0; i < 3; i++) PO[i] = P.pos[i] - T.Ow[i];
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)PO[i] * (double)PO[i];
    const float dist3D = (float)std::sqrt(s);   // cv::norm: normL2_<float, double>
    if (g) { g->dist3D = dist3D; g->minDistance = minDistance; g->maxDistance = maxDistance; }
    r.status = DISTANCE;
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    double dt = 0;
    for (int i = 0; i < 3; i++) dt += (double)PO[i] * (double)P.normal[i];   // Mat::dot: dotProd_<float>, a double sum
    if (g) g->dot = dt;
    r.status = VIEW_ANGLE;
    if (dt < 0.5 * dist3D) return false;
    const float ratio = P.maxDistance / dist3D;
    const float lv = predictLevel(ratio, logScaleFactor);
    if (g) g->ratio = ratio;
    r.status = LEVEL_RANGE;
    if (!(lv >= 0.f)) { r.level = -1; return false; }
    if (!(lv < (float)nlevels)) { r.level = (int8_t)nlevels; return false; }
    r.level = (int8_t)(int)lv;
    if (g) g->radius = th * scaleFactors[r.level];
    r.status = NO_CANDIDATE;
    return true;
}

// ------------------------------------------------------------------------------------------------ the keyframe grid
struct CellGrid {
    Grid g;
    std::vector<std::vector<int> > cell;   // [ix * rows + iy]: feature indices in insertion order
    void build(const Grid& grid, const KeyPt* keys, int n)
    {
        g = grid;
        cell.assign((size_t)g.cols * g.rows, std::vector<int>());
        for (int i = 0; i < n; i++) {   // Frame.cc:230-245, PosInGrid :382-392
            const float fx = std::round((keys[i].x - g.minX) * g.invW), fy = std::round((keys[i].y - g.minY) * g.invH);
            if (!(fx >= 0.f && fx < (float)g.cols && fy >= 0.f && fy < (float)g.rows)) continue;
            cell[(size_t)(int)fx * g.rows + (int)fy].push_back(i);
        }
    }
    // KeyFrame::GetFeaturesInArea (KeyFrame.cc:618-657)
    void inArea(const KeyPt* keys, float x, float y, float r, std::vector<int>& out) const
    {
        out.clear();
        const int nMinCellX = std::max(0, (int)std::floor((x - g.minX - r) * g.invW));
        if (nMinCellX >= g.cols) return;
        const int nMaxCellX = std::min(g.cols - 1, (int)std::ceil((x - g.minX + r) * g.invW));
        if (nMaxCellX < 0) return;
        const int nMinCellY = std::max(0, (int)std::floor((y - g.minY - r) * g.invH));
        if (nMinCellY >= g.rows) return;
        const int nMaxCellY = std::min(g.rows - 1, (int)std::ceil((y - g.minY + r) * g.invH));
        if (nMaxCellY < 0) return;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<int>& c = cell[(size_t)ix * g.rows + iy];
                for (size_t j = 0; j < c.size(); j++) {
                    const KeyPt& kp = keys[c[j]];
                    const float distx = kp.x - x, disty = kp.y - y;
                    if (std::fabs(distx) < r && std::fabs(disty) < r) out.push_back(c[j]);
                }
            }
    }
};

inline int descriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// :1053-1081 for a pair that passed project(): the best feature of the window under the point's descriptor, no chi-square
inline void searchWindow(const CellGrid& grid, const KeyPt* keys, const uint8_t* desc, float u, float v, float radius, int pred,
                         const uint8_t* dMP, int& bestIdx, int& bestDist)
{
    std::vector<int> vIndices;
    grid.inArea(keys, u, v, radius, vIndices);
    bestDist = 256; bestIdx = -1;   // (INT_MAX in the reference: reported as 256, above every distance)
    for (size_t k = 0; k < vIndices.size(); k++) {
        const int idx = vIndices[k];
        const int kpLevel = keys[idx].octave;
        if (kpLevel < pred - 1 || kpLevel > pred) continue;
        const int dist = descriptorDistance(dMP, desc + (size_t)idx * 32);
        if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
    }
}

// :1010-1081 for one (target, point) pair
inline Result pair(const Target& T, const CellGrid& grid, const KeyPt* keys, const uint8_t* desc, const Point& P, float th,
                   const float* scaleFactors, int nlevels, float logScaleFactor, Gates* g = nullptr)
{
    Result r;
    if (!project(T, P, th, scaleFactors, nlevels, logScaleFactor, r, g)) return r;
    int bi, bd;
    searchWindow(grid, keys, desc, r.u, r.v, th * scaleFactors[r.level], r.level, P.desc, bi, bd);
    r.bestIdx = bi; r.bestDist = bd;
    r.status = bi >= 0 ? FOUND : NO_CANDIDATE;
    return r;
}

// ------------------------------------------------------------------------------------------------ the serial map model
struct Event { int32_t type, a, b, c; };   // REPLACE: a replaced by b at target number c; ADD: point a observed by keyframe b at feature c
enum { EV_REPLACE = 1, EV_ADD = 2 };

struct Model {
    struct KF {
        std::vector<KeyPt> keys; std::vector<uint8_t> desc; CellGrid grid;
        std::vector<int> slot;   // mvpMapPoints: a point id or -1
        bool bad;
    };
    struct MP {
        Point rec; std::vector<std::pair<int, int> > obs;   // (keyframe, feature) in insertion order
        bool bad; int replaced; int nvisible, nfound;
    };
    struct Corrected { int kf; Target rec; };   // one entry of CorrectedSim3: the keyframe and its decomposed Scw
    std::vector<KF> kfs;
    std::vector<MP> mps;
    std::vector<Event> events;
    std::vector<float> sf; float logScaleFactor;
    long rescored = 0;   // searchAndFuseByRule: the pairs scored again on the host

    int addKeyFrame(const Grid& grid, const KeyPt* keys, const uint8_t* desc, int n)
    {
        KF k; k.keys.assign(keys, keys + n); k.desc.assign(desc, desc + (size_t)n * 32);
        k.grid.build(grid, keys, n); k.slot.assign((size_t)n, -1); k.bad = false;
        kfs.push_back(k);
        return (int)kfs.size() - 1;
    }
    int addMapPoint(const Point& rec)
    {
        MP p; p.rec = rec; p.bad = false; p.replaced = -1; p.nvisible = p.nfound = 1;
        mps.push_back(p);
        return (int)mps.size() - 1;
    }
    bool isInKeyFrame(int mp, int kf) const
    {
        for (size_t i = 0; i < mps[mp].obs.size(); i++) if (mps[mp].obs[i].first == kf) return true;
        return false;
    }
    void addObservation(int mp, int kf, int idx) { if (!isInKeyFrame(mp, kf)) mps[mp].obs.push_back(std::make_pair(kf, idx)); }
    // KeyFrame.cc:246-259
    std::set<int> getMapPoints(int kf) const
    {
        std::set<int> s;
        for (size_t i = 0; i < kfs[kf].slot.size(); i++) if (kfs[kf].slot[i] >= 0 && !mps[kfs[kf].slot[i]].bad) s.insert(kfs[kf].slot[i]);
        return s;
    }
    // MapPoint.cc:242-307
    void computeDistinctiveDescriptors(int mp)
    {
        MP& p = mps[mp];
        if (p.bad || p.obs.empty()) return;
        std::vector<const uint8_t*> vd;
        for (size_t i = 0; i < p.obs.size(); i++)
            if (!kfs[p.obs[i].first].bad) vd.push_back(&kfs[p.obs[i].first].desc[(size_t)p.obs[i].second * 32]);
        if (vd.empty()) return;
        const size_t N = vd.size();
        std::vector<float> D(N * N, 0.f);
        for (size_t i = 0; i < N; i++)
            for (size_t j = i + 1; j < N; j++) D[i * N + j] = D[j * N + i] = (float)descriptorDistance(vd[i], vd[j]);
        int bestMedian = INT_MAX, bestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            std::vector<int> v(D.begin() + i * N, D.begin() + (i + 1) * N);
            std::sort(v.begin(), v.end());
            const int median = v[(size_t)(0.5 * (N - 1))];
            if (median < bestMedian) { bestMedian = median; bestIdx = (int)i; }
        }
        uint8_t tmp[32];
        std::memcpy(tmp, vd[bestIdx], 32);
        std::memcpy(p.rec.desc, tmp, 32);
    }
    // MapPoint.cc:177-215: `self` is replaced by `by`
    void replace(int self, int by, int atTarget)
    {
        if (self == by) return;
        events.push_back(Event{EV_REPLACE, self, by, atTarget});
        std::vector<std::pair<int, int> > obs;
        obs.swap(mps[self].obs);
        mps[self].bad = true;
        const int nvisible = mps[self].nvisible, nfound = mps[self].nfound;
        mps[self].replaced = by;
        for (size_t i = 0; i < obs.size(); i++) {
            const int kf = obs[i].first, idx = obs[i].second;
            if (!isInKeyFrame(by, kf)) { kfs[kf].slot[idx] = by; addObservation(by, kf, idx); }
            else kfs[kf].slot[idx] = -1;
        }
        mps[by].nfound += nfound; mps[by].nvisible += nvisible;
        computeDistinctiveDescriptors(by);
    }
    Result search(const Corrected& c, int mp, float th) const
    {
        const KF& K = kfs[c.kf];
        return pair(c.rec, K.grid, K.keys.data(), K.desc.data(), mps[mp].rec, th, sf.data(), (int)sf.size(), logScaleFactor);
    }
    // :1083-1098: what Fuse does with a pair's best
    void apply(const Corrected& c, int mp, int i, int bestIdx, std::vector<int>& vpReplacePoint)
    {
        KF& K = kfs[c.kf];
        const int inKF = K.slot[bestIdx];
        if (inKF >= 0) {
            if (!mps[inKF].bad) vpReplacePoint[i] = inKF;
        } else {
            events.push_back(Event{EV_ADD, mp, c.kf, bestIdx});
            addObservation(mp, c.kf, bestIdx);
            K.slot[bestIdx] = mp;
        }
    }
    // LoopClosing.cc:601-627 / MultiMapper.cc:668-694 with ORBmatcher.cc:979-1102 inside, serially: the total of nFused
    int searchAndFuse(const std::vector<Corrected>& corrected, const std::vector<int>& loopPoints, float th)
    {
        int total = 0;
        for (size_t t = 0; t < corrected.size(); t++) {
            const Corrected& c = corrected[t];
            std::vector<int> vpReplacePoints(loopPoints.size(), -1);
            const std::set<int> spAlreadyFound = getMapPoints(c.kf);
            for (size_t i = 0; i < loopPoints.size(); i++) {
                const int mp = loopPoints[i];
                if (mps[mp].bad || spAlreadyFound.count(mp)) continue;
                const Result r = search(c, mp, th);
                if (r.status != FOUND || r.bestDist > TH_LOW) continue;
                apply(c, mp, (int)i, r.bestIdx, vpReplacePoints);
                total++;
            }
            for (size_t i = 0; i < loopPoints.size(); i++)
                if (vpReplacePoints[i] >= 0) replace(vpReplacePoints[i], loopPoints[i], (int)t);
        }
        return total;
    }
    // The dense search of every loop point in every target on the map as it stands: what the device returns (hits in
    // target-major order, points ascending; hitStart of corrected.size() + 1 entries)
    void dense(const std::vector<Corrected>& corrected, const std::vector<int>& loopPoints, float th, int maxDist, std::vector<Hit>& hits,
               std::vector<int>& hitStart) const
    {
        hits.clear(); hitStart.assign(1, 0);
        for (size_t t = 0; t < corrected.size(); t++) {
            for (size_t i = 0; i < loopPoints.size(); i++) {
                const Result r = search(corrected[t], loopPoints[i], th);
                if (r.bestIdx >= 0 && r.bestDist <= maxDist) hits.push_back(Hit{(int32_t)t, (int32_t)i, r.bestIdx, r.bestDist});
            }
            hitStart.push_back((int)hits.size());
        }
    }
    // The parallel rule: all pairs searched up front on the map as it stands, the serial part replayed
    // in the reference's order, and a pair of a point that has SURVIVED a Replace (its descriptor may have changed) scored
    // again with the descriptor it holds now.  rescore = false leaves that out: the rule is then wrong, and the tests show it.
    int searchAndFuseByRule(const std::vector<Corrected>& corrected, const std::vector<int>& loopPoints, float th, bool rescore = true)
    {
        std::vector<Hit> hits;
        std::vector<int> hitStart;
        dense(corrected, loopPoints, th, TH_LOW, hits, hitStart);
        std::set<int> survivors;
        int total = 0;
        rescored = 0;
        for (size_t t = 0; t < corrected.size(); t++) {
            const Corrected& c = corrected[t];
            std::vector<int> vpReplacePoints(loopPoints.size(), -1);
            const std::set<int> spAlreadyFound = getMapPoints(c.kf);
            int cur = hitStart[t];
            for (size_t i = 0; i < loopPoints.size(); i++) {
                const int mp = loopPoints[i];
                while (cur < hitStart[t + 1] && hits[cur].point < (int)i) cur++;
                if (mps[mp].bad || spAlreadyFound.count(mp)) continue;
                int bestIdx = -1;
                if (rescore && survivors.count(mp)) {
                    rescored++;
                    const Result r = search(c, mp, th);
                    if (r.status == FOUND && r.bestDist <= TH_LOW) bestIdx = r.bestIdx;
                } else if (cur < hitStart[t + 1] && hits[cur].point == (int)i) bestIdx = hits[cur].bestIdx;
                if (bestIdx < 0) continue;
                apply(c, mp, (int)i, bestIdx, vpReplacePoints);
                total++;
            }
            for (size_t i = 0; i < loopPoints.size(); i++)
                if (vpReplacePoints[i] >= 0) { replace(vpReplacePoints[i], loopPoints[i], (int)t); survivors.insert(loopPoints[i]); }
        }
        return total;
    }
};

}  // namespace loopfuse_ref
