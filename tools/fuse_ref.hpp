// fuse_ref.hpp -- a literal C++ restatement of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:827-975 of both
// scenarios, monocular: mvuRight < 0 everywhere, so the chi-square gate is 5.99 and ur is not formed), of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:454-534) over a small map model, of MapPoint::Replace and
// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:177-215, 242-307), of the keyframe grid (Frame.cc:230-245, 382-392,
// KeyFrame.cc:618-657) and of the OpenCV 3.0 pieces :855-892 call (gemm's small-matrix branch with C, norm and dot on
// CV_32F).  It is the checker of the device SearchInNeighbors (orbslamm_amd/csrc/orbl_kernels.hip, k_fuse_batch): it
// includes no header of the library and is built with g++ -ffp-contract=off (every operation one IEEE op).  The OpenCV
// pieces are restated from the published 3.0 source and are UNPINNED.
//
// Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:979-1102) is the same code except at three points.  Two are parameters here,
// which tools/loopfuse_ref.hpp sets: invz (`1/z` in float here, `1.0/z` rounded to float there: project's Invz) and the 5.99
// chi-square test of the window (absent there: a null invLevelSigma2).  The third, what a hit does to the map, belongs to the
// serial loop each caller models (Model::fuse here, loopfuse_ref::Model::apply there).
//
// PredictScale is the DIRECT formula here, ceil(log(ratio)/logScaleFactor) in float (tests/cpp/mock_slam.hpp:65-68), not a
// break table.  Defined choices, the same on the device:
//   - a level that is NaN or outside [0, nlevels) ends the pair (LEVEL_RANGE; the reference reads mvScaleFactors out of
//     bounds there) and is reported as -1 (below, or NaN) or nlevels (above); no float is converted to int out of range
//   - std::map<KeyFrame*, size_t> is walked in pointer order in the reference; the model walks observations in insertion order
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// The records live in a namespace of their own, so that argument-dependent lookup on them finds no function: loopfuse_ref
// re-exports them and defines a `project` of its own, and a call of either one, unqualified, must not see the other.
namespace fuse_records {

struct KeyPt { float x, y, size, angle, response; int32_t octave, class_id; };   // cv::KeyPoint's layout
struct Grid { float minX, minY, invW, invH; int32_t cols, rows; };
struct Target { float Rcw[9], tcw[3], Ow[3], K[4]; float minX, maxX, minY, maxY; Grid grid; };   // OrblFuseTarget's layout
struct Point { float pos[3], normal[3], minDistance, maxDistance; uint8_t desc[32]; };            // OrblFusePoint's layout
struct Result { int32_t bestIdx, bestDist; float u, v; int8_t level; uint8_t status, pad[2]; };  // OrblFuseResult's layout
struct Gates { float z, dist3D, minDistance, maxDistance, ratio, radius; double dot; };           // what the gates compared

}  // namespace fuse_records

namespace fuse_ref {

using fuse_records::KeyPt;
using fuse_records::Grid;
using fuse_records::Target;
using fuse_records::Point;
using fuse_records::Result;
using fuse_records::Gates;

enum Status : uint8_t { DEPTH = 0, OUTSIDE_IMAGE, DISTANCE, VIEW_ANGLE, LEVEL_RANGE, NO_CANDIDATE, FOUND };
const int TH_LOW = 50;

// MapPoint::PredictScale's expression (MapPoint.cc:393) as a float; the caller range-checks before any conversion
inline float predictLevel(float ratio, float logScaleFactor) { return std::ceil(std::log(ratio) / logScaleFactor); }

// :862 `const float invz = 1/p3Dc.at<float>(2);`: a float division
typedef float (*Invz)(float);
inline float invzFloatDivision(float z) { return 1.0f / z; }

// :855-892 for one pair.  Returns true when the pair reaches the window search; r holds u, v, level and the gate's status
inline bool project(const Target& T, const Point& P, float th, const float* scaleFactors, int nlevels, float logScaleFactor, Result& r,
                    Gates* g = nullptr, Invz invzOf = invzFloatDivision)
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
    const float invz = invzOf(pc[2]);
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

// :894-951 for a pair that passed project(): the best feature of the window under the point's descriptor; a null
// invLevelSigma2 leaves the chi-square test out (bestDist starts at INT_MAX in the reference: reported as 256, above every
// distance)
inline void searchWindow(const CellGrid& grid, const KeyPt* keys, const uint8_t* desc, float u, float v, float radius, int pred,
                         const float* invLevelSigma2, const uint8_t* dMP, int& bestIdx, int& bestDist)
{
    std::vector<int> vIndices;
    grid.inArea(keys, u, v, radius, vIndices);
    bestDist = 256; bestIdx = -1;
    for (size_t k = 0; k < vIndices.size(); k++) {
        const int idx = vIndices[k];
        const KeyPt& kp = keys[idx];
        const int kpLevel = kp.octave;
        if (kpLevel < pred - 1 || kpLevel > pred) continue;
        if (invLevelSigma2) {
            const float ex = u - kp.x, ey = v - kp.y;
            const float e2 = ex * ex + ey * ey;
            if (e2 * invLevelSigma2[kpLevel] > 5.99) continue;
        }
        const int dist = descriptorDistance(dMP, desc + (size_t)idx * 32);
        if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
    }
}

// :855-951 for one (target, point) pair
inline Result pair(const Target& T, const CellGrid& grid, const KeyPt* keys, const uint8_t* desc, const Point& P, float th,
                   const float* scaleFactors, const float* invLevelSigma2, int nlevels, float logScaleFactor, Gates* g = nullptr,
                   Invz invzOf = invzFloatDivision)
{
    Result r;
    if (!project(T, P, th, scaleFactors, nlevels, logScaleFactor, r, g, invzOf)) return r;
    int bi, bd;
    searchWindow(grid, keys, desc, r.u, r.v, th * scaleFactors[r.level], r.level, invLevelSigma2, P.desc, bi, bd);
    r.bestIdx = bi; r.bestDist = bd;
    r.status = bi >= 0 ? FOUND : NO_CANDIDATE;
    return r;
}

// ------------------------------------------------------------------------------------------------ the serial map model
struct Event { int32_t type, a, b, c; };   // REPLACE: a replaced by b at target c; ADD: point a observed by keyframe b at feature c
enum { EV_REPLACE = 1, EV_ADD = 2 };

struct Model {
    struct KF {
        Target rec; std::vector<KeyPt> keys; std::vector<uint8_t> desc; CellGrid grid;
        std::vector<int> slot;            // mvpMapPoints: a point id or -1
        std::vector<int> covis;           // GetBestCovisibilityKeyFrames' order
        bool bad; long fuseTargetFor;
    };
    struct MP {
        Point rec; std::vector<std::pair<int, int> > obs;   // (keyframe, feature) in insertion order
        bool bad; int replaced; long fuseCandidateFor; int nvisible, nfound;
    };
    std::vector<KF> kfs;
    std::vector<MP> mps;
    std::vector<Event> events;
    float th; std::vector<float> sf, invSigma2; float logScaleFactor;
    // called for every pair that reached the window search: a caller's second opinion (the C oracle's window_best)
    void (*windowCheck)(const Model& m, int kf, const Point& P, const Result& r) = nullptr;

    int addKeyFrame(const Target& rec, const KeyPt* keys, const uint8_t* desc, int n)
    {
        KF k; k.rec = rec; k.keys.assign(keys, keys + n); k.desc.assign(desc, desc + (size_t)n * 32);
        k.grid.build(rec.grid, keys, n); k.slot.assign((size_t)n, -1); k.bad = false; k.fuseTargetFor = -1;
        kfs.push_back(k);
        return (int)kfs.size() - 1;
    }
    int addMapPoint(const Point& rec)
    {
        MP p; p.rec = rec; p.bad = false; p.replaced = -1; p.fuseCandidateFor = -1; p.nvisible = p.nfound = 1;
        mps.push_back(p);
        return (int)mps.size() - 1;
    }
    int indexInKeyFrame(int mp, int kf) const
    {
        for (size_t i = 0; i < mps[mp].obs.size(); i++) if (mps[mp].obs[i].first == kf) return mps[mp].obs[i].second;
        return -1;
    }
    bool isInKeyFrame(int mp, int kf) const { return indexInKeyFrame(mp, kf) >= 0; }
    void addObservation(int mp, int kf, int idx) { if (!isInKeyFrame(mp, kf)) mps[mp].obs.push_back(std::make_pair(kf, idx)); }
    int observations(int mp) const { return (int)mps[mp].obs.size(); }   // monocular: nObs counts one per observation
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
    // ORBmatcher.cc:827-975 on the model; vpMapPoints holds ids, -1 for a null
    int fuse(int kf, const std::vector<int>& vpMapPoints)
    {
        KF& K = kfs[kf];
        int nFused = 0;
        for (size_t i = 0; i < vpMapPoints.size(); i++) {
            const int mp = vpMapPoints[i];
            if (mp < 0) continue;
            if (mps[mp].bad || isInKeyFrame(mp, kf)) continue;
            const Result r = pair(K.rec, K.grid, K.keys.data(), K.desc.data(), mps[mp].rec, th, sf.data(), invSigma2.data(), (int)sf.size(), logScaleFactor);
            if (windowCheck && r.status >= NO_CANDIDATE) windowCheck(*this, kf, mps[mp].rec, r);
            if (r.status != FOUND) continue;
            if (r.bestDist <= TH_LOW) {
                const int inKF = K.slot[r.bestIdx];
                if (inKF >= 0) {
                    if (!mps[inKF].bad) {
                        if (observations(inKF) > observations(mp)) replace(mp, inKF, kf);
                        else replace(inKF, mp, kf);
                    }
                } else {
                    events.push_back(Event{EV_ADD, mp, kf, r.bestIdx});
                    addObservation(mp, kf, r.bestIdx);
                    K.slot[r.bestIdx] = mp;
                }
                nFused++;
            }
        }
        return nFused;
    }
    // LocalMapping.cc:454-530 (monocular: nn = 20); the targets in order, repeats included, into `targets`
    void searchInNeighbors(int cur, std::vector<int>& targets)
    {
        targets.clear();
        const std::vector<int>& neigh = kfs[cur].covis;
        for (size_t a = 0; a < neigh.size() && a < 20; a++) {
            const int i = neigh[a];
            if (kfs[i].bad || kfs[i].fuseTargetFor == cur) continue;
            targets.push_back(i);
            kfs[i].fuseTargetFor = cur;
            const std::vector<int>& second = kfs[i].covis;
            for (size_t b = 0; b < second.size() && b < 5; b++) {
                const int i2 = second[b];
                if (kfs[i2].bad || kfs[i2].fuseTargetFor == cur || i2 == cur) continue;
                targets.push_back(i2);
            }
        }
        const std::vector<int> matches = kfs[cur].slot;
        for (size_t t = 0; t < targets.size(); t++) fuse(targets[t], matches);
        std::vector<int> candidates;
        for (size_t t = 0; t < targets.size(); t++) {
            const std::vector<int> pts = kfs[targets[t]].slot;
            for (size_t j = 0; j < pts.size(); j++) {
                const int mp = pts[j];
                if (mp < 0) continue;
                if (mps[mp].bad || mps[mp].fuseCandidateFor == cur) continue;
                mps[mp].fuseCandidateFor = cur;
                candidates.push_back(mp);
            }
        }
        fuse(cur, candidates);
        // the update loop's ComputeDistinctiveDescriptors (:518-530; UpdateNormalAndDepth sums in pointer order and is not modelled)
        const std::vector<int> after = kfs[cur].slot;
        for (size_t i = 0; i < after.size(); i++)
            if (after[i] >= 0 && !mps[after[i]].bad) computeDistinctiveDescriptors(after[i]);
    }
};

}  // namespace fuse_ref
