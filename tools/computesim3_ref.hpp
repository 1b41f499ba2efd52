// computesim3_ref.hpp -- a serial restatement of what LoopClosing::ComputeSim3 (src/LoopClosing.cc:296-347) and MultiMapper::Run do
// per candidate behind Sim3Solver::iterate, for the tests and for tools/computesim3_bench.py: ORBmatcher::SearchBySim3
// (src/ORBmatcher.cc:1104-1328, `m:LINE`), the walk of Optimizer::OptimizeSim3 (src/Optimizer.cc:1401-1481, `o:LINE`) and its solve
// and checks (o:1484-1541: sim3opt_ref.hpp's optimizeSim3, Defined mode), over plain arrays: the map points as a pool of records,
// GetMapPointMatches() as rows of pool ids (-1 null; bit 30 set: the point does not list the keyframe in its observations), the
// entering vpMatches12 as ids with their GetIndexInKeyFrame(pKF2).  Plain C++11 with the standard library alone; it includes
// sim3opt_ref.hpp for the solve and no header of the library.  Build with -ffp-contract=off.
// Readings chosen (include/orbslamm_computesim3.h states the same): the cv::Mat expressions in the adapter's cvsem arithmetic
// (include/ORBmatcher_hip.hpp:785-835); PredictScale through the break table of orbl_level_breaks; a level outside [0, nlevels)
// skips the point; a feature at or above the row's length holds no point; a voting entry at slot q means GetIndexInKeyFrame == q.
#pragma once

#include <algorithm>
#include <climits>
#include <vector>

#include "sim3opt_ref.hpp"

namespace computesim3_ref {

constexpr int32_t kNoVote = 1 << 30;
constexpr int kThHigh = 100;
enum Status : uint8_t { ST_NO_POINT = 0, ST_MARKED, ST_BAD, ST_DEPTH, ST_OUTSIDE_IMAGE, ST_DISTANCE, ST_LEVEL_RANGE, ST_NO_CANDIDATE, ST_FOUND };

struct Key { float x, y; int32_t octave; };
struct Grid { float minX, minY, invW, invH; int32_t cols, rows; };
struct Pool { const float* pos; const float* minD; const float* maxD; const uint8_t* flags; const uint8_t* desc; int32_t cap; };   // flags bit 0: isBad()
struct KeyFrame {
    const Key* keys; const uint8_t* desc; int32_t n;     // mvKeysUn, mDescriptors, N
    const int32_t* entries; int32_t nEntries;            // GetMapPointMatches() as far as the store holds it
    float bounds[4];                                     // mnMinX, mnMaxX, mnMinY, mnMaxY
    const float* sf; const float* breaks; const float* invSigma2;   // mvScaleFactors, the break table, mvInvLevelSigma2
};
struct Counters {
    int32_t nMarked1, nMarked2, nSharedIdx2, nNull, nBad, nBeyondStride, nDepth, nOutside, nDistLow, nDistHigh, nLevelOut, nNoCandidate,
        nFound12, nFound21, nOneWay, nNew, nEntering, nWalkNull1, nWalkBad, nWalkNoIndex, nNoVoteNew, nRemoved1, nRemoved2, earlyReturn, maxIt10, nNoVoteSearched;
};
struct Result { sim3opt_ref::Result opt; int32_t nFound, nCorr; };

inline int entryOf(const KeyFrame& kf, int q) { return q < kf.nEntries ? kf.entries[q] : -1; }

// mGrid (Frame.cc:236-244, PosInGrid :382-392): per cell the features in ascending index
inline std::vector<std::vector<int> > assignToGrid(const KeyFrame& kf, const Grid& g)
{
    std::vector<std::vector<int> > cells((size_t)g.cols * g.rows);
    for (int i = 0; i < kf.n; i++) {
        const int px = (int)std::round((kf.keys[i].x - g.minX) * g.invW), py = (int)std::round((kf.keys[i].y - g.minY) * g.invH);
        if (px < 0 || px >= g.cols || py < 0 || py >= g.rows) continue;
        cells[(size_t)px * g.rows + py].push_back(i);
    }
    return cells;
}

// KeyFrame::GetFeaturesInArea (KeyFrame.cc:623-662)
inline void featuresInArea(const KeyFrame& kf, const Grid& g, const std::vector<std::vector<int> >& cells, float x, float y, float r, std::vector<int>& out)
{
    out.clear();
    const int x0 = std::max(0, (int)std::floor((x - g.minX - r) * g.invW));
    if (x0 >= g.cols) return;
    const int x1 = std::min(g.cols - 1, (int)std::ceil((x - g.minX + r) * g.invW));
    if (x1 < 0) return;
    const int y0 = std::max(0, (int)std::floor((y - g.minY - r) * g.invH));
    if (y0 >= g.rows) return;
    const int y1 = std::min(g.rows - 1, (int)std::ceil((y - g.minY + r) * g.invH));
    if (y1 < 0) return;
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++)
            for (int i : cells[(size_t)ix * g.rows + iy]) {
                const float dx = kf.keys[i].x - x, dy = kf.keys[i].y - y;
                if (std::fabs(dx) < r && std::fabs(dy) < r) out.push_back(i);
            }
}

inline int descriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int k = 0; k < 32; k++) { unsigned v = (unsigned)(a[k] ^ b[k]); while (v) { d += (int)(v & 1u); v >>= 1; } }
    return d;
}

// `A*b + c` of CV_32F 3x3 / 3x1: gemm's small branch (the float products summed left to right, then (float)(t*1.0 + c*1.0))
inline void mulAdd(const float* A, const float* b, const float* c, float* o)
{
    for (int i = 0; i < 3; i++) {
        const float t = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2];
        o[i] = (float)((double)t * 1.0 + (double)c[i] * 1.0);
    }
}

// PredictScale (MapPoint.cc:385-394) as the break table restates it: the number of breaks below the ratio, less one
inline int predictLevel(float maxDistance, float dist, const float* breaks, int nlevels)
{
    const float ratio = maxDistance / dist;
    int c = 0;
    for (int j = 0; j <= nlevels; j++) c += ratio > breaks[j] ? 1 : 0;
    return c - 1;
}

// one pass (m:1150-1227 with from = pKF1, to = pKF2; m:1230-1307 the mirror): vnMatch[i] per feature of `from`, status[i]
inline void searchPass(const Pool& pool, const KeyFrame& from, const float* Rfw, const float* tfw, const KeyFrame& to, const Grid& grid, const float* sR,
                       const float* t, const float* K1, const std::vector<uint8_t>& already, float th, int nlevels, int32_t* vnMatch, uint8_t* status,
                       Counters& br, int32_t& nFoundPass)
{
    const std::vector<std::vector<int> > cells = assignToGrid(to, grid);
    std::vector<int> vIndices;
    for (int i = 0; i < from.n; i++) {
        vnMatch[i] = -1;
        status[i] = ST_NO_POINT;
        const int e = entryOf(from, i);
        if (i >= from.nEntries) br.nBeyondStride++;
        const int id = e & ~kNoVote;
        if (e < 0 || id >= pool.cap) { if (i < from.nEntries) br.nNull++; continue; }   // m:1154 !pMP
        status[i] = ST_MARKED;
        if (already[(size_t)i]) continue;                                               // m:1154
        status[i] = ST_BAD;
        if (pool.flags[id] & 1) { br.nBad++; continue; }                                // m:1157
        if (e & kNoVote) br.nNoVoteSearched++;
        float pf[3], pt[3];
        mulAdd(Rfw, pool.pos + 3 * (size_t)id, tfw, pf);                                // m:1161
        mulAdd(sR, pf, t, pt);                                                          // m:1162
        status[i] = ST_DEPTH;
        if (pt[2] < 0.0) { br.nDepth++; continue; }                                     // m:1165
        const float invz = (float)(1.0 / (double)pt[2]);
        const float x = pt[0] * invz, y = pt[1] * invz;
        const float u = K1[0] * x + K1[2], v = K1[1] * y + K1[3];
        status[i] = ST_OUTSIDE_IMAGE;
        if (!(u >= to.bounds[0] && u < to.bounds[1] && v >= to.bounds[2] && v < to.bounds[3])) { br.nOutside++; continue; }   // m:1176
        const float maxDistance = 1.2f * pool.maxD[id], minDistance = 0.8f * pool.minD[id];
        const float dist3D = (float)std::sqrt((double)pt[0] * (double)pt[0] + (double)pt[1] * (double)pt[1] + (double)pt[2] * (double)pt[2]);
        status[i] = ST_DISTANCE;
        if (dist3D < minDistance) { br.nDistLow++; continue; }                          // m:1184
        if (dist3D > maxDistance) { br.nDistHigh++; continue; }
        const int level = predictLevel(pool.maxD[id], dist3D, to.breaks, nlevels);       // m:1188
        status[i] = ST_LEVEL_RANGE;
        if (level < 0 || level >= nlevels) { br.nLevelOut++; continue; }
        const float radius = th * to.sf[level];                                         // m:1191
        featuresInArea(to, grid, cells, u, v, radius, vIndices);
        int bestDist = INT_MAX, bestIdx = -1;
        for (int idx : vIndices) {
            if (to.keys[idx].octave < level - 1 || to.keys[idx].octave > level) continue;   // m:1209
            const int dist = descriptorDistance(pool.desc + 32 * (size_t)id, to.desc + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        status[i] = ST_NO_CANDIDATE;
        if (bestDist <= kThHigh) { vnMatch[i] = bestIdx; status[i] = ST_FOUND; nFoundPass++; } else br.nNoCandidate++;   // m:1223
    }
}

// The whole chain of one job.  m12Id / m12Idx2: the entering vpMatches12 (n1 each; null: none).  Out: res; matchOut / idsOut [n1];
// removed [n1]: sim3opt_ref's byte per correspondence, zero behind nCorr; status and vn [n1 + n2]: pass 1->2's first.
inline void computeSim3(const Pool& pool, const KeyFrame& kf1, const KeyFrame& kf2, const Grid& grid, const sim3opt_ref::Problem& prob, const float* R12,
                        const float* t12, float s12, float th, int nlevels, const int32_t* m12Id, const int32_t* m12Idx2, Result& res, int32_t* matchOut,
                        int32_t* idsOut, uint8_t* removed, uint8_t* status, int32_t* vn, Counters& br)
{
    const int n1 = kf1.n, n2 = kf2.n;
    // m:1121-1123: sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12
    float sR12[9], sR21[9], t21[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            sR12[3 * r + c] = (float)((double)R12[3 * r + c] * (double)s12);
            sR21[3 * r + c] = (float)((double)R12[3 * c + r] * (1.0 / s12));
        }
    for (int r = 0; r < 3; r++) {
        const float m = sR21[3 * r] * t12[0] + sR21[3 * r + 1] * t12[1] + sR21[3 * r + 2] * t12[2];
        t21[r] = (float)((double)m * -1.0);
    }
    // m:1131-1144
    std::vector<uint8_t> already1((size_t)n1, 0), already2((size_t)n2, 0);
    for (int i = 0; i < n1; i++) {
        if (!m12Id || m12Id[i] < 0) continue;
        already1[(size_t)i] = 1;
        br.nMarked1++;
        const int idx2 = m12Idx2[i];
        if (idx2 >= 0 && idx2 < n2) {
            if (already2[(size_t)idx2]) br.nSharedIdx2++; else br.nMarked2++;
            already2[(size_t)idx2] = 1;
        }
    }
    int32_t* vn1 = vn;
    int32_t* vn2 = vn + n1;
    searchPass(pool, kf1, prob.R1w, prob.t1w, kf2, grid, sR21, t21, prob.K1, already1, th, nlevels, vn1, status, br, br.nFound12);
    searchPass(pool, kf2, prob.R2w, prob.t2w, kf1, grid, sR12, t12, prob.K1, already2, th, nlevels, vn2, status + n1, br, br.nFound21);
    // m:1309-1325 and the table OptimizeSim3 walks: per i the point of pKF2 (its pool id), and its index in pKF2
    std::vector<int32_t> match((size_t)n1, -1), id2((size_t)n1, -1), idx2Of((size_t)n1, -1);
    res.nFound = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        if (m12Id && m12Id[i1] >= 0) { match[(size_t)i1] = m12Idx2[i1]; id2[(size_t)i1] = m12Id[i1]; idx2Of[(size_t)i1] = m12Idx2[i1]; br.nEntering++; }
        const int idx2 = vn1[i1];
        if (idx2 < 0) continue;
        if (vn2[idx2] != i1) { br.nOneWay++; continue; }
        const int e2 = entryOf(kf2, idx2);
        match[(size_t)i1] = idx2; id2[(size_t)i1] = e2 & ~kNoVote;
        idx2Of[(size_t)i1] = (e2 & kNoVote) ? -1 : idx2;    // GetIndexInKeyFrame(pKF2): the observations do not list pKF2
        if (e2 & kNoVote) br.nNoVoteNew++;
        res.nFound++; br.nNew++;
    }
    // o:1401-1481
    std::vector<sim3opt_ref::Corr> corrs;
    std::vector<int> corrFeat;
    for (int i = 0; i < n1; i++) {
        if (id2[(size_t)i] < 0) continue;                                           // o:1403 !vpMatches1[i]
        const int e1 = entryOf(kf1, i);
        const int id1 = e1 & ~kNoVote;
        if (e1 < 0 || id1 >= pool.cap) { br.nWalkNull1++; continue; }               // o:1414 pMP1
        const int i2 = idx2Of[(size_t)i];
        if ((pool.flags[id1] & 1) || (pool.flags[id2[(size_t)i]] & 1)) { br.nWalkBad++; continue; }   // o:1416
        if (i2 < 0) { br.nWalkNoIndex++; continue; }
        sim3opt_ref::Corr c;
        c.obs1[0] = kf1.keys[i].x; c.obs1[1] = kf1.keys[i].y; c.invSigma2_1 = kf1.invSigma2[kf1.keys[i].octave];
        c.obs2[0] = kf2.keys[i2].x; c.obs2[1] = kf2.keys[i2].y; c.invSigma2_2 = kf2.invSigma2[kf2.keys[i2].octave];
        for (int k = 0; k < 3; k++) { c.X1w[k] = pool.pos[3 * (size_t)id1 + k]; c.X2w[k] = pool.pos[3 * (size_t)id2[(size_t)i] + k]; }
        corrs.push_back(c);
        corrFeat.push_back(i);
    }
    const int nCorr = (int)corrs.size();
    res.nCorr = nCorr;
    for (int i = 0; i < n1; i++) removed[i] = 0;
    std::vector<uint8_t> rem((size_t)std::max(nCorr, 1), 0);
    sim3opt_ref::optimizeSim3<sim3opt_ref::Defined>(prob, corrs.data(), nCorr, res.opt, rem.data(), nullptr, true);   // o:1484-1541
    for (int i = 0; i < n1; i++) { matchOut[i] = match[(size_t)i]; idsOut[i] = id2[(size_t)i]; }
    for (int c = 0; c < nCorr; c++) {
        removed[c] = rem[(size_t)c];
        if (rem[(size_t)c]) { matchOut[corrFeat[(size_t)c]] = -1; idsOut[corrFeat[(size_t)c]] = -1; }   // o:1497, o:1532
        if (rem[(size_t)c] == 1) br.nRemoved1++;
        if (rem[(size_t)c] == 2) br.nRemoved2++;
    }
    if (!res.opt.written) br.earlyReturn++;
    if (res.opt.written && res.opt.nBad > 0) br.maxIt10++;
}

// LoopClosing.cc:333 if(nInliers>=20)
inline bool verdict(int nInliers) { return nInliers >= 20; }

}  // namespace computesim3_ref
