// reloc_ref.hpp -- the body of Tracking::Relocalization behind PnPsolver::iterate (src/Tracking.cc:1486-1547, `t:LINE`), restated
// serially over flat arrays: the three calls of Optimizer::PoseOptimization (src/Optimizer.cc:302-341 for the
// edge list, `o:LINE`; tools/poseopt_ref.hpp for the solve, the Defined arithmetic the device is held to), the two calls of
// ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1474-1601, `m:LINE`) with
// Frame::GetFeaturesInArea (src/Frame.cc:327-380, `f:LINE`) and ComputeThreeMaxima (m:1603-1644), and the gates between them.
// Plain C++11, no project header but poseopt_ref.hpp: the side the device entry is held to, byte for byte.
// Readings chosen (the entry's header states the same): the cv::Mat expressions as OpenCV's small-matrix branches compute them;
// PredictScale through a break table (the number of breaks below RAW max / dist3D, less one); a level outside [0, nlevels)
// skips the point; a NaN u or v is outside the image; nothing at or above the store's stride, or behind the row's end, holds a
// point; bit 30 of an entry is not part of the id; a feature at or above n takes no part in a search.
//
// The arrays: the pool as pos[3 id], minD[id], maxD[id] (raw mfMinDistance / mfMaxDistance), flags[id] (bit 0 isBad) and
// desc[32 id]; the frame's mvKeysUn as keys[nKeys] with its descriptors, grid and image bounds; the keyframe's match list as
// entries[nEntries] and its keys' angles; ids[n], the pool id of vvpMapPointMatches[i][t] where vbInliers[t], else -1.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>

#include "poseopt_ref.hpp"

namespace reloc_ref {

const int32_t kNoVote = 1 << 30;
const int kHistoLength = 30;                                     // m:39
const uint8_t kKeep = 0xff;
enum Exit { kRejected = 0, kFirst, kWideShort, kSecond, kNarrowShort, kThird };
enum Status { kNotRun = 0, kNoPoint, kBad, kFound, kOutOfImage, kDistance, kLevelRange, kInView };

struct Key { float x, y; int32_t octave; float angle; };
struct Grid { float minX, minY, invW, invH; int32_t cols, rows; };
struct Pool { const float* pos; const float* minD; const float* maxD; const uint8_t* flags; const uint8_t* desc; int32_t cap; };
struct Frame { const Key* keys; const uint8_t* desc; int32_t nKeys; Grid grid; float bounds[4]; };   // bounds: mnMinX, mnMaxX, mnMinY, mnMaxY
struct KeyFrame { const int32_t* entries; int32_t nEntries, stride; const float* angles; int32_t nAngles; };
struct Levels { const float* invSigma2; const float* sf; const float* breaks; int32_t nlevels; };
struct Result {
    poseopt_ref::Result opt[3];
    float Tcw[16];
    int32_t exit, nGood[3], nAdditional[2];
};
// which branches ran, for the tests that must see each one: per exit, per gate (both searches added up), per search outcome
struct Branches {
    int32_t exits[6];
    int32_t below3Edges, secondAbove, secondBelow, thirdSucceeds, thirdFails, nDiscarded1, nDiscarded3, nKeptOutlier2;
    int32_t nNull, nBeyondStride, nBeyondRow, nNoVote, nBad, nFound, nBehindCamera, nOutU, nOutV, nDistLow, nDistHigh, nLevelBelow, nLevelAbove, nInView;
    int32_t nEmptyWindow, nOccupiedSkipped, nNoneFree, nBestAboveDist[2], nBestAtDist[2], nContended, nMatched, nRotPruned, nBeyondN;   // [2]: the wide search, the narrow one
};

// ---------------------------------------------------------------------------------------------------------------------
// Optimizer::PoseOptimization over the frame's point list.  -1: what the device refuses behind its kernel
inline int solve(const Pool& pool, const Frame& F, const Levels& L, const std::vector<int32_t>& list, const float* Tcw, const float* K,
                 poseopt_ref::Result& res, uint8_t* outlierOut)
{
    const int n = (int)list.size();
    std::vector<poseopt_ref::Edge> edges;
    std::vector<int> indexEdge;
    for (int t = 0; t < n; t++) {                                // o:302
        const int32_t id = list[(size_t)t];
        if (id < 0) continue;                                    // o:305 if(pMP)
        if (id >= pool.cap || t >= F.nKeys) return -1;
        const Key& kp = F.keys[t];                               // o:316
        if (kp.octave < 0 || kp.octave >= L.nlevels) return -1;
        poseopt_ref::Edge e;
        e.u = kp.x; e.v = kp.y;                                  // o:317
        e.invSigma2 = L.invSigma2[kp.octave];                    // o:322
        for (int k = 0; k < 3; k++) e.Xw[k] = pool.pos[3 * (size_t)id + k];   // o:333-336
        edges.push_back(e);                                      // o:339
        indexEdge.push_back(t);                                  // o:340
    }
    poseopt_ref::Frame pf;
    std::memcpy(pf.Tcw, Tcw, sizeof pf.Tcw);
    std::memcpy(pf.K, K, sizeof pf.K);
    std::vector<uint8_t> edgeOutlier(edges.size() + 1, 0);
    poseopt_ref::poseOptimization<poseopt_ref::Defined>(pf, edges.data(), (int)edges.size(), res, edgeOutlier.data(), nullptr);
    for (size_t e = 0; e < edges.size(); e++) outlierOut[indexEdge[e]] = edgeOutlier[e];   // o:311, o:410 / :416 mvbOutlier[idx]
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// mGrid (f:236-244, PosInGrid f:382-392): per cell the features in ascending index
inline std::vector<std::vector<int> > assignToGrid(const Frame& F)
{
    const Grid& g = F.grid;
    std::vector<std::vector<int> > cells((size_t)g.cols * g.rows);
    for (int i = 0; i < F.nKeys; i++) {
        const int px = (int)std::round((F.keys[i].x - g.minX) * g.invW), py = (int)std::round((F.keys[i].y - g.minY) * g.invH);
        if (px < 0 || px >= g.cols || py < 0 || py >= g.rows) continue;
        cells[(size_t)px * g.rows + py].push_back(i);
    }
    return cells;
}

// Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (f:327-380)
inline void featuresInArea(const Frame& F, const std::vector<std::vector<int> >& cells, float x, float y, float r, int minLevel, int maxLevel,
                           std::vector<int>& out)
{
    const Grid& g = F.grid;
    out.clear();
    const int x0 = std::max(0, (int)std::floor((x - g.minX - r) * g.invW));          // f:332
    if (x0 >= g.cols) return;
    const int x1 = std::min(g.cols - 1, (int)std::ceil((x - g.minX + r) * g.invW));  // f:336
    if (x1 < 0) return;
    const int y0 = std::max(0, (int)std::floor((y - g.minY - r) * g.invH));          // f:340
    if (y0 >= g.rows) return;
    const int y1 = std::min(g.rows - 1, (int)std::ceil((y - g.minY + r) * g.invH));  // f:344
    if (y1 < 0) return;
    const bool checkLevels = minLevel > 0 || maxLevel >= 0;                          // f:348
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++)
            for (int i : cells[(size_t)ix * g.rows + iy]) {
                const Key& kp = F.keys[i];
                if (checkLevels) {
                    if (kp.octave < minLevel) continue;                              // f:363
                    if (maxLevel >= 0 && kp.octave > maxLevel) continue;             // f:365
                }
                const float dx = kp.x - x, dy = kp.y - y;
                if (std::fabs(dx) < r && std::fabs(dy) < r) out.push_back(i);        // f:372
            }
}

inline int descriptorDistance(const uint8_t* a, const uint8_t* b)                    // m:1649-1665
{
    int d = 0;
    for (int k = 0; k < 32; k++) { unsigned v = (unsigned)(a[k] ^ b[k]); while (v) { d += (int)(v & 1u); v >>= 1; } }
    return d;
}

inline void threeMaxima(const int* histo, int L, int& ind1, int& ind2, int& ind3)    // m:1603-1644
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = histo[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
}

// PredictScale (MapPoint.cc:385-394) as the break table restates it: the number of breaks below the ratio, less one
inline int predictLevel(float maxDistance, float dist, const float* breaks, int nlevels)
{
    const float ratio = maxDistance / dist;
    int c = 0;
    for (int j = 0; j <= nlevels; j++) c += ratio > breaks[j] ? 1 : 0;
    return c - 1;
}

// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (m:1474-1601) on the frame's point list; n: mCurrentFrame.N.
// Returns nmatches, or -1: a row entry with a point whose keyframe key does not exist (refused)
inline int searchByProjection(const Pool& pool, const Frame& F, const KeyFrame& kf, const Levels& L, const float* Tcw, const float* K,
                              const std::set<int32_t>& sFound, float th, int orbDist, int checkOri, std::vector<int32_t>& list, uint8_t* status, Branches& b, int which)
{
    const int n = (int)list.size();
    int nmatches = 0;                                                                // m:1476
    // m:1478-1480: Rcw, tcw, Ow = -Rcw.t()*tcw (GEMM_1_T: double sums in k order, then the scale by -1)
    float Ow[3];
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)Tcw[4 * k + i] * (double)Tcw[4 * k + 3];
        Ow[i] = (float)(s * -1.0);
    }
    std::vector<int> rotHist[kHistoLength];                                          // m:1483
    const float factor = 1.0f / kHistoLength;                                        // m:1486
    const std::vector<std::vector<int> > cells = assignToGrid(F);
    std::vector<int> vIndices2;
    std::vector<uint8_t> takenNow((size_t)std::max(F.nKeys, 1), 0);
    for (int q = kf.stride; q < kf.nEntries; q++) if (kf.entries[q] >= 0) b.nBeyondStride++;
    for (int q = 0; q < kf.stride; q++) {                                            // m:1490
        status[q] = kNoPoint;
        if (q >= kf.nEntries) { b.nBeyondRow++; continue; }
        const int32_t e = kf.entries[q];
        const int32_t id = e & ~kNoVote;
        if (e < 0 || id >= pool.cap) { b.nNull++; continue; }                        // m:1494 if(pMP)
        if (q >= kf.nAngles) return -1;
        if (e & kNoVote) b.nNoVote++;
        status[q] = kBad;
        if (pool.flags[id] & 1) { b.nBad++; continue; }                              // m:1496 !pMP->isBad()
        status[q] = kFound;
        if (sFound.count(id)) { b.nFound++; continue; }                              // m:1496 !sAlreadyFound.count(pMP)
        const float* x3Dw = pool.pos + 3 * (size_t)id;                               // m:1499
        float x3Dc[3];
        for (int i = 0; i < 3; i++) {                                                // m:1500 Rcw*x3Dw+tcw: gemm's small branch
            const float t = Tcw[4 * i] * x3Dw[0] + Tcw[4 * i + 1] * x3Dw[1] + Tcw[4 * i + 2] * x3Dw[2];
            x3Dc[i] = (float)((double)t * 1.0 + (double)Tcw[4 * i + 3] * 1.0);
        }
        const float xc = x3Dc[0], yc = x3Dc[1];                                      // m:1502-1503
        const float invzc = (float)(1.0 / (double)x3Dc[2]);                          // m:1504 (no depth gate)
        const float u = K[0] * xc * invzc + K[2];                                    // m:1506
        const float v = K[1] * yc * invzc + K[3];                                    // m:1507
        status[q] = kOutOfImage;
        if (!(u >= F.bounds[0] && u <= F.bounds[1])) { b.nOutU++; continue; }        // m:1509
        if (!(v >= F.bounds[2] && v <= F.bounds[3])) { b.nOutV++; continue; }        // m:1511
        if (x3Dc[2] < 0.f) b.nBehindCamera++;
        const float PO[3] = {x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]};     // m:1515
        const float dist3D = (float)std::sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);   // m:1516
        const float maxDistance = 1.2f * pool.maxD[id], minDistance = 0.8f * pool.minD[id];   // m:1518-1519
        status[q] = kDistance;
        if (dist3D < minDistance) { b.nDistLow++; continue; }                        // m:1522
        if (dist3D > maxDistance) { b.nDistHigh++; continue; }
        const int level = predictLevel(pool.maxD[id], dist3D, L.breaks, L.nlevels);  // m:1525
        status[q] = kLevelRange;
        if (level < 0) { b.nLevelBelow++; continue; }
        if (level >= L.nlevels) { b.nLevelAbove++; continue; }
        status[q] = kInView;
        b.nInView++;
        const float radius = th * L.sf[level];                                       // m:1528
        featuresInArea(F, cells, u, v, radius, level - 1, level + 1, vIndices2);     // m:1530
        if (vIndices2.empty()) { b.nEmptyWindow++; continue; }                       // m:1532
        const uint8_t* dMP = pool.desc + 32 * (size_t)id;                            // m:1535
        int bestDist = 256, bestIdx2 = -1, bestAny = 256;                            // m:1537-1538
        bool lostToEarlier = false;
        for (int i2 : vIndices2) {                                                   // m:1540
            const int dist = descriptorDistance(dMP, F.desc + 32 * (size_t)i2);      // m:1548
            if (i2 >= n) { b.nBeyondN++; continue; }                                 // (a feature at or above N is none of the frame's)
            if (list[(size_t)i2] >= 0) {                                             // m:1543 if(CurrentFrame.mvpMapPoints[i2]) continue;
                b.nOccupiedSkipped++;
                if (takenNow[(size_t)i2] && dist < bestAny) { bestAny = dist; lostToEarlier = true; }
                continue;
            }
            if (dist < bestAny) { bestAny = dist; lostToEarlier = false; }
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }                 // m:1550
        }
        if (bestDist <= orbDist) {                                                   // m:1557
            if (bestDist == orbDist) b.nBestAtDist[which]++;
            if (lostToEarlier) b.nContended++;
            list[(size_t)bestIdx2] = id;                                             // m:1559
            takenNow[(size_t)bestIdx2] = 1;
            nmatches++;                                                              // m:1560
            b.nMatched++;
            if (checkOri) {                                                          // m:1562
                float rot = kf.angles[q] - F.keys[bestIdx2].angle;                   // m:1564
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round((double)(rot * factor));                   // m:1567
                if (bin == kHistoLength) bin = 0;
                if (bin < 0 || bin >= kHistoLength) return -1;                       // m:1570 assert
                rotHist[bin].push_back(bestIdx2);                                    // m:1571
            }
        } else if (bestIdx2 < 0) b.nNoneFree++;
        else b.nBestAboveDist[which]++;
    }
    if (checkOri) {                                                                  // m:1579
        int histo[kHistoLength], ind1, ind2, ind3;
        for (int i = 0; i < kHistoLength; i++) histo[i] = (int)rotHist[i].size();
        threeMaxima(histo, kHistoLength, ind1, ind2, ind3);                          // m:1585
        for (int i = 0; i < kHistoLength; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;                       // m:1589
            for (int t : rotHist[i]) { list[(size_t)t] = -1; nmatches--; b.nRotPruned++; }   // m:1593-1594
        }
    }
    return nmatches;                                                                 // m:1600
}

// ---------------------------------------------------------------------------------------------------------------------
// t:1486-1547 for one candidate.  status: 2 * stride bytes (the wide search's, then the narrow one's; kNotRun where not reached).
// 0, or -1: an input the device refuses with ORBX_E_INVALID behind its kernels (nothing is written then)
inline int relocalize(const Pool& pool, const Frame& F, const KeyFrame& kf, const Levels& L, const int32_t* ids, int n, const float* Tcw, const float* K,
                      int checkOri, Result& res, int32_t* idsOut, uint8_t* outlierOut, uint8_t* status, Branches& br)
{
    Branches b = br;
    Result r;
    std::memset(&r, 0, sizeof r);
    std::vector<uint8_t> outl((size_t)n + 1, kKeep), st((size_t)2 * std::max(kf.stride, 0) + 1, kNotRun);
    std::vector<int32_t> list((size_t)n, -1);
    std::set<int32_t> sFound;                                                        // t:1488
    for (int t = 0; t < n; t++) {                                                    // t:1492
        list[(size_t)t] = ids[t];                                                    // t:1496 / :1500
        if (ids[t] >= 0) sFound.insert(ids[t]);                                      // t:1497
    }
    std::memcpy(r.Tcw, Tcw, sizeof r.Tcw);                                           // t:1486
    auto leave = [&](int exit) {
        r.exit = exit;
        b.exits[exit]++;
        res = r;
        for (int t = 0; t < n; t++) { idsOut[t] = list[(size_t)t]; outlierOut[t] = outl[(size_t)t]; }
        if (status) std::memcpy(status, st.data(), (size_t)2 * kf.stride);
        br = b;
        return 0;
    };
    auto discard = [&](int32_t& counter) {
        for (int io = 0; io < n; io++)
            if (list[(size_t)io] >= 0 && outl[(size_t)io] == 1) { list[(size_t)io] = -1; counter++; }
    };
    if (solve(pool, F, L, list, r.Tcw, K, r.opt[0], outl.data())) return -1;         // t:1503
    std::memcpy(r.Tcw, r.opt[0].Tcw, sizeof r.Tcw);                                  // o:470 pFrame->SetPose (o:386: not below 3 edges, where opt.Tcw is the pose as it came)
    int nGood = r.opt[0].nGood;
    r.nGood[0] = nGood;
    if (r.opt[0].nInitial < 3) b.below3Edges++;
    if (nGood < 10) return leave(kRejected);                                         // t:1505
    discard(b.nDiscarded1);                                                          // t:1508-1510
    if (!(nGood < 50)) return leave(kFirst);                                         // t:1513
    int nadditional = searchByProjection(pool, F, kf, L, r.Tcw, K, sFound, 10.f, 100, checkOri, list, st.data(), b, 0);   // t:1515
    if (nadditional < 0) return -1;
    r.nAdditional[0] = nadditional;
    if (!(nadditional + nGood >= 50)) return leave(kWideShort);                      // t:1517
    if (solve(pool, F, L, list, r.Tcw, K, r.opt[1], outl.data())) return -1;         // t:1519
    std::memcpy(r.Tcw, r.opt[1].Tcw, sizeof r.Tcw);
    nGood = r.opt[1].nGood;
    r.nGood[1] = nGood;
    for (int t = 0; t < n; t++) if (list[(size_t)t] >= 0 && outl[(size_t)t] == 1) b.nKeptOutlier2++;
    if (!(nGood > 30 && nGood < 50)) {                                               // t:1523
        if (nGood >= 50) b.secondAbove++; else b.secondBelow++;
        return leave(kSecond);
    }
    sFound.clear();                                                                  // t:1525
    for (int ip = 0; ip < n; ip++)
        if (list[(size_t)ip] >= 0) sFound.insert(list[(size_t)ip]);                  // t:1526-1528
    nadditional = searchByProjection(pool, F, kf, L, r.Tcw, K, sFound, 3.f, 64, checkOri, list, st.data() + kf.stride, b, 1);   // t:1529
    if (nadditional < 0) return -1;
    r.nAdditional[1] = nadditional;
    if (!(nGood + nadditional >= 50)) return leave(kNarrowShort);                    // t:1532
    if (solve(pool, F, L, list, r.Tcw, K, r.opt[2], outl.data())) return -1;         // t:1534
    std::memcpy(r.Tcw, r.opt[2].Tcw, sizeof r.Tcw);
    nGood = r.opt[2].nGood;
    r.nGood[2] = nGood;
    discard(b.nDiscarded3);                                                          // t:1536-1538
    if (nGood >= 50) b.thirdSucceeds++; else b.thirdFails++;
    return leave(kThird);
}

// t:1546 if(nGood>=50)
inline int nGoodAtExit(const Result& r) { return r.exit == kThird ? r.nGood[2] : r.exit == kSecond || r.exit == kNarrowShort ? r.nGood[1] : r.nGood[0]; }
inline bool verdict(const Result& r) { return r.exit != kRejected && nGoodAtExit(r) >= 50; }

}  // namespace reloc_ref
