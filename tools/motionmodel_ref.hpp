// motionmodel_ref.hpp -- Tracking::TrackWithMotionModel (src/Tracking.cc:925-969, `t:LINE`, monocular), restated serially over
// flat arrays: the pose product, both calls of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
// (src/ORBmatcher.cc:1332-1472, `m:LINE`) with Frame::GetFeaturesInArea and ComputeThreeMaxima (tools/reloc_ref.hpp's statements
// of them), the retry, the gate, and Optimizer::PoseOptimization with the discard loop behind it (tools/trackpose_ref.hpp over
// tools/poseopt_ref.hpp).  Plain C++11, no project header but those two: the side the device entry is held to, byte for byte.
// Readings chosen (the entry's header states the same): the cv::Mat products as OpenCV's small-matrix branch computes them (float
// products summed left to right, then the double alpha / beta step); 1.0/z in double, narrowed; a NaN u or v is outside the
// image; a last-frame feature at or above the last frame's key count holds no point; a feature at or above n takes no part in a
// search; an octave at or above nlevels has the scale factor 0; the query descriptor of m:1397 is the last frame's own row, as the resident search takes it; nmatches counts a feature
// twice when two points took it one after the other, as the reference's counter does.
//
// The arrays: the pool as pos[3 id] and flags[id] (bit 1 Observations() > 0); the current frame's mvKeysUn as
// cur.keys[cur.nKeys] with its descriptors, grid and image bounds; the last frame's keys (octave, angle) and descriptors;
// lastIds[nq], the pool id of mLastFrame.mvpMapPoints[i], -1 where NULL or mvbOutlier[i].
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "reloc_ref.hpp"
#include "trackpose_ref.hpp"

namespace motionmodel_ref {

using reloc_ref::Frame;
using reloc_ref::Key;
using reloc_ref::kHistoLength;

enum Exit { kTracked = 0, kTooFew = 1 };
// the pool's projection status codes, and the byte of a search that did not run
enum Status { kBad = 0, kDepth, kOutOfImage, kDistance, kViewAngle, kLevelRange, kInView, kNoPoint, kNotRun = 0xff };
const int kThHigh = 100;                                         // m:36 TH_HIGH

struct Pool { const float* pos; const uint8_t* flags; int32_t cap; };
struct Last { const Key* keys; const uint8_t* desc; int32_t nKeys; };
struct Levels { const float* invSigma2; const float* sf; int32_t nlevels; };
struct Result {
    trackpose_ref::Result track;
    float TcwPred[16];
    int32_t nSearch[2], wide, status;
};
// which branches ran, for the tests that must see each one; the gates and the search outcomes are added up over both searches
struct Branches {
    int32_t exits[2], retried;
    int32_t nNoPoint, nBehindCamera, nOutU, nOutV, nInView;
    int32_t nEmptyWindow, nObservedSkipped, nOverwritten, nContended, nNoneFree, nBestAboveDist, nBestAtDist, nMatched, nRotPruned, nBeyondN;
    int32_t nDiscarded;
};

// t:925 mVelocity*mLastFrame.mTcw: gemm's small branch with len 4 and no C
inline void poseProduct(const float* V, const float* T, float* out)
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const float s = V[4 * r] * T[c] + V[4 * r + 1] * T[4 + c] + V[4 * r + 2] * T[8 + c] + V[4 * r + 3] * T[12 + c];
            out[4 * r + c] = (float)((double)s * 1.0);
        }
}

// SearchByProjection(CurrentFrame, LastFrame, th, true) (m:1332-1472) from an all-NULL frame: list[t] the pool id feature t holds,
// assign[t] the last-frame feature it came from.  Returns nmatches, or -1: what the device refuses
inline int searchByProjection(const Pool& pool, const Frame& F, const Last& last, const Levels& L, const int32_t* lastIds, int nq, int n,
                              const float* Tcw, const float* K, float th, int checkOri, std::vector<int32_t>& list, std::vector<int32_t>& assign,
                              uint8_t* status, Branches& b)
{
    int nmatches = 0;                                                                // m:1334
    std::vector<int> rotHist[kHistoLength];                                          // m:1337
    const float factor = 1.0f / kHistoLength;                                        // m:1340
    const std::vector<std::vector<int> > cells = reloc_ref::assignToGrid(F);
    std::vector<int> vIndices2;
    std::vector<uint8_t> takenNow((size_t)(F.nKeys > 0 ? F.nKeys : 1), 0);
    for (int i = 0; i < nq; i++) {                                                   // m:1353
        status[i] = kNoPoint;
        const int32_t id = lastIds[i];
        if (id < 0 || id >= pool.cap || i >= last.nKeys) { b.nNoPoint++; continue; } // m:1357-1359 if(pMP) if(!mvbOutlier[i])
        const float* x3Dw = pool.pos + 3 * (size_t)id;                               // m:1362
        float x3Dc[3];
        for (int k = 0; k < 3; k++) {                                                // m:1363 Rcw*x3Dw+tcw: gemm's small branch
            const float t = Tcw[4 * k] * x3Dw[0] + Tcw[4 * k + 1] * x3Dw[1] + Tcw[4 * k + 2] * x3Dw[2];
            x3Dc[k] = (float)((double)t * 1.0 + (double)Tcw[4 * k + 3] * 1.0);
        }
        const float xc = x3Dc[0], yc = x3Dc[1];                                      // m:1365-1366
        const float invzc = (float)(1.0 / (double)x3Dc[2]);                          // m:1367
        status[i] = kDepth;
        if (invzc < 0) { b.nBehindCamera++; continue; }                              // m:1369
        const float u = K[0] * xc * invzc + K[2];                                    // m:1372
        const float v = K[1] * yc * invzc + K[3];                                    // m:1373
        status[i] = kOutOfImage;
        if (!(u >= F.bounds[0] && u <= F.bounds[1])) { b.nOutU++; continue; }        // m:1375
        if (!(v >= F.bounds[2] && v <= F.bounds[3])) { b.nOutV++; continue; }        // m:1377
        status[i] = kInView;
        b.nInView++;
        const int nLastOctave = last.keys[i].octave;                                 // m:1380
        const float radius = th * (nLastOctave < L.nlevels ? L.sf[nLastOctave < 0 ? 0 : nLastOctave] : 0.f);   // m:1383 (a level the table does not hold has no factor: an empty window)
        reloc_ref::featuresInArea(F, cells, u, v, radius, nLastOctave - 1, nLastOctave + 1, vIndices2);   // m:1392
        if (vIndices2.empty()) { b.nEmptyWindow++; continue; }                       // m:1394
        const uint8_t* dMP = last.desc + 32 * (size_t)i;                             // m:1397 as the resident search reads it: the last frame's own row
        int bestDist = 256, bestIdx2 = -1, bestAny = 256;                            // m:1399-1400
        bool lostToEarlier = false;
        for (int i2 : vIndices2) {                                                   // m:1402
            const int dist = reloc_ref::descriptorDistance(dMP, F.desc + 32 * (size_t)i2);   // m:1419
            if (i2 >= n) { b.nBeyondN++; continue; }                                 // (a feature at or above N is none of the frame's)
            if (list[(size_t)i2] >= 0 && (pool.flags[list[(size_t)i2]] & 2)) {       // m:1405-1407 Observations()>0
                b.nObservedSkipped++;
                if (takenNow[(size_t)i2] && dist < bestAny) { bestAny = dist; lostToEarlier = true; }
                continue;
            }
            if (dist < bestAny) { bestAny = dist; lostToEarlier = false; }
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }                 // m:1421
        }
        if (bestDist <= kThHigh) {                                                   // m:1428
            if (bestDist == kThHigh) b.nBestAtDist++;
            if (lostToEarlier) b.nContended++;
            if (list[(size_t)bestIdx2] >= 0) b.nOverwritten++;
            list[(size_t)bestIdx2] = id;                                             // m:1430
            assign[(size_t)bestIdx2] = i;
            takenNow[(size_t)bestIdx2] = 1;
            nmatches++;                                                              // m:1431
            b.nMatched++;
            if (checkOri) {                                                          // m:1433
                float rot = last.keys[i].angle - F.keys[bestIdx2].angle;             // m:1435
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round((double)(rot * factor));                   // m:1438
                if (bin == kHistoLength) bin = 0;
                if (bin < 0 || bin >= kHistoLength) return -1;                       // m:1441 assert
                rotHist[bin].push_back(bestIdx2);                                    // m:1442
            }
        } else if (bestIdx2 < 0) b.nNoneFree++;
        else b.nBestAboveDist++;
    }
    if (checkOri) {                                                                  // m:1450
        int histo[kHistoLength], ind1, ind2, ind3;
        for (int i = 0; i < kHistoLength; i++) histo[i] = (int)rotHist[i].size();
        reloc_ref::threeMaxima(histo, kHistoLength, ind1, ind2, ind3);               // m:1456
        for (int i = 0; i < kHistoLength; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;                       // m:1460
            for (int t : rotHist[i]) { list[(size_t)t] = -1; assign[(size_t)t] = -1; nmatches--; b.nRotPruned++; }   // m:1464-1465
        }
    }
    return nmatches;                                                                 // m:1471
}

// t:925-969 for one job.  status: 2 * nq bytes (search 1's, then search 2's; kNotRun where it did not run).  0, or -1: an input the
// device refuses with ORBX_E_INVALID behind its kernels (nothing is written then)
inline int trackWithMotionModel(const Pool& pool, const Frame& F, const Last& last, const Levels& L, const int32_t* lastIds, int nq, int n,
                                const float* velocity, const float* lastTcw, const float* K, float th, int minMatches, int checkOri,
                                Result& res, int32_t* idsOut, uint8_t* outlierOut, int32_t* assignOut, uint8_t* status, Branches& br)
{
    Branches b = br;
    Result r;
    std::memset(&r, 0, sizeof r);
    poseProduct(velocity, lastTcw, r.TcwPred);                                       // t:925
    std::vector<uint8_t> st((size_t)2 * (nq > 0 ? nq : 0) + 1, (uint8_t)kNotRun);
    std::vector<int32_t> list((size_t)n, -1), assign((size_t)n, -1);                 // t:927
    int nmatches = searchByProjection(pool, F, last, L, lastIds, nq, n, r.TcwPred, K, th, checkOri, list, assign, st.data(), b);   // t:935
    if (nmatches < 0) return -1;
    r.nSearch[0] = nmatches; r.nSearch[1] = -1;
    if (nmatches < minMatches) {                                                     // t:938
        list.assign((size_t)n, -1); assign.assign((size_t)n, -1);                    // t:940
        nmatches = searchByProjection(pool, F, last, L, lastIds, nq, n, r.TcwPred, K, 2.0f * th, checkOri, list, assign, st.data() + nq, b);   // t:941
        if (nmatches < 0) return -1;
        r.wide = 1; r.nSearch[1] = nmatches;
        b.retried++;
    }
    std::vector<uint8_t> outl((size_t)n + 1, 0);
    std::vector<int32_t> ids(list);
    ids.push_back(-1);
    if (nmatches < minMatches) {                                                     // t:944 return false
        r.status = kTooFew;
        std::memcpy(r.track.opt.Tcw, r.TcwPred, sizeof r.TcwPred);
        r.track.nMatches = nmatches;
    } else {
        // t:948-969: the edge list in ascending feature order, the solve from the predicted pose, the discard loop
        std::vector<trackpose_ref::Key> keys((size_t)n + 1);
        for (int t = 0; t < n; t++) {
            if (list[(size_t)t] >= 0 && t >= F.nKeys) return -1;
            if (t < F.nKeys) { keys[(size_t)t].u = F.keys[t].x; keys[(size_t)t].v = F.keys[t].y; keys[(size_t)t].octave = F.keys[t].octave; }
        }
        trackpose_ref::Job J;
        J.keys = keys.data(); J.assign = nullptr; J.ids = nullptr; J.nq = 0; J.baseIds = list.data(); J.n = n; J.discard = 1;
        std::memcpy(J.frame.Tcw, r.TcwPred, sizeof r.TcwPred);
        std::memcpy(J.frame.K, K, sizeof J.frame.K);
        const trackpose_ref::Pool P = {pool.pos, pool.flags, pool.cap};
        trackpose_ref::Branches tb;
        if (trackpose_ref::trackPose(P, J, L.invSigma2, L.nlevels, r.track, ids.data(), outl.data(), &tb)) return -1;
        b.nDiscarded += tb.nOutlierDiscarded;
        r.status = kTracked;
    }
    b.exits[r.status]++;
    res = r;
    for (int t = 0; t < n; t++) { idsOut[t] = ids[(size_t)t]; outlierOut[t] = outl[(size_t)t]; if (assignOut) assignOut[t] = assign[(size_t)t]; }
    if (status && nq > 0) std::memcpy(status, st.data(), (size_t)2 * nq);
    br = b;
    return 0;
}

}  // namespace motionmodel_ref
