// correct_ref.hpp -- the correction of LoopClosing::CorrectLoop (src/LoopClosing.cc:440-524; MultiMapper::UpdatePosesAndAdd,
// src/MultiMapper.cc:512-595, is the same loop over pMap->GetAllKeyFrames()), monocular, restated serially over the arrays of a
// keyframe store and its map-point pool (the correction block of the C ABI).  Plain C++11, no project header: the
// side the device kernels are held to, byte for byte.  Build with -ffp-contract=off: every operation below is one IEEE operation.
// Line numbers are LoopClosing.cc's unless a file is named.
//
// The arrays are refresh_ref.hpp's (entries, keyframe flags, octaves, centres; the pool's fields), here WRITABLE: the loop runs
// in the reference's order and overwrites positions, normals, bounds and camera centres as it goes, so what a later
// UpdateNormalAndDepth reads is whatever the sequence left there -- the mixture of old and new centres is not coded as a rule.
// KeyFrameAndPose is a map<KeyFrame*, g2o::Sim3> in heap-address order; the order is DEFINED as ascending slot, so the map below
// is keyed by slot.  mnId of a keyframe is its slot.  Eigen's quaternion pieces and g2o's Sim3 are sim3opt_ref.hpp's,
// OpenCV's gemm element cv_ref.hpp's, MapPoint::UpdateNormalAndDepth refresh_ref.hpp's.
#pragma once

#include <map>

#include "cv_ref.hpp"
#include "refresh_ref.hpp"
#include "sim3opt_ref.hpp"

namespace correct_ref {

typedef sim3opt_ref::Sim3 Sim3;

// the world the loop runs in: refresh_ref::Store's arrays, the ones the loop writes held through writable pointers
struct World {
    int kfcap, stride;
    const int32_t* entries;
    const uint8_t* kfFlags;
    const uint8_t* octaves;
    float* centres;          // GetCameraCenter() per slot: SetPose overwrites
    int poolCap;
    float* pos;              // SetWorldPos overwrites
    float* normal;           // UpdateNormalAndDepth overwrites
    float* minD;
    float* maxD;
    const uint8_t* ptFlags;
    const int32_t* refKf;    // mpRefKF per pool id as a slot, -1 none
};

// OrbeKeyFrame's and OrbePoint's layouts
struct KeyFrameOut {
    double corrected[8], nonCorrected[8];   // q x y z w, t, s
    float Tiw[12], Ow[3];
    int32_t nPoints;
};
struct PointOut {
    int32_t id, ownerSlot, ownerIdx;
    float pos[3], normal[3], minDistance, maxDistance;
    int32_t nObs;
    uint8_t status, pad[3];
};

// which branches ran, for the tests that must see each one
struct Branches {
    int anchorKf, otherKf, anchorFirst, anchorLast, anchorMiddle, singleKf, scaleOne, scaleOther;
    int nullEntry, emptyRow, badPoint, skippedPoint, againInOwnersRow, againInLaterKf, moved, movedThroughNoVote;
    int obsReposed, obsPending, obsOwner, obsUnlisted, refReposed, refPending, refOwner, refUnlisted, refNone;
    int noObservation, noRef, levelRange, done;
};
const int kBranchInts = 29;

inline void toArray(const Sim3& S, double* o) { for (int k = 0; k < 4; k++) o[k] = S.q[k]; for (int k = 0; k < 3; k++) o[4 + k] = S.t[k]; o[7] = S.s; }

// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of a float pose's rows [R | t] (:464-466, :472-474;
// src/Converter.cc:110-135 widen, g2o:types/sim3.h:64-67 Quaterniond(R))
inline Sim3 sim3OfPose(const float* T)
{
    double R[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
    Sim3 S;
    poseopt_ref::quatFromMatrix(R, S.q);
    for (int i = 0; i < 3; i++) S.t[i] = (double)T[4 * i + 3];
    S.s = 1.0;
    return S;
}

// KeyFrame::SetPose (src/KeyFrame.cc:99-106) of a pose's rows: Rwc = Rcw.t() (:101), Ow = -Rwc*tcw (:102: gemm with alpha = -1),
// Twc = [Rwc | Ow] (:104-106) as four rows
inline void setPose(const float* T, float* Twc, float* Ow)
{
    float Rwc[9];
    const float tcw[3] = {T[3], T[7], T[11]};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rwc[3 * i + j] = T[4 * j + i];
    for (int i = 0; i < 3; i++) Ow[i] = cv_ref::gemmElem(Rwc + 3 * i, tcw, 1, -1.0, 0.f, 0.0);
    if (!Twc) return;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Twc[4 * i + j] = Rwc[3 * i + j]; Twc[4 * i + 3] = Ow[i]; }
    Twc[12] = 0.f; Twc[13] = 0.f; Twc[14] = 0.f; Twc[15] = 1.f;
}

// one element of a 4x4 CV_32F product (matmul.cpp's small-matrix branch, len == 4): four float products summed left to right,
// then (float)(t*1. + 0*0.)
inline float gemmElem4(const float* a, const float* b, int bstep)
{
    const float t = a[0] * b[0] + a[1] * b[bstep] + a[2] * b[2 * bstep] + a[3] * b[3 * bstep];
    return (float)((double)t * 1.0 + (double)0.f * 0.0);
}

struct Args {
    int K;
    const int32_t* slots;    // mvpCurrentConnectedKFs as slots, in the caller's order
    const float* Tiw;        // GetPose() of each, rows [R | t]
    int anchor;              // the position of mpCurrentKF in slots
    const double* Scw;       // mg2oScw: q x y z w, t, s
    const int32_t* skip;     // the points whose mnCorrectedByKF is already mpCurrentKF->mnId
    int nSkip;
    const float* sf;         // mvScaleFactors
    int nlevels;
};

inline refresh_ref::Store viewOf(const World& w)
{
    refresh_ref::Store st;
    st.kfcap = w.kfcap; st.stride = w.stride; st.entries = w.entries; st.kfFlags = w.kfFlags; st.octaves = w.octaves; st.desc = 0; st.centres = w.centres;
    st.poolCap = w.poolCap; st.pos = w.pos; st.normal = w.normal; st.minD = w.minD; st.maxD = w.maxD; st.ptDesc = 0; st.ptFlags = w.ptFlags;
    return st;
}

// :440-524.  obs: MapPoint::mObservations of every point, refresh_ref::Observations(viewOf(w)).  outKf[K] in the caller's order,
// outPts in visiting order (room for every pool id); returns the count of moved points
inline int correctLoop(World& w, const refresh_ref::Observations& obs, const Args& a, KeyFrameOut* outKf, PointOut* outPts, Branches* brp)
{
    Branches none = Branches();
    Branches& br = brp ? *brp : none;
    const refresh_ref::Store st = viewOf(w);
    const int32_t currentId = a.slots[a.anchor];                    // mpCurrentKF->mnId
    std::vector<int32_t> correctedBy((size_t)w.poolCap, -1), correctedRef((size_t)w.poolCap, -1);   // mnCorrectedByKF, mnCorrectedReference
    std::vector<uint8_t> movedNow((size_t)w.poolCap, 0);
    for (int i = 0; i < a.nSkip; i++) correctedBy[(size_t)a.skip[i]] = currentId;
    std::vector<int> listed((size_t)w.kfcap, -1);                   // (for the counters alone) slot -> position in slots
    std::vector<uint8_t> reposed((size_t)w.kfcap, 0);               // (for the counters alone) SetPose has run
    for (int i = 0; i < a.K; i++) listed[(size_t)a.slots[i]] = i;
    Sim3 Scw;
    for (int k = 0; k < 4; k++) Scw.q[k] = a.Scw[k];
    for (int k = 0; k < 3; k++) Scw.t[k] = a.Scw[4 + k];
    Scw.s = a.Scw[7];
    if (Scw.s == 1.0) br.scaleOne++; else br.scaleOther++;
    if (a.K == 1) br.singleKf++;

    std::map<int32_t, Sim3> CorrectedSim3, NonCorrectedSim3;        // :444
    CorrectedSim3[currentId] = Scw;                                 // :445
    float Twc[16], OwUnused[3];
    setPose(a.Tiw + 12 * (size_t)a.anchor, Twc, OwUnused);          // :446 GetPoseInverse(): what SetPose left in Twc
    for (int i = 0; i < a.K; i++) {                                 // :455
        const int32_t pKFi = a.slots[i];                            // :457
        const float* Tiw = a.Tiw + 12 * (size_t)i;                  // :459
        if (i != a.anchor) {                                        // :461
            br.otherKf++;
            float Tic[12];                                          // :463 Tiw*Twc: the three rows that are read
            for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) Tic[4 * r + c] = gemmElem4(Tiw + 4 * r, Twc + c, 4);
            const Sim3 g2oSic = sim3OfPose(Tic);                    // :464-466
            CorrectedSim3[pKFi] = sim3opt_ref::sim3Mul(g2oSic, Scw);   // :467-469
        } else br.anchorKf++;
        NonCorrectedSim3[pKFi] = sim3OfPose(Tiw);                   // :472-476
    }

    int nPts = 0, position = 0;
    for (std::map<int32_t, Sim3>::iterator mit = CorrectedSim3.begin(); mit != CorrectedSim3.end(); ++mit, ++position) {   // :480
        const int32_t pKFi = mit->first;                            // :482
        const Sim3 g2oCorrectedSiw = mit->second;                   // :483
        const Sim3 g2oCorrectedSwi = sim3opt_ref::sim3Inverse(g2oCorrectedSiw);   // :484
        const Sim3 g2oSiw = NonCorrectedSim3[pKFi];                 // :486
        KeyFrameOut& ko = outKf[listed[(size_t)pKFi]];
        if (pKFi == currentId) { if (position == 0) br.anchorFirst++; if (position == a.K - 1) br.anchorLast++; if (position > 0 && position < a.K - 1) br.anchorMiddle++; }
        int owned = 0, held = 0;
        for (int iMP = 0; iMP < w.stride; iMP++) {                  // :488-489 GetMapPointMatches()
            const int32_t e = w.entries[(size_t)pKFi * w.stride + iMP];
            if (e < 0) { br.nullEntry++; continue; }                // :492
            held++;
            const int32_t pMPi = e & ~refresh_ref::kNoVote;
            if (w.ptFlags[pMPi] & 1) { br.badPoint++; continue; }   // :494
            if (correctedBy[(size_t)pMPi] == currentId) {           // :496
                if (!movedNow[(size_t)pMPi]) br.skippedPoint++;
                else if (correctedRef[(size_t)pMPi] == pKFi) br.againInOwnersRow++;
                else br.againInLaterKf++;
                continue;
            }
            float* P = w.pos + 3 * (size_t)pMPi;
            const double eigP3Dw[3] = {(double)P[0], (double)P[1], (double)P[2]};   // :500-501
            double m[3], c[3];
            sim3opt_ref::sim3Map(g2oSiw, eigP3Dw, m);               // :502
            sim3opt_ref::sim3Map(g2oCorrectedSwi, m, c);
            for (int k = 0; k < 3; k++) P[k] = (float)c[k];         // :504-505 toCvMat narrows, SetWorldPos
            correctedBy[(size_t)pMPi] = currentId;                  // :506
            correctedRef[(size_t)pMPi] = pKFi;                      // :507
            movedNow[(size_t)pMPi] = 1;
            br.moved++;
            if (e & refresh_ref::kNoVote) br.movedThroughNoVote++;
            // (the counters: where each observer and the reference keyframe stand in the sequence)
            for (int32_t o = obs.start[(size_t)pMPi]; o < obs.start[(size_t)pMPi + 1]; o++) {
                const int32_t k = obs.kf[(size_t)o];
                if (listed[(size_t)k] < 0) br.obsUnlisted++; else if (k == pKFi) br.obsOwner++; else if (reposed[(size_t)k]) br.obsReposed++; else br.obsPending++;
            }
            const int32_t ref = w.refKf[pMPi];
            if (ref < 0) br.refNone++; else if (listed[(size_t)ref] < 0) br.refUnlisted++; else if (ref == pKFi) br.refOwner++; else if (reposed[(size_t)ref]) br.refReposed++; else br.refPending++;
            refresh_ref::Point t;                                   // :508 UpdateNormalAndDepth()
            std::memset(&t, 0, sizeof t);
            refresh_ref::Branches rb = refresh_ref::Branches();
            const int status = refresh_ref::updateNormalAndDepth(st, obs, pMPi, ref, P, a.sf, a.nlevels, t, rb);
            br.noObservation += rb.noObservation; br.noRef += rb.noRef; br.levelRange += rb.levelRange;
            if (status == refresh_ref::ST_DONE) {
                br.done++;
                for (int k = 0; k < 3; k++) w.normal[3 * (size_t)pMPi + k] = t.normal[k];
                w.minD[pMPi] = t.minDistance; w.maxD[pMPi] = t.maxDistance;
            }
            PointOut& po = outPts[nPts++];
            std::memset(&po, 0, sizeof po);
            po.id = pMPi; po.ownerSlot = pKFi; po.ownerIdx = iMP;
            for (int k = 0; k < 3; k++) { po.pos[k] = P[k]; po.normal[k] = w.normal[3 * (size_t)pMPi + k]; }
            po.minDistance = w.minD[pMPi]; po.maxDistance = w.maxD[pMPi];
            po.nObs = obs.start[(size_t)pMPi + 1] - obs.start[(size_t)pMPi];
            po.status = (uint8_t)status;
            owned++;
        }
        if (!held) br.emptyRow++;
        double eigR[9];                                             // :512 rotation().toRotationMatrix()
        poseopt_ref::quatToMatrix(g2oCorrectedSiw.q, eigR);
        double eigt[3] = {g2oCorrectedSiw.t[0], g2oCorrectedSiw.t[1], g2oCorrectedSiw.t[2]};   // :513
        const double s = g2oCorrectedSiw.s;                         // :514
        const double f = 1. / s;
        for (int k = 0; k < 3; k++) eigt[k] = eigt[k] * f;          // :516
        float correctedTiw[12];                                     // :518 Converter::toCvSE3 (src/Converter.cc:92-108) narrows
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) correctedTiw[4 * r + c] = (float)eigR[3 * r + c]; correctedTiw[4 * r + 3] = (float)eigt[r]; }
        float Ow[3];
        setPose(correctedTiw, 0, Ow);                               // :520
        for (int k = 0; k < 3; k++) w.centres[3 * (size_t)pKFi + k] = Ow[k];
        reposed[(size_t)pKFi] = 1;
        toArray(g2oCorrectedSiw, ko.corrected); toArray(g2oSiw, ko.nonCorrected);
        std::memcpy(ko.Tiw, correctedTiw, sizeof correctedTiw);
        for (int k = 0; k < 3; k++) ko.Ow[k] = Ow[k];
        ko.nPoints = owned;
    }                                                               // (:523 UpdateConnections reads no pose: the caller's)
    return nPts;
}

}  // namespace correct_ref
