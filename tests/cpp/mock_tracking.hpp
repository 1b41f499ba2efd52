// Test infrastructure: what Tracking::SearchLocalPoints touches, for iORB_SLAM::SearchLocalPointsT (include/Tracking_hip.hpp),
// without OpenCV: a MapPoint with Tracking's per-frame fields and counters, a Frame with its pose split as UpdatePoseMatrices
// leaves it (Frame.cc:258-267), its grid (Frame.cc:230-245, 382-392) and GetFeaturesInArea (Frame.cc:327-380).  Frame::isInFrustum
// is the reference's statement (Frame.cc:269-325) over the mock Mat, with the cv::Mat expressions in tools/frustum_ref.hpp's
// forms.  Plain data holders otherwise: nothing here computes what the product computes.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "mock_slam.hpp"

namespace tmock {

using mock::KeyPoint;
using mock::Mat;

struct MapPoint {
    long mnId = 0;
    int poolId = -1;
    Mat mWorldPos = Mat::f32(3, 1), mNormalVector = Mat::f32(3, 1), mDescriptor = Mat::u8(1, 32);
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
    int nObs = 0, mnVisible = 1, mnFound = 1;
    bool mbBad = false;
    // Tracking's per-frame fields (MapPoint.h:97-102)
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = -1;
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    float mTrackViewCos = 1.f;
    long unsigned int mnLastFrameSeen = 0;

    Mat GetWorldPos() { return mWorldPos.clone(); }
    Mat GetNormal() { return mNormalVector.clone(); }
    Mat GetDescriptor() { return mDescriptor.clone(); }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    void IncreaseVisible(int n) { mnVisible += n; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }   // MapPoint.cc:373-383
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    int PredictScale(const float& currentDist, const float& logScaleFactor)   // MapPoint.cc:385-394
    {
        const float ratio = mfMaxDistance / currentDist;
        return (int)std::ceil(std::log(ratio) / logScaleFactor);
    }
};

struct Frame {
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    Mat mDescriptors;
    std::vector<MapPoint*> mvpMapPoints;
    Mat mRcw = Mat::f32(3, 3), mtcw = Mat::f32(3, 1), mOw = Mat::f32(3, 1);
    std::vector<float> mvScaleFactors;
    float mfLogScaleFactor = 0;
    int mnGridCols = 64, mnGridRows = 48;
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    // process-wide statics in the reference (Frame.cc:29-33)
    static float fx, fy, cx, cy, mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;

    void AssignFeaturesToGrid()   // Frame.cc:230-245, PosInGrid :382-392
    {
        mGrid.assign(mnGridCols, std::vector<std::vector<size_t> >(mnGridRows));
        for (int i = 0; i < N; i++) {
            const float px = std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv), py = std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
            if (!(px >= 0.f && px < (float)mnGridCols && py >= 0.f && py < (float)mnGridRows)) continue;
            mGrid[(int)px][(int)py].push_back(i);
        }
    }
    std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const int minLevel = -1, const int maxLevel = -1) const   // Frame.cc:327-380
    {
        std::vector<size_t> vIndices;
        const int nMinCellX = std::max(0, (int)std::floor((x - mnMinX - r) * mfGridElementWidthInv));
        if (nMinCellX >= mnGridCols) return vIndices;
        const int nMaxCellX = std::min((int)mnGridCols - 1, (int)std::ceil((x - mnMinX + r) * mfGridElementWidthInv));
        if (nMaxCellX < 0) return vIndices;
        const int nMinCellY = std::max(0, (int)std::floor((y - mnMinY - r) * mfGridElementHeightInv));
        if (nMinCellY >= mnGridRows) return vIndices;
        const int nMaxCellY = std::min((int)mnGridRows - 1, (int)std::ceil((y - mnMinY + r) * mfGridElementHeightInv));
        if (nMaxCellY < 0) return vIndices;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t>& vCell = mGrid[ix][iy];
                for (size_t j = 0; j < vCell.size(); j++) {
                    const KeyPoint& kpUn = mvKeysUn[vCell[j]];
                    if (bCheckLevels) {
                        if (kpUn.octave < minLevel) continue;
                        if (maxLevel >= 0) if (kpUn.octave > maxLevel) continue;
                    }
                    const float distx = kpUn.pt.x - x, disty = kpUn.pt.y - y;
                    if (std::fabs(distx) < r && std::fabs(disty) < r) vIndices.push_back(vCell[j]);
                }
            }
        return vIndices;
    }
    bool isInFrustum(MapPoint* pMP, float viewingCosLimit)   // Frame.cc:269-325
    {
        pMP->mbTrackInView = false;
        Mat P = pMP->GetWorldPos();
        float Pc[3];
        for (int i = 0; i < 3; i++) {   // mRcw*P+mtcw: gemm's small-matrix branch with a C
            const float s = mRcw.at<float>(i, 0) * P.at<float>(0) + mRcw.at<float>(i, 1) * P.at<float>(1) + mRcw.at<float>(i, 2) * P.at<float>(2);
            Pc[i] = (float)((double)s * 1.0 + (double)mtcw.at<float>(i) * 1.0);
        }
        const float &PcX = Pc[0], &PcY = Pc[1], &PcZ = Pc[2];
        if (PcZ < 0.0f) return false;
        const float invz = 1.0f / PcZ;
        const float u = fx * PcX * invz + cx;
        const float v = fy * PcY * invz + cy;
        if (u != u || v != v) return false;   // the defined choice of DESIGN.md 8q
        if (u < mnMinX || u > mnMaxX) return false;
        if (v < mnMinY || v > mnMaxY) return false;
        const float maxDistance = pMP->GetMaxDistanceInvariance();
        const float minDistance = pMP->GetMinDistanceInvariance();
        float PO[3];
        double s2 = 0;
        for (int i = 0; i < 3; i++) { PO[i] = P.at<float>(i) - mOw.at<float>(i); s2 += (double)PO[i] * (double)PO[i]; }
        const float dist = (float)std::sqrt(s2);   // cv::norm
        if (dist < minDistance || dist > maxDistance) return false;
        Mat Pn = pMP->GetNormal();
        double dt = 0;
        for (int i = 0; i < 3; i++) dt += (double)PO[i] * (double)Pn.at<float>(i);   // Mat::dot
        const float viewCos = (float)(dt / dist);
        if (viewCos < viewingCosLimit) return false;
        const float lv = std::ceil(std::log(pMP->mfMaxDistance / dist) / mfLogScaleFactor);
        if (!(lv >= 0.f) || !(lv < (float)mvScaleFactors.size())) return false;   // the defined choice of DESIGN.md 8q
        const int nPredictedLevel = pMP->PredictScale(dist, mfLogScaleFactor);
        pMP->mbTrackInView = true;
        pMP->mTrackProjX = u;
        pMP->mTrackProjY = v;
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;
        return true;
    }
};
float Frame::fx = 0, Frame::fy = 0, Frame::cx = 0, Frame::cy = 0, Frame::mnMinX = 0, Frame::mnMaxX = 0, Frame::mnMinY = 0,
      Frame::mnMaxY = 0, Frame::mfGridElementWidthInv = 0, Frame::mfGridElementHeightInv = 0;

}  // namespace tmock
