// Test infrastructure: Tracking::TrackWithMotionModel (src/Tracking.cc:917-978, monocular, behind UpdateLastFrame) and
// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1332-1472) written serially over mock types
// (mock_trackpose.hpp's Frame and MapPoint), for the program that holds iORB_SLAM::TrackWithMotionModelT::Run to them
// (motionmodel_dropin_gpu.cpp).  The program's reference Tracking derives from MotionModelLoopsT and supplies PoseOptimization.
// Plain reference-shaped code: nothing here computes what the product computes.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "mock_slam.hpp"

namespace refmotion {

using mock::Mat;
using std::vector;

static const int TH_HIGH = 100, HISTO_LENGTH = 30;

inline int descriptorDistance(const Mat& a, const unsigned char* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a.ptr<unsigned char>(0)[i] ^ b[i]));
    return d;
}

// A*B for 4 x 4 float matrices as cv::gemm's small branch computes it: float products summed left to right, then the double alpha
inline Mat mul44(const Mat& A, const Mat& B)
{
    Mat D = Mat::f32(4, 4);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const float s = A.at<float>(r, 0) * B.at<float>(0, c) + A.at<float>(r, 1) * B.at<float>(1, c) + A.at<float>(r, 2) * B.at<float>(2, c) + A.at<float>(r, 3) * B.at<float>(3, c);
            D.at<float>(r, c) = (float)((double)s * 1.0);
        }
    return D;
}

inline void computeThreeMaxima(vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3)   // ORBmatcher.cc:1603-1644
{
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
}

template <class Frame, class MapPoint>
struct MotionModelLoopsT {
    Frame mCurrentFrame, mLastFrame;
    Mat mVelocity = Mat::f32(4, 4);
    bool mbOnlyTracking = false, mbVO = false;
    int nmatchesAtReturn = 0, nmatchesMapAtReturn = 0;

    // ORBmatcher.cc:1332-1472 with bMono = true: no bForward / bBackward, no right coordinate
    static int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, bool mbCheckOrientation)
    {
        int nmatches = 0;
        vector<int> rotHist[HISTO_LENGTH];
        const float factor = 1.0f / HISTO_LENGTH;
        const Mat& T = CurrentFrame.mTcw;
        for (int i = 0; i < LastFrame.N; i++) {
            MapPoint* pMP = LastFrame.mvpMapPoints[i];
            if (!pMP) continue;
            if (LastFrame.mvbOutlier[i]) continue;
            Mat x3Dw = pMP->GetWorldPos();
            float x3Dc[3];
            for (int k = 0; k < 3; k++) {   // Rcw*x3Dw+tcw
                const float t = T.at<float>(k, 0) * x3Dw.at<float>(0) + T.at<float>(k, 1) * x3Dw.at<float>(1) + T.at<float>(k, 2) * x3Dw.at<float>(2);
                x3Dc[k] = (float)((double)t * 1.0 + (double)T.at<float>(k, 3) * 1.0);
            }
            const float xc = x3Dc[0], yc = x3Dc[1];
            const float invzc = 1.0 / x3Dc[2];
            if (invzc < 0) continue;
            float u = Frame::fx * xc * invzc + Frame::cx;
            float v = Frame::fy * yc * invzc + Frame::cy;
            if (u < Frame::mnMinX || u > Frame::mnMaxX) continue;
            if (v < Frame::mnMinY || v > Frame::mnMaxY) continue;
            int nLastOctave = LastFrame.mvKeysUn[i].octave;
            float radius = th * CurrentFrame.mvScaleFactors[nLastOctave];
            vector<size_t> vIndices2 = CurrentFrame.GetFeaturesInArea(u, v, radius, nLastOctave - 1, nLastOctave + 1);
            if (vIndices2.empty()) continue;
            const Mat dMP = pMP->GetDescriptor();
            int bestDist = 256, bestIdx2 = -1;
            for (size_t k = 0; k < vIndices2.size(); k++) {
                const size_t i2 = vIndices2[k];
                if (CurrentFrame.mvpMapPoints[i2])
                    if (CurrentFrame.mvpMapPoints[i2]->Observations() > 0) continue;
                const int dist = descriptorDistance(dMP, CurrentFrame.mDescriptors.template ptr<unsigned char>((int)i2));
                if (dist < bestDist) { bestDist = dist; bestIdx2 = (int)i2; }
            }
            if (bestDist <= TH_HIGH) {
                CurrentFrame.mvpMapPoints[bestIdx2] = pMP;
                nmatches++;
                if (mbCheckOrientation) {
                    float rot = LastFrame.mvKeysUn[i].angle - CurrentFrame.mvKeysUn[bestIdx2].angle;
                    if (rot < 0.0) rot += 360.0f;
                    int bin = round(rot * factor);
                    if (bin == HISTO_LENGTH) bin = 0;
                    rotHist[bin].push_back(bestIdx2);
                }
            }
        }
        if (mbCheckOrientation) {
            int ind1 = -1, ind2 = -1, ind3 = -1;
            computeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
            for (int i = 0; i < HISTO_LENGTH; i++) {
                if (i != ind1 && i != ind2 && i != ind3) {
                    for (size_t j = 0, jend = rotHist[i].size(); j < jend; j++) {
                        CurrentFrame.mvpMapPoints[rotHist[i][j]] = static_cast<MapPoint*>(NULL);
                        nmatches--;
                    }
                }
            }
        }
        return nmatches;
    }

    // Tracking.cc:917-978 behind UpdateLastFrame; PoseOptimization(Frame*) is the deriving program's
    template <class Optimize>
    bool TrackWithMotionModel(Optimize PoseOptimization)
    {
        mCurrentFrame.SetPose(mul44(mVelocity, mLastFrame.mTcw));
        std::fill(mCurrentFrame.mvpMapPoints.begin(), mCurrentFrame.mvpMapPoints.end(), static_cast<MapPoint*>(NULL));
        int th = 15;
        int nmatches = SearchByProjection(mCurrentFrame, mLastFrame, th, true);
        if (nmatches < 20) {
            std::fill(mCurrentFrame.mvpMapPoints.begin(), mCurrentFrame.mvpMapPoints.end(), static_cast<MapPoint*>(NULL));
            nmatches = SearchByProjection(mCurrentFrame, mLastFrame, 2 * th, true);
        }
        nmatchesAtReturn = nmatches; nmatchesMapAtReturn = 0;
        if (nmatches < 20) return false;
        PoseOptimization(&mCurrentFrame);
        int nmatchesMap = 0;
        for (int i = 0; i < mCurrentFrame.N; i++) {
            if (mCurrentFrame.mvpMapPoints[i]) {
                if (mCurrentFrame.mvbOutlier[i]) {
                    MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
                    mCurrentFrame.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
                    mCurrentFrame.mvbOutlier[i] = false;
                    pMP->mbTrackInView = false;
                    pMP->mnLastFrameSeen = mCurrentFrame.mnId;
                    nmatches--;
                } else if (mCurrentFrame.mvpMapPoints[i]->Observations() > 0) nmatchesMap++;
            }
        }
        nmatchesAtReturn = nmatches; nmatchesMapAtReturn = nmatchesMap;
        if (mbOnlyTracking) { mbVO = nmatchesMap < 10; return nmatches > 20; }
        return nmatchesMap >= 10;
    }
};

}  // namespace refmotion
