// Test infrastructure: what Tracking::TrackLocalMap and the tail of Tracking::TrackWithMotionModel touch, for
// iORB_SLAM::TrackLocalMapT / TrackWithMotionModelT (include/Tracking_hip.hpp): mock_tracking.hpp's Frame and MapPoint (the pose
// split, the grid, isInFrustum) with the members those lack -- the MapPoint's observations, found counter and UpdateLocalMap's stamp;
// a KeyFrame as UpdateLocalMap sees it (mock_localmap_update.hpp's, over this MapPoint); the Frame's mTcw, mvbOutlier,
// mvInvLevelSigma2, mpReferenceKF and SetPose with UpdatePoseMatrices (Frame.cc:252-267).  Plain data holders: nothing here
// computes what the product computes.
#pragma once

#include <map>
#include <set>
#include <vector>

#include "mock_tracking.hpp"

namespace qmock {

using mock::KeyPoint;
using mock::Mat;

struct KeyFrame;

struct MapPoint : tmock::MapPoint {
    std::map<KeyFrame*, size_t> mObservations;
    long unsigned int mnTrackReferenceForFrame = 0;

    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    int Observations() { return (int)mObservations.size(); }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    void IncreaseFound(int n) { mnFound += n; }
};

struct KeyFrame {
    long unsigned int mnId = 0;
    bool mbBad = false;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame*> mspChildrens;
    KeyFrame* mpParent = nullptr;
    long unsigned int mnTrackReferenceForFrame = 0;

    bool isBad() { return mbBad; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N)   // KeyFrame.cc:181-189
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::set<KeyFrame*> GetChilds() { return mspChildrens; }
    KeyFrame* GetParent() { return mpParent; }
};

// (tmock::Frame's own mvpMapPoints, a vector of its MapPoint, is hidden by this one and stays empty: none of its members reads it)
struct Frame : tmock::Frame {
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvInvLevelSigma2;
    Mat mTcw = Mat::f32(4, 4);
    KeyFrame* mpReferenceKF = nullptr;
    int setPoseCalls = 0;

    void SetPose(Mat Tcw) { mTcw = Tcw.clone(); UpdatePoseMatrices(); setPoseCalls++; }   // Frame.cc:252-256
    void UpdatePoseMatrices()   // Frame.cc:258-267: mRcw, mtcw, mOw = -mRcw.t()*mtcw (a float product, accumulated in double as gemm does)
    {
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) mRcw.at<float>(r, c) = mTcw.at<float>(r, c); mtcw.at<float>(r) = mTcw.at<float>(r, 3); }
        for (int r = 0; r < 3; r++) {
            double s = 0;
            for (int c = 0; c < 3; c++) s += (double)mRcw.at<float>(c, r) * (double)mtcw.at<float>(c);
            mOw.at<float>(r) = -(float)s;
        }
    }
};

}  // namespace qmock
