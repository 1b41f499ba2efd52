// Test infrastructure: what Tracking::UpdateLocalMap touches, for iORB_SLAM::UpdateLocalMapT (include/Tracking_hip.hpp): a
// MapPoint with its observations and Tracking's stamp, a KeyFrame with its match slots, its ordered covisible neighbours, its
// spanning-tree links and Tracking's stamp, a Frame with its MapPoints and reference keyframe.  Plain data holders: nothing here
// computes what the product computes.
#pragma once

#include <cstddef>
#include <map>
#include <set>
#include <vector>

namespace umock {

struct KeyFrame;

struct MapPoint {
    long unsigned int mnId = 0;
    int poolId = -1;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    long unsigned int mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;

    bool isBad() { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
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

struct Frame {
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<MapPoint*> mvpMapPoints;
    KeyFrame* mpReferenceKF = nullptr;
};

}  // namespace umock
