// Test infrastructure: what LocalMapping::CreateNewMapPoints touches beyond tests/cpp/mock_slam.hpp (from which these are
// derived): the covisibility query, the scene's median depth, the scale members of a KeyFrame, a MapPoint that is built from
// a position and a reference keyframe, and a Map.  Plain data holders: nothing here computes what the product computes.
#pragma once

#include <list>

#include "mock_slam.hpp"

namespace lmock {

// the cv::Mat the drop-in builds x3D in
struct Mat {
    int rows = 0, cols = 0;
    std::vector<float> d;
    Mat() {}
    Mat(int r, int c, int /*type*/) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
};

struct Map;

struct KeyFrame : mock::KeyFrame {
    float mfScaleFactor = 1.2f;
    int mnScaleLevels = 8;
    float medianDepth = -1.f;                        // what ComputeSceneMedianDepth(2) returns (KeyFrame.cc:630-661 reads the map)
    std::vector<KeyFrame*> covisible;                // best first
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N)
    {
        return (int)covisible.size() < N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
    }
    float ComputeSceneMedianDepth(const int /*q*/) { return medianDepth; }
};

struct MapPoint : mock::MapPoint {
    KeyFrame* mpRefKF = nullptr;
    Map* mpMap = nullptr;
    int nDistinctive = 0, nUpdateNormal = 0;         // calls of the two members, in the order the replay makes them
    int observationsAtDistinctive = 0;
    MapPoint(const Mat& Pos, KeyFrame* pRefKF, Map* pMap) : mpRefKF(pRefKF), mpMap(pMap)
    {
        for (int r = 0; r < 3; r++) mWorldPos.at<float>(r, 0) = Pos.at<float>(r, 0);
    }
    void ComputeDistinctiveDescriptors() { nDistinctive++; observationsAtDistinctive = (int)mObservations.size(); }
    void UpdateNormalAndDepth() { nUpdateNormal++; }
};

struct Map {
    std::vector<MapPoint*> points;
    void AddMapPoint(MapPoint* pMP) { points.push_back(pMP); }
};

}  // namespace lmock
