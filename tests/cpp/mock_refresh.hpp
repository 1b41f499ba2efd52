// Test infrastructure: what MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth touch, for
// iORB_SLAM::RefreshMapPointsT (include/MapPoint_hip.hpp): a KeyFrame with its descriptors, octaves, scale table and camera
// centre, a MapPoint with its observations (ordered by mnId, the DEFINED order of the headers), reference keyframe, position
// and the four members the refresh writes.  Nothing here computes what the product computes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace rmock {

struct MapPoint;

struct KeyFrame {
    long unsigned int mnId = 0;
    bool mbBad = false;
    int N = 0;
    std::vector<uint8_t> mDescriptors;      // N x 32
    std::vector<int> mvOctaves;             // mvKeysUn[i].octave
    std::vector<MapPoint*> mvpMapPoints;    // N match slots
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    float mOw[3] = {0.f, 0.f, 0.f};

    bool isBad() { return mbBad; }
};

struct ById {
    bool operator()(const KeyFrame* a, const KeyFrame* b) const { return a->mnId < b->mnId; }
};

struct MapPoint {
    long unsigned int mnId = 0;
    bool mbBad = false;
    std::map<KeyFrame*, size_t, ById> mObservations;
    KeyFrame* mpRefKF = nullptr;
    float mWorldPos[3] = {0.f, 0.f, 0.f}, mNormalVector[3] = {0.f, 0.f, 0.f};
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
    uint8_t mDescriptor[32] = {0};

    bool isBad() { return mbBad; }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    void AddObservation(KeyFrame* pKF, size_t idx) { if (!mObservations.count(pKF)) mObservations[pKF] = idx; }
};

}  // namespace rmock
