// Test infrastructure: what LoopClosing::CorrectLoop's correction (LoopClosing.cc:455-524) and MultiMapper::UpdatePosesAndAdd's
// (MultiMapper.cc:523-595) touch, for iORB_SLAM::CorrectLoopPosesT (include/LoopClosing_hip.hpp): a KeyFrame with its pose, camera
// centre, match slots, octaves and scale table, a MapPoint with its observations (ordered by mnId, the DEFINED order of the
// headers), reference keyframe, position, normal, bounds and the two correction members; g2o::Sim3 is mock_sim3opt.hpp's.
// Nothing here computes what the product computes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "mock_sim3opt.hpp"

namespace cmock {

struct MapPoint;

struct KeyFrame {
    long unsigned int mnId = 0;
    float Tcw[12] = {0};                    // rows [R | t]
    float Ow[3] = {0.f, 0.f, 0.f};
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<int> mvOctaves;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    int setPoseCalls = 0;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
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
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    bool isBad() { return mbBad; }
};

typedef std::map<KeyFrame*, s3mock::Sim3, ById> KeyFrameAndPose;

}  // namespace cmock
