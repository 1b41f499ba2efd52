// Test infrastructure: the reference's Frame as Optimizer::PoseOptimization sees it (src/Optimizer.cc:261-473), on top of
// tests/cpp/mock_slam.hpp: the members that function touches which mock::Frame lacks (mvInvLevelSigma2, SetPose).  Plain data
// holders: nothing here computes what the product computes.
#pragma once

#include "mock_slam.hpp"

namespace pomock {

struct Frame : mock::Frame {
    std::vector<float> mvInvLevelSigma2;
    int setPoseCalls = 0;
    void SetPose(mock::Mat Tcw) { mTcw = Tcw.clone(); setPoseCalls++; }   // Frame.cc: mTcw = Tcw.clone(); UpdatePoseMatrices()
};

}  // namespace pomock
