// Test infrastructure: what Tracking::TrackReferenceKeyFrame touches beyond mock_trackpose.hpp's Frame, KeyFrame and MapPoint, for
// iORB_SLAM::TrackReferenceKeyFrameT (include/Tracking_hip.hpp): the keyframe's descriptors, mvKeysUn and FeatureVector, and the
// frame's FeatureVector -- a DBoW2::FeatureVector (a map from node id to feature indices, both ascending) held as CSR arrays.
// Plain data holders: nothing here computes what the product computes.
#pragma once

#include <cstdint>
#include <vector>

#include "mock_trackpose.hpp"

namespace rmock {

using mock::KeyPoint;
using mock::Mat;
using qmock::MapPoint;

struct FeatureVector {
    std::vector<uint32_t> node;    // ascending
    std::vector<int32_t> start;    // node.size() + 1
    std::vector<int32_t> idx;      // ascending inside a node
};

struct KeyFrame : qmock::KeyFrame {
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    Mat mDescriptors;
    FeatureVector mFeatVec;
};

struct Frame : qmock::Frame {
    FeatureVector mFeatVec;
};

}  // namespace rmock
