// Test infrastructure: what LoopClosing::SearchAndFuse touches beyond tests/cpp/mock_fuse.hpp, for
// iORB_SLAM::SearchAndFuseT (include/LoopClosing_hip.hpp): KeyFrame::GetMapPoints (KeyFrame.cc:246-259).  The map points, and
// with them Replace and ComputeDistinctiveDescriptors (the reference's own), are mock_fuse.hpp's; a lmock::KeyFrame is a
// fmock::KeyFrame to them.
#pragma once

#include <set>

#include "mock_fuse.hpp"

namespace lmock {

using fmock::MapPoint;
using mock::Mat;

struct KeyFrame : fmock::KeyFrame {
    std::set<MapPoint*> GetMapPoints()
    {
        std::set<MapPoint*> s;
        for (size_t i = 0; i < mvpMapPoints.size(); i++) {
            if (!mvpMapPoints[i]) continue;
            MapPoint* pMP = mvpMapPoints[i];
            if (!pMP->isBad()) s.insert(pMP);
        }
        return s;
    }
};

}  // namespace lmock
