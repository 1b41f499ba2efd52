// Test infrastructure: what LocalMapping::SearchInNeighbors touches, for iORB_SLAM::SearchInNeighborsT
// (include/LocalMapping_hip.hpp), without OpenCV.  Unlike the plain data holders of mock_slam.hpp, MapPoint::Replace and
// MapPoint::ComputeDistinctiveDescriptors here are the reference's own (MapPoint.cc:177-215, 242-307), because the drop-in's
// dirty path exists only through them: Replace moves the observations and ends in ComputeDistinctiveDescriptors of the
// survivor.  std::map<KeyFrame*, size_t> is walked in pointer order in the reference; here observations keep their
// INSERTION order, so that a run does not depend on the allocator (tools/fuse_ref.hpp's model does the same).
// KeyFrame::GetFeaturesInArea is KeyFrame.cc:618-657 over a grid filled as Frame.cc:230-245.  Replace and AddObservation are
// logged in call order.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <utility>
#include <vector>

#include "mock_slam.hpp"

namespace fmock {

using mock::KeyPoint;
using mock::Mat;

struct KeyFrame;
struct MapPoint;
struct Event { int type; MapPoint* a; void* b; int c; };   // 1: a->Replace(b); 2: a->AddObservation(b, c)
static std::vector<Event> g_events;

struct MapPoint {
    long mnId = 0;
    Mat mWorldPos = Mat::f32(3, 1), mNormalVector = Mat::f32(3, 1), mDescriptor = Mat::u8(1, 32);
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
    std::vector<std::pair<KeyFrame*, size_t> > mObservations;
    int nObs = 0, mnVisible = 1, mnFound = 1;
    bool mbBad = false;
    MapPoint* mpReplaced = nullptr;
    long mnFuseCandidateForKF = -1;
    int nDistinctive = 0, nUpdateNormal = 0;

    Mat GetWorldPos() { return mWorldPos.clone(); }
    Mat GetNormal() { return mNormalVector.clone(); }
    Mat GetDescriptor() { return mDescriptor.clone(); }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    bool IsInKeyFrame(KeyFrame* pKF)
    {
        for (size_t i = 0; i < mObservations.size(); i++) if (mObservations[i].first == pKF) return true;
        return false;
    }
    void AddObservation(KeyFrame* pKF, size_t idx, bool log = true)   // MapPoint.cc:98-109, monocular
    {
        if (log) g_events.push_back(Event{2, this, pKF, (int)idx});
        if (IsInKeyFrame(pKF)) return;
        mObservations.push_back(std::make_pair(pKF, idx));
        nObs++;
    }
    void IncreaseVisible(int n) { mnVisible += n; }
    void IncreaseFound(int n) { mnFound += n; }
    void Replace(MapPoint* pMP);
    void ComputeDistinctiveDescriptors();
    void UpdateNormalAndDepth() { nUpdateNormal++; }
};

struct KeyFrame {
    long mnId = 0, mnFuseTargetForKF = -1;
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    Mat mDescriptors;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2;
    float mfLogScaleFactor = 0;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0, mnGridCols = 64, mnGridRows = 48;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    std::vector<MapPoint*> mvpMapPoints;
    Mat Tcw = Mat::f32(4, 4), Ow = Mat::f32(3, 1);
    bool mbBad = false;
    std::vector<KeyFrame*> covisible;   // best first
    int nUpdateConnections = 0;

    bool isBad() { return mbBad; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n)
    {
        return (int)covisible.size() < n ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + n);
    }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }
    void ReplaceMapPointMatch(const size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
    Mat GetRotation() { Mat R = Mat::f32(3, 3); for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    Mat GetTranslation() { Mat t = Mat::f32(3, 1); for (int r = 0; r < 3; r++) t.at<float>(r, 0) = Tcw.at<float>(r, 3); return t; }
    Mat GetCameraCenter() { return Ow.clone(); }
    void UpdateConnections() { nUpdateConnections++; }
    void AssignFeaturesToGrid()   // Frame.cc:230-245, PosInGrid :382-392
    {
        mGrid.assign(mnGridCols, std::vector<std::vector<size_t> >(mnGridRows));
        for (int i = 0; i < N; i++) {
            const float px = std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv), py = std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
            if (!(px >= 0.f && px < (float)mnGridCols && py >= 0.f && py < (float)mnGridRows)) continue;
            mGrid[(int)px][(int)py].push_back(i);
        }
    }
    std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r) const   // KeyFrame.cc:618-657
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
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t>& vCell = mGrid[ix][iy];
                for (size_t j = 0; j < vCell.size(); j++) {
                    const KeyPoint& kpUn = mvKeysUn[vCell[j]];
                    const float distx = kpUn.pt.x - x, disty = kpUn.pt.y - y;
                    if (std::fabs(distx) < r && std::fabs(disty) < r) vIndices.push_back(vCell[j]);
                }
            }
        return vIndices;
    }
};

inline void MapPoint::Replace(MapPoint* pMP)   // MapPoint.cc:177-215
{
    if (pMP->mnId == this->mnId) return;
    g_events.push_back(Event{1, this, pMP, 0});
    std::vector<std::pair<KeyFrame*, size_t> > obs;
    obs.swap(mObservations);
    mbBad = true;
    const int nvisible = mnVisible, nfound = mnFound;
    mpReplaced = pMP;
    for (size_t i = 0; i < obs.size(); i++) {
        KeyFrame* pKF = obs[i].first;
        if (!pMP->IsInKeyFrame(pKF)) { pKF->ReplaceMapPointMatch(obs[i].second, pMP); pMP->AddObservation(pKF, obs[i].second, false); }
        else pKF->EraseMapPointMatch(obs[i].second);
    }
    pMP->IncreaseFound(nfound);
    pMP->IncreaseVisible(nvisible);
    pMP->ComputeDistinctiveDescriptors();
}

inline void MapPoint::ComputeDistinctiveDescriptors()   // MapPoint.cc:242-307
{
    nDistinctive++;
    if (mbBad || mObservations.empty()) return;
    std::vector<const unsigned char*> vDescriptors;
    for (size_t i = 0; i < mObservations.size(); i++) {
        KeyFrame* pKF = mObservations[i].first;
        if (!pKF->isBad()) vDescriptors.push_back(pKF->mDescriptors.ptr<unsigned char>((int)mObservations[i].second));
    }
    if (vDescriptors.empty()) return;
    const size_t n = vDescriptors.size();
    std::vector<float> Distances(n * n, 0.f);
    for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
            int distij = 0;
            for (int b = 0; b < 32; b++) distij += __builtin_popcount((unsigned)(vDescriptors[i][b] ^ vDescriptors[j][b]));
            Distances[i * n + j] = Distances[j * n + i] = (float)distij;
        }
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < n; i++) {
        std::vector<int> vDists(Distances.begin() + i * n, Distances.begin() + (i + 1) * n);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (n - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    unsigned char tmp[32];
    std::memcpy(tmp, vDescriptors[BestIdx], 32);
    std::memcpy(mDescriptor.ptr<unsigned char>(0), tmp, 32);
}

}  // namespace fmock
