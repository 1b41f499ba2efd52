// Test infrastructure: what KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling touch, for
// iORB_SLAM::UpdateConnectionsT (include/KeyFrame_hip.hpp) and iORB_SLAM::KeyFrameCullingT (include/LocalMapping_hip.hpp): a
// MapPoint with its observations, a KeyFrame with its match slots, octaves, weight map, ordered lists and spanning-tree
// links.  The bookkeeping members (AddConnection, EraseObservation, SetBadFlag ...) keep the lists consistent the way the
// reference's do; SetBadFlag's spanning-tree repair is cut down to "the children go to the parent".  Nothing here computes
// what the product computes.
#pragma once

#include <algorithm>
#include <cstddef>
#include <list>
#include <map>
#include <set>
#include <vector>

namespace cmock {

struct KeyFrame;
struct Map { long unsigned int mnId = 0; };
struct KeyPoint { int octave = 0; };

struct MapPoint {
    long unsigned int mnId = 0;
    int poolId = -1;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    int nObs = 0;

    bool isBad() { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    void AddObservation(KeyFrame* pKF, size_t idx) { if (!mObservations.count(pKF)) { mObservations[pKF] = idx; nObs++; } }
    inline void EraseObservation(KeyFrame* pKF);   // MapPoint.cc: the point goes bad at two observations left
    inline void SetBadFlag();
};

struct KeyFrame {
    long unsigned int mnId = 0;
    Map* mpMap = nullptr;
    bool mbBad = false, mbFirstConnection = true, mbOtherMapFirst = false, mbNotErase = false, mbToBeErased = false, mbMMKeyframe = false;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyPoint> mvKeysUn;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    std::set<KeyFrame*> mspChildrens, mspMMNeighbours;
    KeyFrame* mpParent = nullptr;

    bool isBad() { return mbBad; }
    bool isOtherMapFirst() { return mbOtherMapFirst; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::set<KeyFrame*> GetConnectedKeyFrames()
    {
        std::set<KeyFrame*> s;
        for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(); mit != mConnectedKeyFrameWeights.end(); mit++) s.insert(mit->first);
        return s;
    }
    std::set<KeyFrame*> GetChilds() { return mspChildrens; }
    KeyFrame* GetParent() { return mpParent; }
    void AddChild(KeyFrame* pKF) { mspChildrens.insert(pKF); }
    void EraseChild(KeyFrame* pKF) { mspChildrens.erase(pKF); }
    void ChangeParent(KeyFrame* pKF) { mpParent = pKF; if (pKF) pKF->AddChild(this); }
    void setConnectedWithOtherMapKF(bool b) { mbMMKeyframe = b; }
    void AddOtherMapKF(KeyFrame* pKF) { mspMMNeighbours.insert(pKF); }
    void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }

    void UpdateBestCovisibles()   // KeyFrame.cc:149-168
    {
        std::vector<std::pair<int, KeyFrame*> > vPairs;
        for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(); mit != mConnectedKeyFrameWeights.end(); mit++)
            vPairs.push_back(std::make_pair(mit->second, mit->first));
        std::sort(vPairs.begin(), vPairs.end());
        mvpOrderedConnectedKeyFrames.clear(); mvOrderedWeights.clear();
        for (size_t i = vPairs.size(); i-- > 0;) { mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second); mvOrderedWeights.push_back(vPairs[i].first); }
    }
    void AddConnection(KeyFrame* pKF, const int& weight)   // KeyFrame.cc:134-147
    {
        if (mConnectedKeyFrameWeights.count(pKF) && mConnectedKeyFrameWeights[pKF] == weight) return;
        mConnectedKeyFrameWeights[pKF] = weight;
        UpdateBestCovisibles();
    }
    void EraseConnection(KeyFrame* pKF) { if (mConnectedKeyFrameWeights.erase(pKF)) UpdateBestCovisibles(); }

    // THE ONE-MEMBER PATCH of INTEGRATION.md: KeyFrame.cc:368-398 given what :302-363 computed -- the other-map marks over the
    // members in sorted order, the three assignments, the first-connection parent
    void AssignConnections(const std::map<KeyFrame*, int>& KFcounter, const std::vector<KeyFrame*>& vpOrdered, const std::vector<int>& vOrderedWs)
    {
        for (size_t i = vpOrdered.size(); i-- > 0;)   // (vPairs ascends where the ordered list descends)
            if (vpOrdered[i]->mpMap->mnId != mpMap->mnId) {
                mbMMKeyframe = true;
                mspMMNeighbours.insert(vpOrdered[i]);
                vpOrdered[i]->setConnectedWithOtherMapKF(true);
                vpOrdered[i]->AddOtherMapKF(this);
            }
        mConnectedKeyFrameWeights = KFcounter;
        mvpOrderedConnectedKeyFrames = vpOrdered;
        mvOrderedWeights = vOrderedWs;
        if (mbFirstConnection && mnId != 0) {
            mpParent = mvpOrderedConnectedKeyFrames.front();
            mpParent->AddChild(this);
            mbFirstConnection = false;
        }
    }

    void SetBadFlag()   // KeyFrame.cc:490-582, the spanning tree cut down
    {
        if (mnId == 0 || mbOtherMapFirst) return;
        if (mbNotErase) { mbToBeErased = true; return; }
        for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(); mit != mConnectedKeyFrameWeights.end(); mit++) mit->first->EraseConnection(this);
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        mConnectedKeyFrameWeights.clear();
        mvpOrderedConnectedKeyFrames.clear();
        const std::set<KeyFrame*> children = mspChildrens;
        for (std::set<KeyFrame*>::const_iterator sit = children.begin(); sit != children.end(); sit++) (*sit)->ChangeParent(mpParent);
        mspChildrens.clear();
        if (mpParent) mpParent->EraseChild(this);
        mbBad = true;
    }
};

inline void MapPoint::SetBadFlag()
{
    const std::map<KeyFrame*, size_t> obs = mObservations;
    mbBad = true;
    mObservations.clear();
    for (std::map<KeyFrame*, size_t>::const_iterator mit = obs.begin(); mit != obs.end(); mit++) mit->first->EraseMapPointMatch(mit->second);
}

inline void MapPoint::EraseObservation(KeyFrame* pKF)
{
    if (!mObservations.count(pKF)) return;
    mObservations.erase(pKF);
    nObs--;
    if (nObs <= 2) SetBadFlag();
}

}  // namespace cmock
