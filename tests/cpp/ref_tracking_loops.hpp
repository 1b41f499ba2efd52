// Test infrastructure: the serial loops of Tracking::UpdateLocalMap (src/Tracking.cc:1253-1397), Tracking::SearchLocalPoints
// (:1206-1256) and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-129, monocular) over mock types, for the
// programs that hold a drop-in to them: ONE statement of these loops, templated on the mocks (Frame with mvpMapPoints, the grid,
// isInFrustum; KeyFrame and MapPoint as mock_trackpose.hpp has them).  A program's reference Tracking derives from TrackingLoopsT
// and adds what it checks.  (localmap_dropin_gpu.cpp and localmap_update_dropin_gpu.cpp predate this header and keep their own
// statements.)  Plain reference-shaped code: nothing here computes what the product computes.
#pragma once

#include <map>
#include <set>
#include <vector>

#include "mock_slam.hpp"

namespace refloops {

using mock::Mat;
using std::map;
using std::set;
using std::vector;

static const int TH_HIGH = 100;

inline int descriptorDistance(const Mat& a, const unsigned char* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a.ptr<unsigned char>(0)[i] ^ b[i]));
    return d;
}
inline float radiusByViewingCos(const float& viewCos) { if (viewCos > 0.998) return 2.5; else return 4.0; }

template <class Frame, class KeyFrame, class MapPoint>
struct TrackingLoopsT {
    Frame mCurrentFrame;
    vector<KeyFrame*> mvpLocalKeyFrames;
    vector<MapPoint*> mvpLocalMapPoints;
    KeyFrame* mpReferenceKF = nullptr;


    // ORBmatcher.cc:45-129, monocular
    static int SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th, float mfNNratio)
    {
        int nmatches = 0;
        const bool bFactor = th != 1.0;
        for (size_t iMP = 0; iMP < vpMapPoints.size(); iMP++) {
            MapPoint* pMP = vpMapPoints[iMP];
            if (!pMP->mbTrackInView) continue;
            if (pMP->isBad()) continue;
            const int& nPredictedLevel = pMP->mnTrackScaleLevel;
            float r = radiusByViewingCos(pMP->mTrackViewCos);
            if (bFactor) r *= th;
            const vector<size_t> vIndices = F.GetFeaturesInArea(pMP->mTrackProjX, pMP->mTrackProjY, r * F.mvScaleFactors[nPredictedLevel], nPredictedLevel - 1, nPredictedLevel);
            if (vIndices.empty()) continue;
            const Mat MPdescriptor = pMP->GetDescriptor();
            int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
            for (size_t k = 0; k < vIndices.size(); k++) {
                const size_t idx = vIndices[k];
                if (F.mvpMapPoints[idx]) if (F.mvpMapPoints[idx]->Observations() > 0) continue;
                const int dist = descriptorDistance(MPdescriptor, F.mDescriptors.template ptr<unsigned char>((int)idx));
                if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = F.mvKeysUn[idx].octave; bestIdx = (int)idx; }
                else if (dist < bestDist2) { bestLevel2 = F.mvKeysUn[idx].octave; bestDist2 = dist; }
            }
            if (bestDist <= TH_HIGH) {
                if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue;
                F.mvpMapPoints[bestIdx] = pMP;
                nmatches++;
            }
        }
        return nmatches;
    }

    void SearchLocalPoints()   // Tracking.cc:1206-1256
    {
        Frame& F = mCurrentFrame;
        for (size_t t = 0; t < F.mvpMapPoints.size(); t++) {
            MapPoint* pMP = F.mvpMapPoints[t];
            if (pMP) {
                if (pMP->isBad()) F.mvpMapPoints[t] = static_cast<MapPoint*>(NULL);
                else { pMP->IncreaseVisible(1); pMP->mnLastFrameSeen = F.mnId; pMP->mbTrackInView = false; }
            }
        }
        int nToMatch = 0;
        for (size_t i = 0; i < mvpLocalMapPoints.size(); i++) {
            MapPoint* pMP = mvpLocalMapPoints[i];
            if (pMP->mnLastFrameSeen == F.mnId) continue;
            if (pMP->isBad()) continue;
            if (F.isInFrustum(pMP, 0.5)) { pMP->IncreaseVisible(1); nToMatch++; }
        }
        if (nToMatch > 0) SearchByProjection(F, mvpLocalMapPoints, 1.f, 0.8f);
    }

    void UpdateLocalPoints()   // Tracking.cc:1263-1286
    {
        mvpLocalMapPoints.clear();
        for (typename vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
            KeyFrame* pKF = *itKF;
            const vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
            for (typename vector<MapPoint*>::const_iterator itMP = vpMPs.begin(), itEndMP = vpMPs.end(); itMP != itEndMP; itMP++) {
                MapPoint* pMP = *itMP;
                if (!pMP) continue;
                if (pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;
                if (!pMP->isBad()) { mvpLocalMapPoints.push_back(pMP); pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId; }
            }
        }
    }

    void UpdateLocalKeyFrames()   // Tracking.cc:1289-1397
    {
        map<KeyFrame*, int> keyframeCounter;
        for (int i = 0; i < mCurrentFrame.N; i++) {
            if (mCurrentFrame.mvpMapPoints[i]) {
                MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
                if (!pMP->isBad()) {
                    const map<KeyFrame*, size_t> observations = pMP->GetObservations();
                    for (typename map<KeyFrame*, size_t>::const_iterator it = observations.begin(), itend = observations.end(); it != itend; it++) keyframeCounter[it->first]++;
                } else mCurrentFrame.mvpMapPoints[i] = NULL;
            }
        }
        if (keyframeCounter.empty()) return;
        int max = 0;
        KeyFrame* pKFmax = static_cast<KeyFrame*>(NULL);
        mvpLocalKeyFrames.clear();
        mvpLocalKeyFrames.reserve(3 * keyframeCounter.size() + 1);
        for (typename map<KeyFrame*, int>::const_iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {
            KeyFrame* pKF = it->first;
            if (pKF->isBad()) continue;
            if (it->second > max) { max = it->second; pKFmax = pKF; }
            mvpLocalKeyFrames.push_back(it->first);
            pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        }
        for (typename vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
            if (mvpLocalKeyFrames.size() > 80) break;
            KeyFrame* pKF = *itKF;
            const vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (typename vector<KeyFrame*>::const_iterator itNeighKF = vNeighs.begin(), itEndNeighKF = vNeighs.end(); itNeighKF != itEndNeighKF; itNeighKF++) {
                KeyFrame* pNeighKF = *itNeighKF;
                if (!pNeighKF->isBad() && pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pNeighKF);
                    pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            }
            const set<KeyFrame*> spChilds = pKF->GetChilds();
            for (typename set<KeyFrame*>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) {
                KeyFrame* pChildKF = *sit;
                if (!pChildKF->isBad() && pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pChildKF);
                    pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            }
            KeyFrame* pParent = pKF->GetParent();
            if (pParent && pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                mvpLocalKeyFrames.push_back(pParent);
                pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                break;
            }
        }
        if (pKFmax) { mpReferenceKF = pKFmax; mCurrentFrame.mpReferenceKF = mpReferenceKF; }
    }

};

}  // namespace refloops
