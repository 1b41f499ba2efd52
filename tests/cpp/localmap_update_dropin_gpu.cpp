// iORB_SLAM::UpdateLocalMapT::SyncKeyFrame / Run (include/Tracking_hip.hpp) on mock keyframes, MapPoints and frames
// (mock_localmap_update.hpp) against the serial reference loop -- Tracking::UpdateLocalMap (Tracking.cc:1253-1397) -- over a copy
// of the same mocks: mvpLocalKeyFrames, mvpLocalMapPoints, every keyframe's and point's mnTrackReferenceForFrame, mpReferenceKF,
// F.mpReferenceKF and the frame's nulled bad matches.  The mock keyframes lie in ONE vector in mnId order, so the reference's
// map<KeyFrame*,int> and set<KeyFrame*> iterate in ascending mnId: the defined choice of include/orbslamm_localmap.h.
// Built by tests/test_gpu_localmap_update.py; needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "Tracking_hip.hpp"
#include "mock_localmap_update.hpp"
#include "dropin_test.hpp"

using umock::Frame;
using umock::KeyFrame;
using umock::MapPoint;
using namespace std;

struct Tracking {
    Frame mCurrentFrame;
    vector<KeyFrame*> mvpLocalKeyFrames;
    vector<MapPoint*> mvpLocalMapPoints;
    KeyFrame* mpReferenceKF = nullptr;

    void UpdateLocalPoints()   // Tracking.cc:1263-1286
    {
        mvpLocalMapPoints.clear();
        for (vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
            KeyFrame* pKF = *itKF;
            const vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
            for (vector<MapPoint*>::const_iterator itMP = vpMPs.begin(), itEndMP = vpMPs.end(); itMP != itEndMP; itMP++) {
                MapPoint* pMP = *itMP;
                if (!pMP) continue;
                if (pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;
                if (!pMP->isBad()) {
                    mvpLocalMapPoints.push_back(pMP);
                    pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                }
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
                    for (map<KeyFrame*, size_t>::const_iterator it = observations.begin(), itend = observations.end(); it != itend; it++) keyframeCounter[it->first]++;
                } else {
                    mCurrentFrame.mvpMapPoints[i] = NULL;
                }
            }
        }
        if (keyframeCounter.empty()) return;
        int max = 0;
        KeyFrame* pKFmax = static_cast<KeyFrame*>(NULL);
        mvpLocalKeyFrames.clear();
        mvpLocalKeyFrames.reserve(3 * keyframeCounter.size() + 1);   // (+ 1: the parent of the last step may be the 3n + 1st element)
        for (map<KeyFrame*, int>::const_iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {
            KeyFrame* pKF = it->first;
            if (pKF->isBad()) continue;
            if (it->second > max) { max = it->second; pKFmax = pKF; }
            mvpLocalKeyFrames.push_back(it->first);
            pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        }
        for (vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
            if (mvpLocalKeyFrames.size() > 80) break;
            KeyFrame* pKF = *itKF;
            const vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (vector<KeyFrame*>::const_iterator itNeighKF = vNeighs.begin(), itEndNeighKF = vNeighs.end(); itNeighKF != itEndNeighKF; itNeighKF++) {
                KeyFrame* pNeighKF = *itNeighKF;
                if (!pNeighKF->isBad()) {
                    if (pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                        mvpLocalKeyFrames.push_back(pNeighKF);
                        pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                        break;
                    }
                }
            }
            const set<KeyFrame*> spChilds = pKF->GetChilds();
            for (set<KeyFrame*>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) {
                KeyFrame* pChildKF = *sit;
                if (!pChildKF->isBad()) {
                    if (pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                        mvpLocalKeyFrames.push_back(pChildKF);
                        pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                        break;
                    }
                }
            }
            KeyFrame* pParent = pKF->GetParent();
            if (pParent) {
                if (pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pParent);
                    pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            }
        }
        if (pKFmax) {
            mpReferenceKF = pKFmax;
            mCurrentFrame.mpReferenceKF = mpReferenceKF;
        }
    }

    void UpdateLocalMap() { UpdateLocalKeyFrames(); UpdateLocalPoints(); }   // :1253-1261
};

struct World {
    vector<KeyFrame> kfs;
    vector<MapPoint> pts;
    Tracking trk;
};

static const int NKF = 140, NPTS = 6000, SLOTS = 180, WINDOW = 420;

// keyframe k sees a window of the points around k; the newest keyframe's points do not list it yet (CreateNewKeyFrame ..
// ProcessNewKeyFrame), and a few observations are missing elsewhere; more than ten ordered neighbours; a spanning tree
static void makeWorld(World& w, unsigned seed)
{
    mt19937 rng(seed);
    uniform_real_distribution<float> U(0.f, 1.f);
    w.kfs.assign(NKF, KeyFrame());
    w.pts.assign(NPTS, MapPoint());
    for (int i = 0; i < NPTS; i++) { w.pts[i].mnId = i; w.pts[i].poolId = NPTS - 1 - i; w.pts[i].mbBad = U(rng) < 0.05f; }
    for (int k = 0; k < NKF; k++) {
        KeyFrame& kf = w.kfs[k];
        kf.mnId = k; kf.mbBad = k > 0 && U(rng) < 0.08f;
        kf.mvpMapPoints.assign(SLOTS, nullptr);
        const int lo = (int)((long)k * (NPTS - WINDOW) / NKF);
        set<MapPoint*> held;   // (a MapPoint fills one match slot of a keyframe at the most)
        for (int i = 0; i < SLOTS; i++) {
            if (U(rng) < 0.25f) continue;
            MapPoint* p = &w.pts[lo + (int)(U(rng) * WINDOW)];
            if (!held.insert(p).second) continue;
            kf.mvpMapPoints[i] = p;
            if (k != NKF - 1 && U(rng) < 0.95f) p->mObservations[&kf] = i;
        }
        for (int j = 1; j <= 14; j++) {
            const int o = k + ((j & 1) ? (j + 1) / 2 : -(j / 2)) * (1 + (int)(U(rng) * 3));
            if (o >= 0 && o < NKF && o != k) kf.mvpOrderedConnectedKeyFrames.push_back(&w.kfs[o]);
        }
        if (k > 0) {
            kf.mpParent = &w.kfs[k - 1 - (int)(U(rng) * std::min(k, 4))];
            kf.mpParent->mspChildrens.insert(&kf);
        }
    }
}

// a frame looking at the points around `centre`: nulls, bad points and points in two features
static void makeFrame(World& w, long unsigned int id, int centre, unsigned seed, bool lonely)
{
    mt19937 rng(seed);
    uniform_real_distribution<float> U(0.f, 1.f);
    Frame& F = w.trk.mCurrentFrame;
    F.mnId = id; F.N = 400; F.mvpMapPoints.assign(F.N, nullptr);
    for (int i = 0; i < F.N; i++) {
        if (U(rng) < 0.3f) continue;
        MapPoint* p = &w.pts[std::min(NPTS - 1, std::max(0, centre + (int)((U(rng) - 0.5f) * WINDOW)))];
        if (lonely && !p->mObservations.empty() && !p->mbBad) continue;   // only points nobody observes, and bad ones: no vote at all
        F.mvpMapPoints[i] = p;
        if (i + 1 < F.N && U(rng) < 0.05f) F.mvpMapPoints[++i] = p;
    }
}

static int compare(World& dev, World& ref, const char* tag)
{
    Tracking &a = dev.trk, &b = ref.trk;
    if (a.mvpLocalKeyFrames.size() != b.mvpLocalKeyFrames.size()) { fprintf(stderr, "%s: %zu local keyframes, want %zu\n", tag, a.mvpLocalKeyFrames.size(), b.mvpLocalKeyFrames.size()); return 1; }
    for (size_t i = 0; i < a.mvpLocalKeyFrames.size(); i++)
        if (a.mvpLocalKeyFrames[i]->mnId != b.mvpLocalKeyFrames[i]->mnId) { fprintf(stderr, "%s: local keyframe %zu is %lu, want %lu\n", tag, i, a.mvpLocalKeyFrames[i]->mnId, b.mvpLocalKeyFrames[i]->mnId); return 1; }
    if (a.mvpLocalMapPoints.size() != b.mvpLocalMapPoints.size()) { fprintf(stderr, "%s: %zu local points, want %zu\n", tag, a.mvpLocalMapPoints.size(), b.mvpLocalMapPoints.size()); return 1; }
    for (size_t i = 0; i < a.mvpLocalMapPoints.size(); i++)
        if (a.mvpLocalMapPoints[i]->mnId != b.mvpLocalMapPoints[i]->mnId) { fprintf(stderr, "%s: local point %zu is %lu, want %lu\n", tag, i, a.mvpLocalMapPoints[i]->mnId, b.mvpLocalMapPoints[i]->mnId); return 1; }
    for (int k = 0; k < NKF; k++)
        if (dev.kfs[k].mnTrackReferenceForFrame != ref.kfs[k].mnTrackReferenceForFrame) { fprintf(stderr, "%s: keyframe %d stamped %lu, want %lu\n", tag, k, dev.kfs[k].mnTrackReferenceForFrame, ref.kfs[k].mnTrackReferenceForFrame); return 1; }
    for (int i = 0; i < NPTS; i++)
        if (dev.pts[i].mnTrackReferenceForFrame != ref.pts[i].mnTrackReferenceForFrame) { fprintf(stderr, "%s: point %d stamped %lu, want %lu\n", tag, i, dev.pts[i].mnTrackReferenceForFrame, ref.pts[i].mnTrackReferenceForFrame); return 1; }
    const long ra = a.mpReferenceKF ? (long)a.mpReferenceKF->mnId : -1, rb = b.mpReferenceKF ? (long)b.mpReferenceKF->mnId : -1;
    const long fa = a.mCurrentFrame.mpReferenceKF ? (long)a.mCurrentFrame.mpReferenceKF->mnId : -1, fb = b.mCurrentFrame.mpReferenceKF ? (long)b.mCurrentFrame.mpReferenceKF->mnId : -1;
    if (ra != rb || fa != fb) { fprintf(stderr, "%s: mpReferenceKF %ld / %ld, want %ld / %ld\n", tag, ra, fa, rb, fb); return 1; }
    for (int i = 0; i < a.mCurrentFrame.N; i++) {
        const long pa = a.mCurrentFrame.mvpMapPoints[i] ? (long)a.mCurrentFrame.mvpMapPoints[i]->mnId : -1, pb = b.mCurrentFrame.mvpMapPoints[i] ? (long)b.mCurrentFrame.mvpMapPoints[i]->mnId : -1;
        if (pa != pb) { fprintf(stderr, "%s: feature %d holds %ld, want %ld\n", tag, i, pa, pb); return 1; }
    }
    return 0;
}

typedef iORB_SLAM::UpdateLocalMapT<Frame, KeyFrame, MapPoint> ULM;

static ULM::Result run(orbu_store_t* store, World& w)
{
    World* pw = &w;
    return ULM::Run(store, w.trk.mCurrentFrame, w.trk.mvpLocalKeyFrames, w.trk.mvpLocalMapPoints, w.trk.mpReferenceKF,
                    [](MapPoint* p) { return p->poolId; }, [](KeyFrame* k) { return (int)k->mnId; }, [pw](int slot) { return &pw->kfs[(size_t)slot]; },
                    [pw](int id) { return &pw->pts[(size_t)(NPTS - 1 - id)]; });
}

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    orbm_t* m = nullptr;
    OX(orbm_create(0, &m));
    long totalKf = 0, totalPts = 0, nulled = 0;
    int noVotes = 0;
    for (unsigned seed = 1; seed <= 3; seed++) {
        World ref, dev;
        makeWorld(ref, seed);
        makeWorld(dev, seed);
        orbw_pool_t* pool = nullptr;
        OX(orbw_pool_create(m, NPTS, &pool));
        vector<int32_t> ids(NPTS);
        vector<OrbwPoint> recs(NPTS);
        for (int i = 0; i < NPTS; i++) {
            ids[i] = dev.pts[i].poolId;
            memset(&recs[i], 0, sizeof(OrbwPoint));
            recs[i].flags = (uint8_t)((dev.pts[i].mbBad ? ORBW_FLAG_BAD : 0) | ORBW_FLAG_OBSERVED);
        }
        OX(orbw_pool_set(pool, ids.data(), recs.data(), NPTS));
        orbu_store_t* store = nullptr;
        OX(orbu_store_create(pool, NKF, SLOTS, 16, NPTS, &store));
        int orphans = 0;
        try {
            for (int k = 0; k < NKF; k++) orphans += ULM::SyncKeyFrame(store, &dev.kfs[k], [](MapPoint* p) { return p->poolId; }, [](KeyFrame* kf) { return (int)kf->mnId; });
        } catch (const std::exception& e) { fprintf(stderr, "SyncKeyFrame threw: %s\n", e.what()); return 2; }
        if (orphans != 0) { fprintf(stderr, "%d observations without a match slot in a world that has none\n", orphans); return 1; }
        // frames along the map, the newest keyframe's neighbourhood among them, then a frame nobody votes for
        const int centres[5] = {300, 2500, NPTS - 300, 1200, 4000};
        for (int f = 0; f < 6; f++) {
            const bool lonely = f == 5;
            makeFrame(ref, 10 + f, centres[f % 5], seed * 100 + f, lonely);
            makeFrame(dev, 10 + f, centres[f % 5], seed * 100 + f, lonely);
            for (int i = 0; i < ref.trk.mCurrentFrame.N; i++) nulled += ref.trk.mCurrentFrame.mvpMapPoints[i] && ref.trk.mCurrentFrame.mvpMapPoints[i]->mbBad;
            ref.trk.UpdateLocalMap();
            ULM::Result got;
            try { got = run(store, dev); } catch (const std::exception& e) { fprintf(stderr, "Run threw: %s\n", e.what()); return 2; }
            char tag[64];
            snprintf(tag, sizeof tag, "seed %u frame %d", seed, f);
            if (compare(dev, ref, tag)) return 1;
            if ((got.status == ORBU_NO_VOTES) != lonely) { fprintf(stderr, "%s: status %d\n", tag, got.status); return 1; }
            noVotes += got.status == ORBU_NO_VOTES;
            totalKf += got.nkf; totalPts += got.nL;
        }
        // a refusal throws with everything as it came: a store too small for the local points
        {
            orbu_store_t* small = nullptr;
            OX(orbu_store_create(pool, NKF, SLOTS, 16, 50, &small));
            for (int k = 0; k < NKF; k++) ULM::SyncKeyFrame(small, &dev.kfs[k], [](MapPoint* p) { return p->poolId; }, [](KeyFrame* kf) { return (int)kf->mnId; });
            // SyncKeyFrame's count: two points of keyframe 5 whose observation of it names a slot that does not hold them (one an
            // empty slot, one a slot past the vector), and one whose observation names the wrong slot of two that both hold it
            // (that one HAS a match slot: not counted)
            {
                KeyFrame& kf = dev.kfs[5];
                std::vector<int> held, empty;
                for (int i = 0; i < SLOTS; i++) (kf.mvpMapPoints[i] && kf.mvpMapPoints[i]->mObservations.count(&kf) ? held : empty).push_back(i);
                for (size_t e = 0; e < empty.size();) { if (kf.mvpMapPoints[empty[e]]) empty.erase(empty.begin() + e); else e++; }
                if (held.size() < 3 || empty.size() < 2) { fprintf(stderr, "keyframe 5 has too few slots for the count's case\n"); return 1; }
                std::map<KeyFrame*, size_t> keep[3];
                for (int j = 0; j < 3; j++) keep[j] = kf.mvpMapPoints[held[j]]->mObservations;
                kf.mvpMapPoints[held[0]]->mObservations[&kf] = (size_t)empty[0];
                kf.mvpMapPoints[held[1]]->mObservations[&kf] = (size_t)SLOTS + 7;
                kf.mvpMapPoints[empty[1]] = kf.mvpMapPoints[held[2]];   // in two slots, its observation names the first
                const int count = ULM::SyncKeyFrame(small, &kf, [](MapPoint* p) { return p->poolId; }, [](KeyFrame* k) { return (int)k->mnId; });
                kf.mvpMapPoints[empty[1]] = nullptr;
                for (int j = 0; j < 3; j++) kf.mvpMapPoints[held[j]]->mObservations = keep[j];
                if (count != 2) { fprintf(stderr, "SyncKeyFrame counted %d observations without a match slot, want 2\n", count); return 1; }
                ULM::SyncKeyFrame(small, &kf, [](MapPoint* p) { return p->poolId; }, [](KeyFrame* k) { return (int)k->mnId; });
            }
            makeFrame(ref, 30, 2500, seed, false);
            makeFrame(dev, 30, 2500, seed, false);
            bool threw = false;
            try { run(small, dev); } catch (const std::runtime_error&) { threw = true; }
            if (!threw) { fprintf(stderr, "a store of 50 local points did not refuse\n"); return 1; }
            if (compare(dev, ref, "after a refusal")) return 1;   // (ref has not run either: both hold frame 30 untouched)
            OX(orbu_store_destroy(small));
        }
        OX(orbu_store_destroy(store));
        OX(orbw_pool_destroy(pool));
    }
    if (totalKf < 300 || totalPts < 10000 || nulled < 10 || noVotes != 3) {
        fprintf(stderr, "the scenes do not exercise the function: %ld keyframes, %ld points, %ld nulled, %d without votes\n", totalKf, totalPts, nulled, noVotes);
        return 1;
    }
    orbm_destroy(m);
    printf("localmap update dropin ok: %ld local keyframes, %ld local points\n", totalKf, totalPts);
    return 0;
}
