// iORB_SLAM::UpdateConnectionsT::Run / RunAll (include/KeyFrame_hip.hpp) and iORB_SLAM::KeyFrameCullingT::Run
// (include/LocalMapping_hip.hpp) on mock keyframes and MapPoints (mock_covis.hpp) against the two members written serially --
// KeyFrame::UpdateConnections (KeyFrame.cc:300-400) and LocalMapping::KeyFrameCulling (LocalMapping.cc:632-698) -- over a copy
// of the same mocks.  The mock keyframes lie in ONE vector in mnId order, so the members' map<KeyFrame*,int> iteration and
// pair<int,KeyFrame*> comparison are ascending mnId: the defined slot order of include/orbslamm_covis.h.
// Built by tests/test_gpu_covis.py (and, syntax only, by tests/test_covis_cpu.py); needs a GPU to run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "KeyFrame_hip.hpp"
#include "LocalMapping_hip.hpp"
#include "Tracking_hip.hpp"
#include "mock_covis.hpp"
#include "dropin_test.hpp"

using cmock::KeyFrame;
using cmock::MapPoint;
using namespace std;

// ---- the two members, serially
static void UpdateConnections(KeyFrame* self)   // KeyFrame.cc:300-400
{
    map<KeyFrame*, int> KFcounter;
    const vector<MapPoint*> vpMP = self->mvpMapPoints;
    for (vector<MapPoint*>::const_iterator vit = vpMP.begin(); vit != vpMP.end(); vit++) {
        MapPoint* pMP = *vit;
        if (!pMP || pMP->isBad()) continue;
        const map<KeyFrame*, size_t> observations = pMP->GetObservations();
        for (map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            if (mit->first->mnId == self->mnId) continue;
            KFcounter[mit->first]++;
        }
    }
    if (KFcounter.empty()) return;
    int nmax = 0;
    KeyFrame* pKFmax = NULL;
    const int th = 15;
    vector<pair<int, KeyFrame*> > vPairs;
    for (map<KeyFrame*, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); mit++) {
        if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; }
        if (mit->second >= th) { vPairs.push_back(make_pair(mit->second, mit->first)); (mit->first)->AddConnection(self, mit->second); }
    }
    if (vPairs.empty()) { vPairs.push_back(make_pair(nmax, pKFmax)); pKFmax->AddConnection(self, nmax); }
    sort(vPairs.begin(), vPairs.end());
    list<KeyFrame*> lKFs;
    list<int> lWs;
    for (size_t i = 0; i < vPairs.size(); i++) {
        lKFs.push_front(vPairs[i].second);
        lWs.push_front(vPairs[i].first);
        if (vPairs[i].second->mpMap->mnId != self->mpMap->mnId) {
            self->mbMMKeyframe = true;
            self->mspMMNeighbours.insert(vPairs[i].second);
            vPairs[i].second->setConnectedWithOtherMapKF(true);
            vPairs[i].second->AddOtherMapKF(self);
        }
    }
    self->mConnectedKeyFrameWeights = KFcounter;
    self->mvpOrderedConnectedKeyFrames = vector<KeyFrame*>(lKFs.begin(), lKFs.end());
    self->mvOrderedWeights = vector<int>(lWs.begin(), lWs.end());
    if (self->mbFirstConnection && self->mnId != 0) {
        self->mpParent = self->mvpOrderedConnectedKeyFrames.front();
        self->mpParent->AddChild(self);
        self->mbFirstConnection = false;
    }
}

static void KeyFrameCulling(KeyFrame* mpCurrentKeyFrame)   // LocalMapping.cc:632-698, monocular
{
    vector<KeyFrame*> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();
    for (vector<KeyFrame*>::iterator vit = vpLocalKeyFrames.begin(); vit != vpLocalKeyFrames.end(); vit++) {
        KeyFrame* pKF = *vit;
        if (pKF->mnId == 0 || pKF->isOtherMapFirst()) continue;
        const vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
        const int thObs = 3;
        int nRedundantObservations = 0, nMPs = 0;
        for (size_t i = 0; i < vpMapPoints.size(); i++) {
            MapPoint* pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad()) continue;
            nMPs++;
            if (pMP->Observations() > thObs) {
                const int& scaleLevel = pKF->mvKeysUn[i].octave;
                const map<KeyFrame*, size_t> observations = pMP->GetObservations();
                int nObs = 0;
                for (map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
                    KeyFrame* pKFi = mit->first;
                    if (pKFi == pKF) continue;
                    const int& scaleLeveli = pKFi->mvKeysUn[mit->second].octave;
                    if (scaleLeveli <= scaleLevel + 1) { nObs++; if (nObs >= thObs) break; }
                }
                if (nObs >= thObs) nRedundantObservations++;
            }
        }
        if (nRedundantObservations > 0.9 * nMPs) pKF->SetBadFlag();
    }
}

// ---- worlds
struct World {
    vector<KeyFrame> kfs;
    vector<MapPoint> pts;
    cmock::Map mapA, mapB;
    int nextPt = 0;
    void init(int nkf, int npts, int slots)
    {
        kfs.assign(nkf, KeyFrame());
        pts.assign(npts, MapPoint());
        mapA.mnId = 0; mapB.mnId = 1;
        for (int i = 0; i < npts; i++) { pts[i].mnId = i; pts[i].poolId = npts - 1 - i; }
        for (int k = 0; k < nkf; k++) {
            kfs[k].mnId = k; kfs[k].mpMap = &mapA;
            kfs[k].mvpMapPoints.assign(slots, nullptr);
            kfs[k].mvKeysUn.assign(slots, cmock::KeyPoint());
        }
    }
    // point p into the first free slot of keyframe k; observe: the point lists the keyframe
    int put(int k, int p, int octave, bool observe = true)
    {
        KeyFrame& kf = kfs[k];
        for (size_t i = 0; i < kf.mvpMapPoints.size(); i++)
            if (!kf.mvpMapPoints[i]) {
                kf.mvpMapPoints[i] = &pts[p];
                kf.mvKeysUn[i].octave = octave;
                if (observe) pts[p].AddObservation(&kf, i);
                return (int)i;
            }
        fprintf(stderr, "keyframe %d is full\n", k);
        exit(1);
    }
};

static const int NKF = 30, NPTS = 1500, SLOTS = 96;

// keyframe k sees a window of the points around k: neighbours share more than th points, far keyframes a few or none; a few
// points are bad, a few match slots hold a point that does not list the keyframe; the last ten keyframes are another map's
static void makeCovisWorld(World& w, unsigned seed)
{
    mt19937 rng(seed);
    uniform_real_distribution<float> U(0.f, 1.f);
    w.init(NKF, NPTS, SLOTS);
    for (int i = 0; i < NPTS; i++) w.pts[i].mbBad = U(rng) < 0.04f;
    for (int k = 0; k < NKF; k++) {
        if (k >= 20) w.kfs[k].mpMap = &w.mapB;
        if (k == 17) continue;   // a keyframe without points: its counter is empty
        const int lo = k * (NPTS - 200) / NKF;
        set<int> held;
        for (int i = 0; i < 80; i++) {
            const int p = lo + (int)(U(rng) * 200);
            if (!held.insert(p).second) continue;
            w.put(k, p, (int)(U(rng) * 8), U(rng) < 0.93f);
        }
    }
}

static int sameKeyFrames(World& a, World& b, const char* tag)
{
    for (size_t k = 0; k < a.kfs.size(); k++) {
        KeyFrame &x = a.kfs[k], &y = b.kfs[k];
        map<long, int> wx, wy;
        for (map<KeyFrame*, int>::iterator it = x.mConnectedKeyFrameWeights.begin(); it != x.mConnectedKeyFrameWeights.end(); it++) wx[(long)it->first->mnId] = it->second;
        for (map<KeyFrame*, int>::iterator it = y.mConnectedKeyFrameWeights.begin(); it != y.mConnectedKeyFrameWeights.end(); it++) wy[(long)it->first->mnId] = it->second;
        if (wx != wy) { fprintf(stderr, "%s: keyframe %zu: weight maps of %zu and %zu\n", tag, k, wx.size(), wy.size()); return 1; }
        if (x.mvpOrderedConnectedKeyFrames.size() != y.mvpOrderedConnectedKeyFrames.size() || x.mvOrderedWeights != y.mvOrderedWeights) { fprintf(stderr, "%s: keyframe %zu: ordered lists of %zu and %zu\n", tag, k, x.mvpOrderedConnectedKeyFrames.size(), y.mvpOrderedConnectedKeyFrames.size()); return 1; }
        for (size_t i = 0; i < x.mvpOrderedConnectedKeyFrames.size(); i++)
            if (x.mvpOrderedConnectedKeyFrames[i]->mnId != y.mvpOrderedConnectedKeyFrames[i]->mnId) { fprintf(stderr, "%s: keyframe %zu: ordered[%zu] is %lu, want %lu\n", tag, k, i, x.mvpOrderedConnectedKeyFrames[i]->mnId, y.mvpOrderedConnectedKeyFrames[i]->mnId); return 1; }
        const long px = x.mpParent ? (long)x.mpParent->mnId : -1, py = y.mpParent ? (long)y.mpParent->mnId : -1;
        if (px != py) { fprintf(stderr, "%s: keyframe %zu: parent %ld, want %ld\n", tag, k, px, py); return 1; }
        set<long> cx, cy, mx, my;
        for (set<KeyFrame*>::iterator it = x.mspChildrens.begin(); it != x.mspChildrens.end(); it++) cx.insert((long)(*it)->mnId);
        for (set<KeyFrame*>::iterator it = y.mspChildrens.begin(); it != y.mspChildrens.end(); it++) cy.insert((long)(*it)->mnId);
        for (set<KeyFrame*>::iterator it = x.mspMMNeighbours.begin(); it != x.mspMMNeighbours.end(); it++) mx.insert((long)(*it)->mnId);
        for (set<KeyFrame*>::iterator it = y.mspMMNeighbours.begin(); it != y.mspMMNeighbours.end(); it++) my.insert((long)(*it)->mnId);
        if (cx != cy || mx != my) { fprintf(stderr, "%s: keyframe %zu: children or other-map neighbours differ\n", tag, k); return 1; }
        if (x.mbFirstConnection != y.mbFirstConnection || x.mbMMKeyframe != y.mbMMKeyframe || x.mbBad != y.mbBad) { fprintf(stderr, "%s: keyframe %zu: flags differ\n", tag, k); return 1; }
        for (size_t i = 0; i < x.mvpMapPoints.size(); i++) {
            const long a0 = x.mvpMapPoints[i] ? (long)x.mvpMapPoints[i]->mnId : -1, b0 = y.mvpMapPoints[i] ? (long)y.mvpMapPoints[i]->mnId : -1;
            if (a0 != b0) { fprintf(stderr, "%s: keyframe %zu: slot %zu holds %ld, want %ld\n", tag, k, i, a0, b0); return 1; }
        }
    }
    for (size_t i = 0; i < a.pts.size(); i++)
        if (a.pts[i].mbBad != b.pts[i].mbBad || a.pts[i].nObs != b.pts[i].nObs || a.pts[i].mObservations.size() != b.pts[i].mObservations.size()) { fprintf(stderr, "%s: point %zu differs\n", tag, i); return 1; }
    return 0;
}

struct NoFrame {};
typedef iORB_SLAM::UpdateLocalMapT<NoFrame, KeyFrame, MapPoint> ULM;
typedef iORB_SLAM::UpdateConnectionsT<KeyFrame, MapPoint> UC;
typedef iORB_SLAM::KeyFrameCullingT<KeyFrame, MapPoint> KFC;

static int idOf(MapPoint* p) { return p->poolId; }
static int slotOf(KeyFrame* k) { return (int)k->mnId; }

// a pool and a store holding the world as it is
static int upload(orbm_t* m, World& w, orbw_pool_t** pool, orbu_store_t** store)
{
    const int n = (int)w.pts.size();
    OX(orbw_pool_create(m, n, pool));
    vector<int32_t> ids(n);
    vector<OrbwPoint> recs(n);
    for (int i = 0; i < n; i++) {
        ids[i] = w.pts[i].poolId;
        memset(&recs[i], 0, sizeof(OrbwPoint));
        recs[i].flags = (uint8_t)((w.pts[i].mbBad ? ORBW_FLAG_BAD : 0) | (w.pts[i].nObs > 0 ? ORBW_FLAG_OBSERVED : 0));
    }
    OX(orbw_pool_set(*pool, ids.data(), recs.data(), n));
    OX(orbu_store_create(*pool, (int)w.kfs.size(), (int)w.kfs[0].mvpMapPoints.size(), 64, n, store));
    for (size_t k = 0; k < w.kfs.size(); k++) {
        ULM::SyncKeyFrame(*store, &w.kfs[k], idOf, slotOf);
        KFC::SyncOctaves(*store, &w.kfs[k], slotOf);
    }
    return 0;
}

// both entries over every keyframe of two stores: the same bytes
static int sameStores(orbu_store_t* a, orbu_store_t* b, int nkf, const char* tag)
{
    vector<int32_t> tg(nkf);
    for (int k = 0; k < nkf; k++) tg[k] = k;
    OrbnConnections ra, rb;
    OX(orbn_update_connections(a, tg.data(), nkf, 15, &ra));
    OX(orbn_update_connections(b, tg.data(), nkf, 15, &rb));
    bool same = !memcmp(ra.status, rb.status, nkf * 4) && !memcmp(ra.kf_max, rb.kf_max, nkf * 4) && !memcmp(ra.n_max, rb.n_max, nkf * 4) &&
                !memcmp(ra.cnt_start, rb.cnt_start, (nkf + 1) * 4) && !memcmp(ra.ord_start, rb.ord_start, (nkf + 1) * 4);
    same = same && !memcmp(ra.cnt_kf, rb.cnt_kf, ra.cnt_start[nkf] * 4) && !memcmp(ra.cnt_w, rb.cnt_w, ra.cnt_start[nkf] * 4) &&
           !memcmp(ra.ord_kf, rb.ord_kf, ra.ord_start[nkf] * 4) && !memcmp(ra.ord_w, rb.ord_w, ra.ord_start[nkf] * 4);
    if (!same) { fprintf(stderr, "%s: the store the drop-in kept and a store made from the serial world give other connections\n", tag); return 1; }
    OrbnCulling ca, cb;
    OX(orbn_culling_counts(a, tg.data(), nkf, 3, &ca));
    const vector<int32_t> mps(ca.n_mps, ca.n_mps + nkf), red(ca.n_redundant, ca.n_redundant + nkf);
    OX(orbn_culling_counts(b, tg.data(), nkf, 3, &cb));
    if (memcmp(mps.data(), cb.n_mps, nkf * 4) || memcmp(red.data(), cb.n_redundant, nkf * 4)) { fprintf(stderr, "%s: the two stores give other culling counts\n", tag); return 1; }
    return 0;
}

static int testConnections(orbm_t* m)
{
    long members = 0, otherMap = 0;
    for (unsigned seed = 1; seed <= 2; seed++) {
        World ref, dev;
        makeCovisWorld(ref, seed);
        makeCovisWorld(dev, seed);
        orbw_pool_t* pool = nullptr;
        orbu_store_t* store = nullptr;
        if (int rc = upload(m, dev, &pool, &store)) return rc;
        World* pd = &dev;
        auto kfOf = [pd](int slot) { return &pd->kfs[(size_t)slot]; };
        // every keyframe in an order that is not the slots', then again (no first connection any more), then one alone
        vector<int> order;
        for (int k = 0; k < NKF; k++) order.push_back((k * 7 + 3) % NKF);
        for (int turn = 0; turn < 2; turn++) {
            vector<KeyFrame*> vp;
            for (int k = 0; k < NKF; k++) { UpdateConnections(&ref.kfs[order[k]]); vp.push_back(&dev.kfs[order[k]]); }
            UC::Result r;
            try { r = UC::RunAll(store, vp, slotOf, kfOf); } catch (const std::exception& e) { fprintf(stderr, "RunAll threw: %s\n", e.what()); return 2; }
            if (sameKeyFrames(dev, ref, turn ? "RunAll again" : "RunAll")) return 1;
            if (r.nEmpty != 1 || r.nUpdated != NKF - 1 || (turn == 0 && r.nGraphRecords < NKF - 1)) { fprintf(stderr, "RunAll: %d updated, %d empty, %d graph records\n", r.nUpdated, r.nEmpty, r.nGraphRecords); return 1; }
        }
        // a point moves: one keyframe alone
        for (int q = 0, moved = 0; q < SLOTS && moved < 12; q++) {
            MapPoint* pMP = ref.kfs[5].mvpMapPoints[q];
            if (!pMP || std::count(ref.kfs[9].mvpMapPoints.begin(), ref.kfs[9].mvpMapPoints.end(), pMP)) continue;   // (a point fills one slot of a keyframe)
            ref.put(9, (int)pMP->mnId, 1); dev.put(9, (int)pMP->mnId, 1); moved++;
        }
        ULM::SyncKeyFrame(store, &dev.kfs[9], idOf, slotOf);
        UpdateConnections(&ref.kfs[9]);
        try { UC::Run(store, &dev.kfs[9], slotOf, kfOf); } catch (const std::exception& e) { fprintf(stderr, "Run threw: %s\n", e.what()); return 2; }
        if (sameKeyFrames(dev, ref, "Run")) return 1;
        for (int k = 0; k < NKF; k++) { members += (long)ref.kfs[k].mvpOrderedConnectedKeyFrames.size(); otherMap += (long)ref.kfs[k].mspMMNeighbours.size(); }
        // a refusal throws with every keyframe as it came
        bool threw = false;
        try { UC::RunAll(store, vector<KeyFrame*>(1, &dev.kfs[3]), [](KeyFrame*) { return NKF + 5; }, kfOf); } catch (const std::runtime_error&) { threw = true; }
        if (!threw || sameKeyFrames(dev, ref, "after a refusal")) { fprintf(stderr, "a slot outside the store did not refuse cleanly\n"); return 1; }
        OX(orbu_store_destroy(store));
        OX(orbw_pool_destroy(pool));
    }
    if (members < 40 || otherMap < 2) { fprintf(stderr, "the worlds do not exercise the member: %ld ordered members, %ld other-map neighbours\n", members, otherMap); return 1; }
    return 0;
}

// The culling world.  Keyframe 1 (C) is the current one; its covisible list is 0 (skipped: mnId 0), 2 (A), 3 (B), 4 (D); 5, 6, 7
// (X, Y, Z) are the background.  All octaves are 2, X's are 3.
//   A  30 points seen by A X Y Z, 2 fragile ones seen by A B X, 10 shared ones seen by A B D X Y: 40 of 42 redundant -> culled
//   B  8 points seen by B X Y Z, the 2 fragile, the 10 shared: 18 of 20, and 18 > 18.0 is false -> NOT redundant at first.  A's
//      SetBadFlag leaves the fragile points with two observations: they go bad, B holds 18 of 18 -> culled
//   D  the 10 shared: redundant at first (A B X Y); with A and B gone Observations() is 3 -> NOT redundant any more
static void makeCullingWorld(World& w)
{
    w.init(8, 200, 64);
    const int A = 2, B = 3, D = 4, X = 5, Y = 6, Z = 7;
    int p = 0;
    for (int i = 0; i < 30; i++, p++) { w.put(A, p, 2); w.put(X, p, 3); w.put(Y, p, 2); w.put(Z, p, 2); }
    for (int i = 0; i < 2; i++, p++) { w.put(A, p, 2); w.put(B, p, 2); w.put(X, p, 3); }
    for (int i = 0; i < 10; i++, p++) { w.put(A, p, 2); w.put(B, p, 2); w.put(D, p, 2); w.put(X, p, 3); w.put(Y, p, 2); }
    for (int i = 0; i < 8; i++, p++) { w.put(B, p, 2); w.put(X, p, 3); w.put(Y, p, 2); w.put(Z, p, 2); }
    for (int i = 0; i < 20; i++, p++) { w.put(1, p, 2); w.put(0, p, 2); w.put(Z, p, 2); }   // what C and keyframe 0 see
    for (size_t k = 0; k < w.kfs.size(); k++) UpdateConnections(&w.kfs[k]);
    KeyFrame& C = w.kfs[1];
    C.mvpOrderedConnectedKeyFrames.clear();
    for (int k : {0, A, B, D}) C.mvpOrderedConnectedKeyFrames.push_back(&w.kfs[k]);
}

static int testCulling(orbm_t* m)
{
    World ref, dev;
    makeCullingWorld(ref);
    makeCullingWorld(dev);
    orbw_pool_t* pool = nullptr;
    orbu_store_t* store = nullptr;
    if (int rc = upload(m, dev, &pool, &store)) return rc;
    // the verdicts against the world as it is: A redundant, B not, D redundant
    const int32_t tg[3] = {2, 3, 4};
    OrbnCulling c;
    OX(orbn_culling_counts(store, tg, 3, 3, &c));
    if (!(c.redundant[0] == 1 && c.redundant[1] == 0 && c.redundant[2] == 1 && c.n_mps[0] == 42 && c.n_redundant[0] == 40 && c.n_mps[1] == 20 && c.n_redundant[1] == 18)) {
        fprintf(stderr, "the culling world is not the one described: verdicts %d %d %d, A %d of %d, B %d of %d\n", c.redundant[0], c.redundant[1], c.redundant[2], c.n_redundant[0],
                c.n_mps[0], c.n_redundant[1], c.n_mps[1]);
        return 1;
    }
    KeyFrameCulling(&ref.kfs[1]);
    KFC::Result r;
    try { r = KFC::Run(pool, store, &dev.kfs[1], idOf, slotOf); } catch (const std::exception& e) { fprintf(stderr, "KeyFrameCulling threw: %s\n", e.what()); return 2; }
    if (sameKeyFrames(dev, ref, "culling")) return 1;
    const bool bad[8] = {false, false, true, true, false, false, false, false};
    for (int k = 0; k < 8; k++)
        if (dev.kfs[k].mbBad != bad[k] || ref.kfs[k].mbBad != bad[k]) { fprintf(stderr, "culling: keyframe %d bad %d / %d, want %d\n", k, (int)dev.kfs[k].mbBad, (int)ref.kfs[k].mbBad, (int)bad[k]); return 1; }
    if (r.nCulled != 2 || r.nCalls != 3) { fprintf(stderr, "culling: %d culled in %d calls, want 2 in 3\n", r.nCulled, r.nCalls); return 1; }
    if (!(dev.pts[30].mbBad && dev.pts[31].mbBad)) { fprintf(stderr, "culling: the fragile points did not go bad\n"); return 1; }
    // what the drop-in sent up equals a store made from the serial world
    orbw_pool_t* pool2 = nullptr;
    orbu_store_t* store2 = nullptr;
    if (int rc = upload(m, ref, &pool2, &store2)) return rc;
    if (sameStores(store, store2, 8, "after the culling")) return 1;
    OX(orbu_store_destroy(store2));
    OX(orbw_pool_destroy(pool2));
    OX(orbu_store_destroy(store));
    OX(orbw_pool_destroy(pool));
    return 0;
}

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    orbm_t* m = nullptr;
    OX(orbm_create(0, &m));
    if (int rc = testConnections(m)) return rc;
    if (int rc = testCulling(m)) return rc;
    orbm_destroy(m);
    printf("covis drop-ins: ok\n");
    return 0;
}
