// iORB_SLAM::TrackLocalMapT::Run and TrackWithMotionModelT::Finish (include/Tracking_hip.hpp) on mock frames, keyframes and MapPoints
// (mock_trackpose.hpp) against the reference written serially over a copy of the same mocks: Tracking::TrackLocalMap
// (Tracking.cc:980-1024: UpdateLocalMap :1253-1397, SearchLocalPoints :1206-1256 with ORBmatcher::SearchByProjection :45-129 -- those
// loops are ref_tracking_loops.hpp's --, PoseOptimization through the restatement's Defined mode, the loop :994-1013, the verdict :1017-1023) and the tail of
// Tracking::TrackWithMotionModel (:947-977) behind a search whose matches are given.  Compared: every mvpMapPoints / mvbOutlier
// entry, every point's mnFound, mnVisible, mbTrackInView, mnLastFrameSeen and stamp, the pose, the counts and both booleans -- on
// rich worlds, and on worlds whose inlier count is exactly 9, 10, 19, 20, 21, 49 and 50.
// Built by tests/test_gpu_trackpose.py; needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "Tracking_hip.hpp"
#include "mock_trackpose.hpp"
#include "ref_tracking_loops.hpp"
#include "dropin_test.hpp"
#include "../../tools/poseopt_ref.hpp"

using qmock::Frame;
using qmock::KeyFrame;
using qmock::MapPoint;
using mock::KeyPoint;
using mock::Mat;
using namespace std;

static const int W = 640, H = 480, NLEVELS = 8, TH_HIGH = refloops::TH_HIGH, CAP = 512, NKF = 3;

struct Tracking : refloops::TrackingLoopsT<Frame, KeyFrame, MapPoint> {
    bool mbOnlyTracking = false;
    long unsigned int mnLastRelocFrameId = 0;
    int mMaxFrames = 30, mnMatchesInliers = 0;

    // Optimizer.cc:261-473 by the reference's walk, the solve in the restatement's Defined mode
    static int PoseOptimization(Frame* pFrame)
    {
        Frame& F = *pFrame;
        vector<poseopt_ref::Edge> edges;
        vector<int> feature;
        for (int i = 0; i < F.N; i++) {
            MapPoint* p = F.mvpMapPoints[i];
            if (!p) continue;
            F.mvbOutlier[i] = false;
            poseopt_ref::Edge e;
            e.u = F.mvKeysUn[i].pt.x; e.v = F.mvKeysUn[i].pt.y;
            e.invSigma2 = F.mvInvLevelSigma2[F.mvKeysUn[i].octave];
            for (int r = 0; r < 3; r++) e.Xw[r] = p->mWorldPos.at<float>(r, 0);
            edges.push_back(e);
            feature.push_back(i);
        }
        poseopt_ref::Frame rf;
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) rf.Tcw[4 * r + c] = F.mTcw.at<float>(r, c);
        rf.K[0] = Frame::fx; rf.K[1] = Frame::fy; rf.K[2] = Frame::cx; rf.K[3] = Frame::cy;
        vector<uint8_t> outlier(edges.size() + 1, 0);
        poseopt_ref::Result res;
        poseopt_ref::poseOptimization<poseopt_ref::Defined>(rf, edges.data(), (int)edges.size(), res, outlier.data(), nullptr);
        for (size_t k = 0; k < feature.size(); k++) F.mvbOutlier[feature[k]] = outlier[k] != 0;
        if (res.rounds > 0) {
            Mat pose = Mat::f32(4, 4);
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) pose.at<float>(r, c) = res.Tcw[4 * r + c];
            F.SetPose(pose);
        }
        return res.nGood;
    }

    bool TrackLocalMap()   // Tracking.cc:980-1024, monocular
    {
        UpdateLocalKeyFrames(); UpdateLocalPoints();   // UpdateLocalMap, :1253-1261
        SearchLocalPoints();
        PoseOptimization(&mCurrentFrame);
        mnMatchesInliers = 0;
        for (int i = 0; i < mCurrentFrame.N; i++) {
            if (mCurrentFrame.mvpMapPoints[i]) {
                if (!mCurrentFrame.mvbOutlier[i]) {
                    mCurrentFrame.mvpMapPoints[i]->IncreaseFound(1);
                    if (!mbOnlyTracking) { if (mCurrentFrame.mvpMapPoints[i]->Observations() > 0) mnMatchesInliers++; }
                    else mnMatchesInliers++;
                }
            }
        }
        if (mCurrentFrame.mnId < mnLastRelocFrameId + mMaxFrames && mnMatchesInliers < 50) return false;
        if (mnMatchesInliers < 20) return false;
        else return true;
    }

    // Tracking.cc:947-977 behind SearchByProjection(mCurrentFrame, mLastFrame): `matches` is what that search wrote (:1430)
    bool TrackWithMotionModelTail(const vector<pair<int, MapPoint*> >& matches, bool& mbVO, int& nmatchesOut, int& nmatchesMapOut)
    {
        int nmatches = (int)matches.size();
        for (size_t k = 0; k < matches.size(); k++) mCurrentFrame.mvpMapPoints[matches[k].first] = matches[k].second;
        PoseOptimization(&mCurrentFrame);
        int nmatchesMap = 0;
        for (int i = 0; i < mCurrentFrame.N; i++) {
            if (mCurrentFrame.mvpMapPoints[i]) {
                if (mCurrentFrame.mvbOutlier[i]) {
                    MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
                    mCurrentFrame.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
                    mCurrentFrame.mvbOutlier[i] = false;
                    pMP->mbTrackInView = false;
                    pMP->mnLastFrameSeen = mCurrentFrame.mnId;
                    nmatches--;
                } else if (mCurrentFrame.mvpMapPoints[i]->Observations() > 0) nmatchesMap++;
            }
        }
        nmatchesOut = nmatches; nmatchesMapOut = nmatchesMap;
        if (mbOnlyTracking) { mbVO = nmatchesMap < 10; return nmatches > 20; }
        return nmatchesMap >= 10;
    }
};

struct World {
    Tracking trk;
    vector<KeyFrame> kfs;
    vector<MapPoint> pts;
};

// A frame of n features on a jittered lattice (a feature every 14 pixels, so that no window of the search holds two), a true pose
// and a start pose a little off it.  Point i < n is seen within `noise` pixels of feature i at its octave; the points n .. 2n - 1 lie
// anywhere around the frustum.  held: how many features hold their own point before the function (every `stride`-th, the first
// `held` of them), of which every `wrongEvery`-th holds ANOTHER feature's point (a gross outlier); every `grossEvery`-th point lies 5 to 9
// pixels off its feature (matched by a wide window, an outlier of the optimisation).  The three keyframes split the points in order and
// observe them; a few points are bad, a few unobserved (the newest keyframe's are not listed yet).
static void makeWorld(World& w, unsigned seed, int n, int held, int stride, int wrongEvery, bool rich, float noise, int grossEvery = 0)
{
    mt19937 rng(seed);
    uniform_real_distribution<float> U(0.f, 1.f);
    Frame& F = w.trk.mCurrentFrame;
    Frame::fx = 517.3f; Frame::fy = 516.5f; Frame::cx = 318.6f; Frame::cy = 255.3f;
    Frame::mnMinX = 0.f; Frame::mnMaxX = (float)W; Frame::mnMinY = 0.f; Frame::mnMaxY = (float)H;
    Frame::mfGridElementWidthInv = 64.f / W; Frame::mfGridElementHeightInv = 48.f / H;
    F.mnId = 40; F.N = n;
    F.mvScaleFactors.assign(NLEVELS, 1.f);
    for (int l = 1; l < NLEVELS; l++) F.mvScaleFactors[l] = (float)(F.mvScaleFactors[l - 1] * 1.2);
    F.mvInvLevelSigma2.resize(NLEVELS);
    for (int l = 0; l < NLEVELS; l++) F.mvInvLevelSigma2[l] = 1.0f / (F.mvScaleFactors[l] * F.mvScaleFactors[l]);
    F.mfLogScaleFactor = std::log(1.2f);
    F.mvKeysUn.resize(n); F.mDescriptors = Mat::u8(n, 32); F.mvpMapPoints.assign(n, nullptr); F.mvuRight.assign(n, -1.f);
    F.mvbOutlier.assign(n, false);
    const int cols = 44;
    for (int i = 0; i < n; i++) {
        KeyPoint& k = F.mvKeysUn[i];
        const int cell = (i * 37) % (cols * 32);
        k.pt.x = 14.f + 14.f * (cell % cols) + (U(rng) - 0.5f) * 3.f; k.pt.y = 14.f + 14.f * (cell / cols) + (U(rng) - 0.5f) * 3.f;
        k.octave = (int)(U(rng) * 3) % 3; k.size = 31.f * F.mvScaleFactors[k.octave]; k.angle = U(rng) * 360.f; k.response = 1.f; k.class_id = -1;
        for (int b = 0; b < 32; b++) F.mDescriptors.ptr<unsigned char>(i)[b] = (unsigned char)(rng() & 255);
    }
    F.AssignFeaturesToGrid();
    const float a = 0.02f, ca = std::cos(a), sa = std::sin(a);
    const float R[9] = {ca, 0.f, sa, 0.f, 1.f, 0.f, -sa, 0.f, ca}, t[3] = {0.05f, -0.02f, 0.03f};
    // the points as the TRUE pose (R, t) sees them
    float Ow[3];
    for (int r = 0; r < 3; r++) Ow[r] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
    const int npts = rich ? 2 * n : n;
    w.pts.clear();
    w.pts.resize((size_t)npts);   // (each default-constructed: a copied Mat would share its storage, as cv::Mat does)
    for (int i = 0; i < npts; i++) {
        MapPoint& p = w.pts[i];
        p.mnId = i; p.poolId = npts - 1 - i;
        const bool onFeature = i < n;
        const float z = 2.f + U(rng) * 12.f;
        float u, v; int level;
        if (onFeature) {
            const bool gross = grossEvery && (i % grossEvery) == grossEvery - 1;
            u = F.mvKeysUn[i].pt.x + (gross ? 5.f + 4.f * U(rng) : (U(rng) - 0.5f) * 2.f * noise); v = F.mvKeysUn[i].pt.y + (U(rng) - 0.5f) * 2.f * noise; level = F.mvKeysUn[i].octave;
        }
        else { u = -100.f + U(rng) * (W + 200.f); v = -100.f + U(rng) * (H + 200.f); level = (int)(U(rng) * NLEVELS) % NLEVELS; }
        const float Xc[3] = {(u - Frame::cx) / Frame::fx * z, (v - Frame::cy) / Frame::fy * z, z};
        float Xw[3], d[3], dist = 0.f;
        for (int r = 0; r < 3; r++) Xw[r] = R[r] * (Xc[0] - t[0]) + R[3 + r] * (Xc[1] - t[1]) + R[6 + r] * (Xc[2] - t[2]);
        for (int r = 0; r < 3; r++) { d[r] = Xw[r] - Ow[r]; dist += d[r] * d[r]; }
        dist = std::sqrt(dist);
        for (int r = 0; r < 3; r++) { p.mWorldPos.at<float>(r) = Xw[r]; p.mNormalVector.at<float>(r) = d[r] / dist; }
        p.mfMaxDistance = (onFeature ? 0.95f : 0.4f + U(rng) * 2.f) * dist * F.mvScaleFactors[level];
        p.mfMinDistance = p.mfMaxDistance / F.mvScaleFactors[NLEVELS - 1];
        for (int b = 0; b < 32; b++) p.mDescriptor.ptr<unsigned char>(0)[b] = onFeature ? F.mDescriptors.ptr<unsigned char>(i)[b] : (unsigned char)(rng() & 255);
        p.mbBad = rich && U(rng) < 0.04f;
        p.mnVisible = 1 + (int)(U(rng) * 20); p.mnFound = 1 + (int)(U(rng) * 10);
        p.mnLastFrameSeen = F.mnId - 1;
    }
    // three keyframes split the points in order; keyframe 2 is the newest: a tenth of its points do not list it yet
    w.kfs.assign(NKF, KeyFrame());
    const int per = (npts + NKF - 1) / NKF;
    for (int k = 0; k < NKF; k++) {
        KeyFrame& kf = w.kfs[k];
        kf.mnId = k;
        for (int i = k * per; i < std::min(npts, (k + 1) * per); i++) {
            kf.mvpMapPoints.push_back(&w.pts[i]);
            if (!(rich && k == NKF - 1 && U(rng) < 0.1f)) w.pts[i].mObservations[&kf] = kf.mvpMapPoints.size() - 1;
        }
        if (k > 0) { kf.mpParent = &w.kfs[k - 1]; w.kfs[k - 1].mspChildrens.insert(&kf); kf.mvpOrderedConnectedKeyFrames.push_back(&w.kfs[k - 1]); }
        if (k + 1 < NKF) kf.mvpOrderedConnectedKeyFrames.push_back(&w.kfs[k + 1]);
    }
    // the frame's own matches
    int k = 0;
    for (int i = 0; i < n && k < held; i += stride, k++) {
        const bool wrong = wrongEvery && (k % wrongEvery) == wrongEvery - 1;
        F.mvpMapPoints[i] = &w.pts[wrong ? (i + n / 2) % n : i];
    }
    // the start pose: the true one turned by a milliradian and moved by a few millimetres
    const float b = a + 0.001f, cb = std::cos(b), sb = std::sin(b);
    const float Rs[9] = {cb, 0.f, sb, 0.f, 1.f, 0.f, -sb, 0.f, cb};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) F.mTcw.at<float>(r, c) = Rs[3 * r + c]; F.mTcw.at<float>(r, 3) = t[r] + 0.002f * (r - 1); }
    F.mTcw.at<float>(3, 3) = 1.f;
    F.UpdatePoseMatrices();
}

static int compare(World& dev, World& ref, const char* tag)
{
    Frame &a = dev.trk.mCurrentFrame, &b = ref.trk.mCurrentFrame;
    for (int i = 0; i < a.N; i++) {
        const long pa = a.mvpMapPoints[i] ? (long)a.mvpMapPoints[i]->mnId : -1, pb = b.mvpMapPoints[i] ? (long)b.mvpMapPoints[i]->mnId : -1;
        if (pa != pb) { fprintf(stderr, "%s: feature %d holds %ld, want %ld\n", tag, i, pa, pb); return 1; }
        if (a.mvbOutlier[i] != b.mvbOutlier[i]) { fprintf(stderr, "%s: mvbOutlier[%d] = %d, want %d\n", tag, i, (int)a.mvbOutlier[i], (int)b.mvbOutlier[i]); return 1; }
    }
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++)
        if (memcmp(&a.mTcw.at<float>(r, c), &b.mTcw.at<float>(r, c), 4)) { fprintf(stderr, "%s: mTcw(%d, %d) = %.9g, want %.9g\n", tag, r, c, a.mTcw.at<float>(r, c), b.mTcw.at<float>(r, c)); return 1; }
    for (int r = 0; r < 3; r++)
        if (memcmp(&a.mOw.at<float>(r), &b.mOw.at<float>(r), 4)) { fprintf(stderr, "%s: mOw differs\n", tag); return 1; }
    if (a.setPoseCalls != b.setPoseCalls) { fprintf(stderr, "%s: %d SetPose calls, want %d\n", tag, a.setPoseCalls, b.setPoseCalls); return 1; }
    for (size_t i = 0; i < dev.pts.size(); i++) {
        const MapPoint &p = dev.pts[i], &q = ref.pts[i];
        if (p.mnFound != q.mnFound || p.mnVisible != q.mnVisible || p.mbTrackInView != q.mbTrackInView || p.mnLastFrameSeen != q.mnLastFrameSeen ||
            p.mnTrackReferenceForFrame != q.mnTrackReferenceForFrame) {
            fprintf(stderr, "%s: point %zu found %d/%d visible %d/%d inView %d/%d lastSeen %lu/%lu stamp %lu/%lu\n", tag, i, p.mnFound, q.mnFound, p.mnVisible, q.mnVisible,
                    (int)p.mbTrackInView, (int)q.mbTrackInView, p.mnLastFrameSeen, q.mnLastFrameSeen, p.mnTrackReferenceForFrame, q.mnTrackReferenceForFrame);
            return 1;
        }
    }
    return 0;
}

struct Device {
    orbm_t* m = nullptr;
    orbx_t* ex = nullptr;
    orbm_frameset_t* fs = nullptr;
    orbw_pool_t* pool = nullptr;
    orbu_store_t* store = nullptr;
    vector<void*> mem;
};

// the world's frame into slot 1 of a fresh frame set, its points into a fresh pool, its keyframes into a fresh store
static int load(Device& d, World& w)
{
    Frame& F = w.trk.mCurrentFrame;
    const int n = F.N;
    vector<OrbxKeyPoint> keys(n);
    vector<uint8_t> desc((size_t)n * 32);
    for (int i = 0; i < n; i++) {
        const KeyPoint& k = F.mvKeysUn[i];
        keys[i].x = k.pt.x; keys[i].y = k.pt.y; keys[i].size = k.size; keys[i].angle = k.angle; keys[i].response = k.response; keys[i].octave = k.octave; keys[i].class_id = k.class_id;
        memcpy(&desc[(size_t)i * 32], F.mDescriptors.ptr<unsigned char>(i), 32);
    }
    void *dk = nullptr, *dd = nullptr, *dn = nullptr;
    OX(orbx_device_alloc(d.ex, keys.size() * sizeof(OrbxKeyPoint), &dk));
    OX(orbx_device_alloc(d.ex, desc.size(), &dd));
    OX(orbx_device_alloc(d.ex, 4, &dn));
    d.mem.push_back(dk); d.mem.push_back(dd); d.mem.push_back(dn);
    const int32_t count = n;
    OX(orbx_upload(d.ex, dk, keys.data(), keys.size() * sizeof(OrbxKeyPoint)));
    OX(orbx_upload(d.ex, dd, desc.data(), desc.size()));
    OX(orbx_upload(d.ex, dn, &count, 4));
    const float K[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy}, D[5] = {0, 0, 0, 0, 0}, bounds[4] = {0.f, (float)W, 0.f, (float)H};
    OrbmGrid g; g.minX = 0.f; g.minY = 0.f; g.invW = Frame::mfGridElementWidthInv; g.invH = Frame::mfGridElementHeightInv; g.cols = 64; g.rows = 48;
    OX(orbm_frameset_create(d.m, 4, CAP, K, D, &g, bounds, F.mvScaleFactors.data(), NLEVELS, &d.fs));
    OX(orbm_frameset_build(d.fs, 1, 1, (const OrbxKeyPoint*)dk, (const uint8_t*)dd, (const int32_t*)dn, n));
    OX(orbm_frameset_sync(d.fs));
    const int npts = (int)w.pts.size();
    OX(orbw_pool_create(d.m, npts, &d.pool));
    vector<int32_t> ids(npts);
    vector<OrbwPoint> recs(npts);
    for (int i = 0; i < npts; i++) {
        MapPoint& p = w.pts[i];
        ids[i] = p.poolId;
        OrbwPoint& r = recs[i];
        for (int c = 0; c < 3; c++) { r.pos[c] = p.mWorldPos.at<float>(c); r.normal[c] = p.mNormalVector.at<float>(c); }
        r.min_distance = p.mfMinDistance; r.max_distance = p.mfMaxDistance;
        memcpy(r.desc, p.mDescriptor.ptr<unsigned char>(0), 32);
        r.flags = (uint8_t)((p.isBad() ? ORBW_FLAG_BAD : 0) | (p.Observations() > 0 ? ORBW_FLAG_OBSERVED : 0));
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
    }
    OX(orbw_pool_set(d.pool, ids.data(), recs.data(), npts));
    size_t stride = 1;
    for (int k = 0; k < NKF; k++) stride = std::max(stride, w.kfs[k].mvpMapPoints.size());
    OX(orbu_store_create(d.pool, NKF, (int)stride, 4, npts, &d.store));
    typedef iORB_SLAM::UpdateLocalMapT<Frame, KeyFrame, MapPoint> ULM;
    try {
        for (int k = 0; k < NKF; k++) ULM::SyncKeyFrame(d.store, &w.kfs[k], [](MapPoint* p) { return p->poolId; }, [](KeyFrame* kf) { return (int)kf->mnId; });
    } catch (const std::exception& e) { fprintf(stderr, "SyncKeyFrame threw: %s\n", e.what()); return 2; }
    return 0;
}

static int unload(Device& d)
{
    OX(orbu_store_destroy(d.store));
    OX(orbw_pool_destroy(d.pool));
    OX(orbm_frameset_destroy(d.fs));
    for (size_t i = 0; i < d.mem.size(); i++) OX(orbx_device_free(d.ex, d.mem[i]));
    d.mem.clear(); d.store = nullptr; d.pool = nullptr; d.fs = nullptr;
    return 0;
}

typedef iORB_SLAM::TrackLocalMapT<Frame, KeyFrame, MapPoint> TLM;
typedef iORB_SLAM::TrackWithMotionModelT<Frame, MapPoint> TMM;

// TrackLocalMapT::Run on dev against Tracking::TrackLocalMap on ref
static int localMap(Device& d, unsigned seed, int n, int held, int stride, int wrongEvery, bool rich, float noise, bool onlyTracking, long unsigned lastReloc,
                    int wantInliers, bool wantOk, const char* tag, int* inliersOut)
{
    World ref, dev;
    makeWorld(ref, seed, n, held, stride, wrongEvery, rich, noise);
    makeWorld(dev, seed, n, held, stride, wrongEvery, rich, noise);
    ref.trk.mbOnlyTracking = onlyTracking; ref.trk.mnLastRelocFrameId = lastReloc;
    int rc = load(d, dev);
    if (rc) return rc;
    const bool want = ref.trk.TrackLocalMap();
    World* pw = &dev;
    const int npts = (int)dev.pts.size();
    TLM::Options opt;
    opt.verdict.onlyTracking = onlyTracking; opt.verdict.lastRelocFrameId = lastReloc; opt.verdict.maxFrames = 30;
    TLM::Result got;
    try {
        got = TLM::Run(d.m, d.fs, 1, CAP, d.pool, d.store, dev.trk.mCurrentFrame, dev.trk.mvpLocalKeyFrames, dev.trk.mvpLocalMapPoints, dev.trk.mpReferenceKF,
                       [](MapPoint* p) { return p->poolId; }, [](KeyFrame* k) { return (int)k->mnId; }, [pw](int slot) { return &pw->kfs[(size_t)slot]; },
                       [pw, npts](int id) { return &pw->pts[(size_t)(npts - 1 - id)]; }, opt);
    } catch (const std::exception& e) { fprintf(stderr, "%s: Run threw: %s\n", tag, e.what()); return 2; }
    if (compare(dev, ref, tag)) return 1;
    if (got.ok != want || got.nMatchesInliers != ref.trk.mnMatchesInliers) {
        fprintf(stderr, "%s: ok %d (want %d), mnMatchesInliers %d (want %d)\n", tag, (int)got.ok, (int)want, got.nMatchesInliers, ref.trk.mnMatchesInliers);
        return 1;
    }
    if (wantInliers >= 0 && (got.nMatchesInliers != wantInliers || got.ok != wantOk)) {
        fprintf(stderr, "%s: the world was built for %d inliers and ok = %d, it gives %d and %d\n", tag, wantInliers, (int)wantOk, got.nMatchesInliers, (int)got.ok);
        return 1;
    }
    if (dev.trk.mvpLocalMapPoints.size() != ref.trk.mvpLocalMapPoints.size()) { fprintf(stderr, "%s: local points differ\n", tag); return 1; }
    if (inliersOut) *inliersOut = got.nMatchesInliers;
    return unload(d);
}

// TrackWithMotionModelT::Finish on dev against the tail of Tracking::TrackWithMotionModel on ref.  LastFrame is the world's frame
// itself one id earlier: its feature q holds point q for q < nlast (every `grossEvery`-th of them 5 to 9 pixels off), and the search
// from the true pose matches feature q to it.
static int motionModel(Device& d, unsigned seed, int n, int nlast, int grossEvery, float noise, bool onlyTracking, int wantMatches, bool wantOk, const char* tag)
{
    World ref, dev;
    makeWorld(ref, seed, n, 0, 1, 0, false, noise, grossEvery);
    makeWorld(dev, seed, n, 0, 1, 0, false, noise, grossEvery);
    ref.trk.mbOnlyTracking = onlyTracking;
    int rc = load(d, dev);
    if (rc) return rc;
    Frame& F = dev.trk.mCurrentFrame;
    // the last frame: in slot 0, the same features; its points
    {
        // (slot 1's arrays once more into slot 0)
        vector<OrbxKeyPoint> keys(n);
        vector<uint8_t> desc((size_t)n * 32);
        for (int i = 0; i < n; i++) {
            const KeyPoint& k = F.mvKeysUn[i];
            keys[i].x = k.pt.x; keys[i].y = k.pt.y; keys[i].size = k.size; keys[i].angle = k.angle; keys[i].response = k.response; keys[i].octave = k.octave; keys[i].class_id = k.class_id;
            memcpy(&desc[(size_t)i * 32], F.mDescriptors.ptr<unsigned char>(i), 32);
        }
        OX(orbx_upload(d.ex, d.mem[0], keys.data(), keys.size() * sizeof(OrbxKeyPoint)));
        OX(orbm_frameset_build(d.fs, 0, 1, (const OrbxKeyPoint*)d.mem[0], (const uint8_t*)d.mem[1], (const int32_t*)d.mem[2], n));
        OX(orbm_frameset_sync(d.fs));
    }
    vector<MapPoint*> lastDev(n, nullptr), lastRef(n, nullptr);
    vector<int32_t> lastIds(n, -1);
    for (int q = 0; q < nlast; q++) {
        lastDev[q] = &dev.pts[q]; lastRef[q] = &ref.pts[q]; lastIds[q] = dev.pts[q].poolId;
    }
    // SearchByProjection(mCurrentFrame, mLastFrame, th = 15) from the true pose: the world's points project onto their features there,
    // the gross ones a few pixels off, inside the window; the table is taken as the search gives it
    OrbwView view;
    const float a = 0.02f, ca = std::cos(a), sa = std::sin(a);
    const float R[9] = {ca, 0.f, sa, 0.f, 1.f, 0.f, -sa, 0.f, ca}, t[3] = {0.05f, -0.02f, 0.03f};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) view.Rcw[3 * r + c] = R[3 * r + c]; view.tcw[r] = t[r]; view.Ow[r] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]); }
    view.K[0] = Frame::fx; view.K[1] = Frame::fy; view.K[2] = Frame::cx; view.K[3] = Frame::cy;
    view.min_x = 0.f; view.max_x = (float)W; view.min_y = 0.f; view.max_y = (float)H; view.viewing_cos_limit = 0.5f;
    OrbmProjParams pp; pp.mode = 4; pp.nnratio = 0.9f; pp.check_ori = 1; pp.th_dist = TH_HIGH;
    OX(orbw_track_frame_pose(d.fs, 1, 0, d.pool, &pp, &view, lastIds.data(), n, 15.f, F.mvScaleFactors.data(), nullptr));
    const int32_t* assign = nullptr; const int32_t* nm = nullptr;
    OX(orbm_track_results(d.fs, 0, &assign, &nm, nullptr, nullptr));
    vector<pair<int, MapPoint*> > matches;
    for (int i = 0; i < n; i++) if (assign[i] >= 0) matches.push_back(make_pair(i, lastRef[(size_t)assign[i]]));
    if ((int)matches.size() != nm[0]) { fprintf(stderr, "%s: the table holds %zu matches, the count says %d\n", tag, matches.size(), nm[0]); return 1; }
    bool wantVo = false; int wantN = 0, wantMap = 0;
    const bool want = ref.trk.TrackWithMotionModelTail(matches, wantVo, wantN, wantMap);
    // a frame that was not filled with NULL before the search (:940) is refused with nothing written back
    for (int i = 0; i < n; i++) {
        if (assign[i] >= 0) continue;
        F.mvpMapPoints[i] = &dev.pts[0];
        bool threw = false;
        try { TMM::Finish(d.m, d.fs, 1, d.pool, F, lastDev, onlyTracking); } catch (const std::runtime_error&) { threw = true; }
        F.mvpMapPoints[i] = nullptr;
        if (!threw || F.setPoseCalls != 0) { fprintf(stderr, "%s: a frame holding a point the search did not give was not refused\n", tag); return 1; }
        break;
    }
    TMM::Result got;
    try { got = TMM::Finish(d.m, d.fs, 1, d.pool, F, lastDev, onlyTracking); } catch (const std::exception& e) { fprintf(stderr, "%s: Finish threw: %s\n", tag, e.what()); return 2; }
    if (compare(dev, ref, tag)) return 1;
    if (got.ok != want || got.nmatches != wantN || got.nmatchesMap != wantMap || (onlyTracking && got.vo != wantVo)) {
        fprintf(stderr, "%s: ok %d (want %d), nmatches %d (want %d), nmatchesMap %d (want %d), vo %d (want %d)\n", tag, (int)got.ok, (int)want, got.nmatches, wantN, got.nmatchesMap,
                wantMap, (int)got.vo, (int)wantVo);
        return 1;
    }
    if (grossEvery && !(got.nmatches < (int)matches.size() - nlast / (2 * grossEvery))) {
        fprintf(stderr, "%s: %d of %zu matches survive: the gross points were not discarded\n", tag, got.nmatches, matches.size());
        return 1;
    }
    if (wantMatches >= 0 && (got.nmatches != wantMatches || got.ok != wantOk)) {
        fprintf(stderr, "%s: the world was built for %d matches and ok = %d, it gives %d and %d\n", tag, wantMatches, (int)wantOk, got.nmatches, (int)got.ok);
        return 1;
    }
    return unload(d);
}

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    Device d;
    OX(orbm_create(0, &d.m));
    OrbxParams prm; prm.nfeatures = 1000; prm.scaleFactor = 1.2f; prm.nlevels = NLEVELS; prm.iniThFAST = 20; prm.minThFAST = 7;
    OX(orbx_create(&prm, W, H, 1, 0, &d.ex));
    int rc, inliers = 0, total = 0;
    // ---- rich worlds: the frame holds a seventh of its points (a few of them wrong, a few bad), the search adds the rest
    for (unsigned seed = 1; seed <= 3; seed++) {
        char tag[64];
        snprintf(tag, sizeof tag, "local map, rich, seed %u", seed);
        if ((rc = localMap(d, 300 + seed, 479, 70, 7, 5, true, 0.6f, seed == 2, 0, -1, false, tag, &inliers))) return rc;
        if (inliers < 200) { fprintf(stderr, "%s: only %d inliers: the scene does not exercise the function\n", tag, inliers); return 1; }
        total += inliers;
        snprintf(tag, sizeof tag, "motion model, rich, seed %u", seed);
        if ((rc = motionModel(d, 400 + seed, 479, 300, 6, 0.6f, seed == 2, -1, false, tag))) return rc;
    }
    // ---- the verdicts at their thresholds: worlds whose frame holds exactly k exact points and whose local map adds nothing
    const int ks[7] = {9, 10, 19, 20, 21, 49, 50};
    for (int j = 0; j < 7; j++) {
        const int k = ks[j];
        char tag[64];
        snprintf(tag, sizeof tag, "local map, %d inliers", k);
        if ((rc = localMap(d, 500 + k, k, k, 1, 0, false, 0.05f, false, 0, k, k >= 20, tag, nullptr))) return rc;               // :1020
        snprintf(tag, sizeof tag, "local map, %d inliers, relocalised", k);
        if ((rc = localMap(d, 500 + k, k, k, 1, 0, false, 0.05f, false, 25, k, k >= 50, tag, nullptr))) return rc;             // :1017: 40 < 25 + 30
        snprintf(tag, sizeof tag, "local map, %d inliers, only tracking", k);
        if ((rc = localMap(d, 500 + k, k, k, 1, 0, false, 0.05f, true, 0, k, k >= 20, tag, nullptr))) return rc;
        snprintf(tag, sizeof tag, "motion model, %d matches", k);
        if ((rc = motionModel(d, 600 + k, 64, k, 0, 0.05f, false, k, k >= 10, tag))) return rc;                                  // :977
        snprintf(tag, sizeof tag, "motion model, %d matches, only tracking", k);
        if ((rc = motionModel(d, 600 + k, 64, k, 0, 0.05f, true, k, k > 20, tag))) return rc;                                    // :974
    }
    orbx_destroy(d.ex);
    orbm_destroy(d.m);
    printf("trackpose dropin ok: %d inliers over the rich worlds\n", total);
    return 0;
}
