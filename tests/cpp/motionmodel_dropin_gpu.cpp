// iORB_SLAM::TrackWithMotionModelT::Run (include/Tracking_hip.hpp) on mock frames and MapPoints (mock_trackpose.hpp) against
// Tracking::TrackWithMotionModel (Tracking.cc:917-978) written serially over a copy of the same mocks (ref_motionmodel_loops.hpp;
// PoseOptimization through the restatement's Defined mode).  Compared: every mvpMapPoints / mvbOutlier entry of the frame, its pose and
// centre, the number of SetPose calls, every point's mbTrackInView, mnLastFrameSeen, mnFound and mnVisible, the two counts, the return
// value and mbVO -- on a tracked frame, a retried frame, a `return false` frame, and under mbOnlyTracking.
// Built by tests/test_gpu_motionmodel.py; needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "Tracking_hip.hpp"
#include "mock_trackpose.hpp"
#include "ref_motionmodel_loops.hpp"
#include "dropin_test.hpp"
#include "../../tools/poseopt_ref.hpp"

using qmock::Frame;
using qmock::KeyFrame;
using qmock::MapPoint;
using mock::KeyPoint;
using mock::Mat;
using namespace std;

static const int W = 640, H = 480, NLEVELS = 8, CAP = 512;

struct Tracking : refmotion::MotionModelLoopsT<Frame, MapPoint> {
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
};

struct World {
    Tracking trk;
    KeyFrame kf;
    vector<MapPoint> pts;
};

static void fillFrame(Frame& F, int n, long unsigned id)
{
    F.mnId = id; F.N = n;
    F.mvScaleFactors.assign(NLEVELS, 1.f);
    for (int l = 1; l < NLEVELS; l++) F.mvScaleFactors[l] = (float)(F.mvScaleFactors[l - 1] * 1.2);
    F.mvInvLevelSigma2.resize(NLEVELS);
    for (int l = 0; l < NLEVELS; l++) F.mvInvLevelSigma2[l] = 1.0f / (F.mvScaleFactors[l] * F.mvScaleFactors[l]);
    F.mfLogScaleFactor = std::log(1.2f);
    F.mvKeysUn.resize(n); F.mDescriptors = Mat::u8(n, 32); F.mvpMapPoints.assign(n, nullptr); F.mvuRight.assign(n, -1.f);
    F.mvbOutlier.assign(n, false);
}

// The current frame: n features on a jittered lattice (a feature every 14 pixels), a true pose.  The last frame: the same keys and
// descriptors with angles a few degrees off; its feature q < nlast holds point q, which the true pose sees within `noise` pixels of
// current feature q -- except that every `grossEvery`-th lies 5 to 9 pixels off (inside the first window, an outlier of the solve) and
// the points from `farFrom` on lie 24 scaled pixels off (only the window of 2 * th holds them); every 9th last-frame point is flagged an
// outlier of the last frame, every 7th point is unobserved.  mVelocity * mLastFrame.mTcw is the true pose up to float rounding.
static void makeWorld(World& w, unsigned seed, int n, int nlast, int grossEvery, int farFrom, float noise)
{
    mt19937 rng(seed);
    uniform_real_distribution<float> U(0.f, 1.f);
    Frame& F = w.trk.mCurrentFrame;
    Frame& L = w.trk.mLastFrame;
    Frame::fx = 517.3f; Frame::fy = 516.5f; Frame::cx = 318.6f; Frame::cy = 255.3f;
    Frame::mnMinX = 0.f; Frame::mnMaxX = (float)W; Frame::mnMinY = 0.f; Frame::mnMaxY = (float)H;
    Frame::mfGridElementWidthInv = 64.f / W; Frame::mfGridElementHeightInv = 48.f / H;
    fillFrame(F, n, 40); fillFrame(L, n, 39);
    const int cols = 44;
    for (int i = 0; i < n; i++) {
        KeyPoint& k = F.mvKeysUn[i];
        const int cell = (i * 37) % (cols * 32);
        k.pt.x = 14.f + 14.f * (cell % cols) + (U(rng) - 0.5f) * 3.f; k.pt.y = 14.f + 14.f * (cell / cols) + (U(rng) - 0.5f) * 3.f;
        k.octave = (int)(U(rng) * 3) % 3; k.size = 31.f * F.mvScaleFactors[k.octave]; k.angle = U(rng) * 360.f; k.response = 1.f; k.class_id = -1;
        for (int b = 0; b < 32; b++) F.mDescriptors.ptr<unsigned char>(i)[b] = (unsigned char)(rng() & 255);
        L.mvKeysUn[i] = k;
        L.mvKeysUn[i].angle = std::fmod(k.angle + (U(rng) - 0.5f) * 6.f + 360.f, 360.f);
        memcpy(L.mDescriptors.ptr<unsigned char>(i), F.mDescriptors.ptr<unsigned char>(i), 32);
    }
    F.AssignFeaturesToGrid(); L.AssignFeaturesToGrid();
    const float a = 0.02f, ca = std::cos(a), sa = std::sin(a);
    const float R[9] = {ca, 0.f, sa, 0.f, 1.f, 0.f, -sa, 0.f, ca}, t[3] = {0.05f, -0.02f, 0.03f};
    w.pts.clear();
    w.pts.resize((size_t)nlast);   // (each default-constructed: a copied Mat would share its storage, as cv::Mat does)
    w.kf.mnId = 0;
    for (int i = 0; i < nlast; i++) {
        MapPoint& p = w.pts[i];
        p.mnId = i; p.poolId = nlast - 1 - i;
        const float z = 2.f + U(rng) * 12.f, s = F.mvScaleFactors[F.mvKeysUn[i].octave];
        const bool gross = grossEvery && (i % grossEvery) == grossEvery - 1, far = i >= farFrom;
        const float off = far ? 24.f * s : gross ? 5.f + 4.f * U(rng) : (U(rng) - 0.5f) * 2.f * noise;
        const float u = F.mvKeysUn[i].pt.x + off, v = F.mvKeysUn[i].pt.y + (U(rng) - 0.5f) * 2.f * noise;
        const float Xc[3] = {(u - Frame::cx) / Frame::fx * z, (v - Frame::cy) / Frame::fy * z, z};
        for (int r = 0; r < 3; r++) p.mWorldPos.at<float>(r) = R[r] * (Xc[0] - t[0]) + R[3 + r] * (Xc[1] - t[1]) + R[6 + r] * (Xc[2] - t[2]);
        p.mfMaxDistance = 20.f; p.mfMinDistance = 1.f;
        memcpy(p.mDescriptor.ptr<unsigned char>(0), L.mDescriptors.ptr<unsigned char>(i), 32);
        p.mnVisible = 1 + (int)(U(rng) * 20); p.mnFound = 1 + (int)(U(rng) * 10);
        p.mnLastFrameSeen = L.mnId; p.mbTrackInView = true;
        if (i % 7 != 6) p.mObservations[&w.kf] = (size_t)i;
        L.mvpMapPoints[i] = &p;
        L.mvbOutlier[i] = i % 9 == 8;
    }
    // mVelocity: a turn of 10 milliradians about y and a few centimetres; mLastFrame.mTcw = mVelocity^-1 * (R | t)
    const float b = 0.01f, cb = std::cos(b), sb = std::sin(b);
    const float V[16] = {cb, 0.f, sb, 0.03f, 0.f, 1.f, 0.f, -0.01f, -sb, 0.f, cb, 0.02f, 0.f, 0.f, 0.f, 1.f};
    double T[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1}, Vi[16] = {0};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Vi[4 * r + c] = V[4 * c + r];
        Vi[4 * r + 3] = -((double)V[r] * V[3] + (double)V[4 + r] * V[7] + (double)V[8 + r] * V[11]);
    }
    Vi[15] = 1;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += Vi[4 * r + k] * T[4 * k + c];
            L.mTcw.at<float>(r, c) = (float)s;
            w.trk.mVelocity.at<float>(r, c) = V[4 * r + c];
        }
    L.UpdatePoseMatrices();
    F.mTcw.at<float>(0, 0) = F.mTcw.at<float>(1, 1) = F.mTcw.at<float>(2, 2) = F.mTcw.at<float>(3, 3) = 1.f;   // (a new frame's pose is not yet set)
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
        if (p.mnFound != q.mnFound || p.mnVisible != q.mnVisible || p.mbTrackInView != q.mbTrackInView || p.mnLastFrameSeen != q.mnLastFrameSeen) {
            fprintf(stderr, "%s: point %zu found %d/%d visible %d/%d inView %d/%d lastSeen %lu/%lu\n", tag, i, p.mnFound, q.mnFound, p.mnVisible, q.mnVisible,
                    (int)p.mbTrackInView, (int)q.mbTrackInView, p.mnLastFrameSeen, q.mnLastFrameSeen);
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
    vector<void*> mem;
};

static int putFrame(Device& d, Frame& F, int slot)
{
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
    OX(orbm_frameset_build(d.fs, slot, 1, (const OrbxKeyPoint*)dk, (const uint8_t*)dd, (const int32_t*)dn, n));
    OX(orbm_frameset_sync(d.fs));
    return 0;
}

// the world's last frame into slot 0 and its current frame into slot 1 of a fresh frame set, its points into a fresh pool
static int load(Device& d, World& w)
{
    Frame& F = w.trk.mCurrentFrame;
    const float K[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy}, D[5] = {0, 0, 0, 0, 0}, bounds[4] = {0.f, (float)W, 0.f, (float)H};
    OrbmGrid g; g.minX = 0.f; g.minY = 0.f; g.invW = Frame::mfGridElementWidthInv; g.invH = Frame::mfGridElementHeightInv; g.cols = 64; g.rows = 48;
    OX(orbm_frameset_create(d.m, 4, CAP, K, D, &g, bounds, F.mvScaleFactors.data(), NLEVELS, &d.fs));
    int rc;
    if ((rc = putFrame(d, w.trk.mLastFrame, 0)) || (rc = putFrame(d, F, 1))) return rc;
    const int npts = (int)w.pts.size();
    OX(orbw_pool_create(d.m, npts, &d.pool));
    vector<int32_t> ids(npts);
    vector<OrbwPoint> recs(npts);
    for (int i = 0; i < npts; i++) {
        MapPoint& p = w.pts[i];
        ids[i] = p.poolId;
        OrbwPoint& r = recs[i];
        for (int c = 0; c < 3; c++) { r.pos[c] = p.mWorldPos.at<float>(c); r.normal[c] = 0.f; }
        r.min_distance = p.mfMinDistance; r.max_distance = p.mfMaxDistance;
        memcpy(r.desc, p.mDescriptor.ptr<unsigned char>(0), 32);
        r.flags = (uint8_t)((p.isBad() ? ORBW_FLAG_BAD : 0) | (p.Observations() > 0 ? ORBW_FLAG_OBSERVED : 0));
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
    }
    OX(orbw_pool_set(d.pool, ids.data(), recs.data(), npts));
    return 0;
}

static int unload(Device& d)
{
    OX(orbw_pool_destroy(d.pool));
    OX(orbm_frameset_destroy(d.fs));
    for (size_t i = 0; i < d.mem.size(); i++) OX(orbx_device_free(d.ex, d.mem[i]));
    d.mem.clear(); d.pool = nullptr; d.fs = nullptr;
    return 0;
}

typedef iORB_SLAM::TrackWithMotionModelT<Frame, MapPoint> TMM;

// what the case must show: the return value, whether the retry ran, and a floor for the matches left
static int motionModel(Device& d, unsigned seed, int n, int nlast, int grossEvery, int farFrom, bool onlyTracking, int wantOk, bool wantWide, int wantStatus,
                       int minMatches, const char* tag)
{
    World ref, dev;
    makeWorld(ref, seed, n, nlast, grossEvery, farFrom, 0.6f);
    makeWorld(dev, seed, n, nlast, grossEvery, farFrom, 0.6f);
    ref.trk.mbOnlyTracking = onlyTracking;
    int rc = load(d, dev);
    if (rc) return rc;
    const bool want = ref.trk.TrackWithMotionModel(Tracking::PoseOptimization);
    Frame& F = dev.trk.mCurrentFrame;
    // a refusal throws with the frame untouched: a slot outside the set
    {
        bool threw = false;
        try { TMM::Run(d.m, d.fs, 7, 0, d.pool, F, dev.trk.mLastFrame, dev.trk.mVelocity, [](MapPoint* p) { return p->poolId; }, onlyTracking); }
        catch (const std::runtime_error&) { threw = true; }
        if (!threw || F.setPoseCalls != 0) { fprintf(stderr, "%s: a slot outside the set was not refused with the frame untouched\n", tag); return 1; }
    }
    TMM::RunResult got;
    try { got = TMM::Run(d.m, d.fs, 1, 0, d.pool, F, dev.trk.mLastFrame, dev.trk.mVelocity, [](MapPoint* p) { return p->poolId; }, onlyTracking); }
    catch (const std::exception& e) { fprintf(stderr, "%s: Run threw: %s\n", tag, e.what()); return 2; }
    if (compare(dev, ref, tag)) return 1;
    if (got.ok != want || got.nmatches != ref.trk.nmatchesAtReturn || got.nmatchesMap != ref.trk.nmatchesMapAtReturn || (onlyTracking && got.status == ORBQ_MM_TRACKED && got.vo != ref.trk.mbVO)) {
        fprintf(stderr, "%s: ok %d (want %d), nmatches %d (want %d), nmatchesMap %d (want %d), vo %d (want %d)\n", tag, (int)got.ok, (int)want, got.nmatches,
                ref.trk.nmatchesAtReturn, got.nmatchesMap, ref.trk.nmatchesMapAtReturn, (int)got.vo, (int)ref.trk.mbVO);
        return 1;
    }
    if ((wantOk >= 0 && (int)got.ok != wantOk) || got.wide != wantWide || got.status != wantStatus || got.nmatches < minMatches) {
        fprintf(stderr, "%s: the world was built for ok = %d, wide = %d, status %d and %d matches or more; it gives %d, %d, %d, %d (searches %d, %d)\n", tag, wantOk,
                (int)wantWide, wantStatus, minMatches, (int)got.ok, (int)got.wide, got.status, got.nmatches, got.nSearch[0], got.nSearch[1]);
        return 1;
    }
    printf("%s: searches %d, %d; %d matches, %d in the map\n", tag, got.nSearch[0], got.nSearch[1], got.nmatches, got.nmatchesMap);
    return unload(d);
}

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    Device d;
    OX(orbm_create(0, &d.m));
    OrbxParams prm; prm.nfeatures = 1000; prm.scaleFactor = 1.2f; prm.nlevels = NLEVELS; prm.iniThFAST = 20; prm.minThFAST = 7;
    OX(orbx_create(&prm, W, H, 1, 0, &d.ex));
    int rc;
    // a tracked frame: 300 points, every sixth a gross outlier inside the first window
    if ((rc = motionModel(d, 701, 479, 300, 6, 300, false, 1, false, ORBQ_MM_TRACKED, 150, "tracked"))) return rc;
    // a retried frame: 15 points where they are seen (13 of them not outliers of the last frame), 185 more that only 2 * th finds; the
    // verdict is whatever the solve makes of them
    if ((rc = motionModel(d, 702, 479, 200, 0, 15, false, -1, true, ORBQ_MM_TRACKED, 0, "retried"))) return rc;
    // a `return false` frame: 15 points, both searches find fewer than 20
    if ((rc = motionModel(d, 703, 479, 15, 0, 15, false, 0, true, ORBQ_MM_TOO_FEW, 10, "return false"))) return rc;
    // mbOnlyTracking: the verdict reads nmatches, mbVO reads nmatchesMap
    if ((rc = motionModel(d, 704, 479, 300, 6, 300, true, 1, false, ORBQ_MM_TRACKED, 150, "only tracking"))) return rc;
    orbx_destroy(d.ex);
    orbm_destroy(d.m);
    printf("motionmodel dropin ok\n");
    return 0;
}
