// iORB_SLAM::TrackReferenceKeyFrameT::Run (include/Tracking_hip.hpp) on mock frames, keyframes and MapPoints (mock_trackref.hpp)
// against Tracking::TrackReferenceKeyFrame (Tracking.cc:802-844) written serially over a copy of the same mocks: SearchByBoW
// (ORBmatcher.cc:159-290) with the FeatureVectors orbv_transform gives for the same descriptors, the gate of :814, :817-818,
// PoseOptimization through the restatement's Defined mode, the loop :824-841, the verdict :843.  Compared: every mvpMapPoints /
// mvbOutlier entry, every point's mbTrackInView and mnLastFrameSeen, the pose and mOw, the SetPose calls, the counts and the boolean
// -- on rich worlds (null, bad, unobserved and wrong entries), on worlds of exactly 15 and 14 matches (the too-few frame
// bit-identical to before the call) and of exactly 10 and 9 observed inliers.
// Built by tests/test_gpu_trackref.py; needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "Tracking_hip.hpp"
#include "mock_trackref.hpp"
#include "dropin_test.hpp"
#include "../../tools/poseopt_ref.hpp"

using rmock::Frame;
using rmock::KeyFrame;
using rmock::MapPoint;
using rmock::FeatureVector;
using mock::KeyPoint;
using mock::Mat;
using namespace std;

static const int W = 640, H = 480, NLEVELS = 8, CAP = 512, TH_LOW = 50, HISTO_LENGTH = 30, VOC_K = 6, LEVELSUP = 1;

static void computeThreeMaxima(const vector<int>* histo, int L, int& ind1, int& ind2, int& ind3)   // ORBmatcher.cc:1596-1645
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
}

struct Tracking {
    Frame mCurrentFrame;
    Mat mLastTcw = Mat::f32(4, 4);   // mLastFrame.mTcw
    KeyFrame* mpReferenceKF = nullptr;

    // ORBmatcher.cc:159-290 with mfNNratio, mbCheckOrientation
    static int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches, float mfNNratio, bool mbCheckOrientation)
    {
        const vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
        vpMapPointMatches = vector<MapPoint*>(F.N, static_cast<MapPoint*>(NULL));
        const FeatureVector &fk = pKF->mFeatVec, &ff = F.mFeatVec;
        int nmatches = 0;
        vector<int> rotHist[HISTO_LENGTH];
        const float factor = 1.0f / HISTO_LENGTH;
        size_t a = 0, b = 0;
        while (a < fk.node.size() && b < ff.node.size()) {
            if (fk.node[a] == ff.node[b]) {
                for (int iKF = fk.start[a]; iKF < fk.start[a + 1]; iKF++) {
                    const unsigned int realIdxKF = (unsigned int)fk.idx[iKF];
                    MapPoint* pMP = realIdxKF < vpMapPointsKF.size() ? vpMapPointsKF[realIdxKF] : static_cast<MapPoint*>(NULL);
                    if (!pMP) continue;
                    if (pMP->isBad()) continue;
                    const unsigned char* dKF = pKF->mDescriptors.ptr<unsigned char>((int)realIdxKF);
                    int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
                    for (int iF = ff.start[b]; iF < ff.start[b + 1]; iF++) {
                        const unsigned int realIdxF = (unsigned int)ff.idx[iF];
                        if (vpMapPointMatches[realIdxF]) continue;
                        const int dist = descriptorDistance(dKF, F.mDescriptors.ptr<unsigned char>((int)realIdxF));
                        if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdxF = (int)realIdxF; }
                        else if (dist < bestDist2) bestDist2 = dist;
                    }
                    if (bestDist1 <= TH_LOW) {
                        if ((float)bestDist1 < mfNNratio * (float)bestDist2) {
                            vpMapPointMatches[bestIdxF] = pMP;
                            if (mbCheckOrientation) {
                                float rot = pKF->mvKeysUn[realIdxKF].angle - F.mvKeysUn[bestIdxF].angle;
                                if (rot < 0.0) rot += 360.0f;
                                int bin = (int)round(rot * factor);
                                if (bin == HISTO_LENGTH) bin = 0;
                                rotHist[bin].push_back(bestIdxF);
                            }
                            nmatches++;
                        }
                    }
                }
                a++; b++;
            } else if (fk.node[a] < ff.node[b]) a++;
            else b++;
        }
        if (mbCheckOrientation) {
            int ind1, ind2, ind3;
            computeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
            for (int i = 0; i < HISTO_LENGTH; i++) {
                if (i == ind1 || i == ind2 || i == ind3) continue;
                for (size_t j = 0; j < rotHist[i].size(); j++) { vpMapPointMatches[rotHist[i][j]] = static_cast<MapPoint*>(NULL); nmatches--; }
            }
        }
        return nmatches;
    }

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

    bool TrackReferenceKeyFrame(int& nBow, int& nmatchesMapOut)   // Tracking.cc:802-844
    {
        vector<MapPoint*> vpMapPointMatches;
        int nmatches = SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches, 0.7f, true);
        nBow = nmatches; nmatchesMapOut = 0;
        if (nmatches < 15) return false;
        mCurrentFrame.mvpMapPoints = vpMapPointMatches;
        mCurrentFrame.SetPose(mLastTcw);
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
        nmatchesMapOut = nmatchesMap;
        return nmatchesMap >= 10;
    }
};

struct World {
    Tracking trk;
    KeyFrame kf;
    vector<MapPoint> pts;
    vector<int> src;   // frame feature i copies keyframe feature src[i] and sees point i
};

struct Device {
    orbm_t* m = nullptr;
    orbx_t* ex = nullptr;
    orbv_t* voc = nullptr;
    orbm_frameset_t* fs = nullptr;
    orbw_pool_t* pool = nullptr;
    orbu_store_t* store = nullptr;
    vector<void*> mem;
};

// A frame of n features on a jittered lattice, a true pose and mLastFrame's pose a little off it; point i is seen within `noise`
// pixels of feature i at its octave.  The keyframe has n features of random descriptors; frame feature i is keyframe feature src[i]
// with `nflip` bits flipped and its angle within 3 degrees.  The keyframe's match list holds point i at feature src[i], but: every
// nullEvery-th is NULL, every badEvery-th point is bad, every wrongEvery-th feature holds ANOTHER feature's point, every
// unobsEvery-th point has no observation (the keyframe holds it in the match slot only: ORBU_ENTRY_NO_VOTE in the store).
static void makeWorld(World& w, unsigned seed, int n, int nflip, int nullEvery, int badEvery, int wrongEvery, int unobsEvery, float noise)
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
    KeyFrame& kf = w.kf;
    kf.mnId = 0; kf.N = n;
    kf.mvKeysUn.resize(n); kf.mDescriptors = Mat::u8(n, 32); kf.mvpMapPoints.assign(n, nullptr);
    w.src.resize(n);
    for (int i = 0; i < n; i++) w.src[i] = i;
    shuffle(w.src.begin(), w.src.end(), rng);
    const int cols = 44;
    for (int q = 0; q < n; q++) {
        KeyPoint& k = kf.mvKeysUn[q];
        k.pt.x = 20.f + U(rng) * 600.f; k.pt.y = 20.f + U(rng) * 440.f; k.octave = 0; k.size = 31.f; k.angle = U(rng) * 360.f; k.response = 1.f; k.class_id = -1;
        for (int b = 0; b < 32; b++) kf.mDescriptors.ptr<unsigned char>(q)[b] = (unsigned char)(rng() & 255);
    }
    for (int i = 0; i < n; i++) {
        KeyPoint& k = F.mvKeysUn[i];
        const int cell = (i * 37) % (cols * 32);
        k.pt.x = 14.f + 14.f * (cell % cols) + (U(rng) - 0.5f) * 3.f; k.pt.y = 14.f + 14.f * (cell / cols) + (U(rng) - 0.5f) * 3.f;
        k.octave = (int)(U(rng) * 3) % 3; k.size = 31.f * F.mvScaleFactors[k.octave]; k.response = 1.f; k.class_id = -1;
        k.angle = std::fmod(kf.mvKeysUn[w.src[i]].angle + (U(rng) - 0.5f) * 6.f + 360.f, 360.f);
        unsigned char* d = F.mDescriptors.ptr<unsigned char>(i);
        memcpy(d, kf.mDescriptors.ptr<unsigned char>(w.src[i]), 32);
        for (int f = 0; f < nflip; f++) { const unsigned bit = rng() & 255; d[bit >> 3] ^= (unsigned char)(1u << (bit & 7)); }
    }
    F.AssignFeaturesToGrid();
    const float a = 0.02f, ca = std::cos(a), sa = std::sin(a);
    const float R[9] = {ca, 0.f, sa, 0.f, 1.f, 0.f, -sa, 0.f, ca}, t[3] = {0.05f, -0.02f, 0.03f};
    float Ow[3];
    for (int r = 0; r < 3; r++) Ow[r] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
    w.pts.clear();
    w.pts.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        MapPoint& p = w.pts[i];
        p.mnId = i; p.poolId = n - 1 - i;
        const float z = 2.f + U(rng) * 12.f;
        const float u = F.mvKeysUn[i].pt.x + (U(rng) - 0.5f) * 2.f * noise, v = F.mvKeysUn[i].pt.y + (U(rng) - 0.5f) * 2.f * noise;
        const int level = F.mvKeysUn[i].octave;
        const float Xc[3] = {(u - Frame::cx) / Frame::fx * z, (v - Frame::cy) / Frame::fy * z, z};
        float Xw[3], d[3], dist = 0.f;
        for (int r = 0; r < 3; r++) Xw[r] = R[r] * (Xc[0] - t[0]) + R[3 + r] * (Xc[1] - t[1]) + R[6 + r] * (Xc[2] - t[2]);
        for (int r = 0; r < 3; r++) { d[r] = Xw[r] - Ow[r]; dist += d[r] * d[r]; }
        dist = std::sqrt(dist);
        for (int r = 0; r < 3; r++) { p.mWorldPos.at<float>(r) = Xw[r]; p.mNormalVector.at<float>(r) = d[r] / dist; }
        p.mfMaxDistance = 0.95f * dist * F.mvScaleFactors[level];
        p.mfMinDistance = p.mfMaxDistance / F.mvScaleFactors[NLEVELS - 1];
        memcpy(p.mDescriptor.ptr<unsigned char>(0), F.mDescriptors.ptr<unsigned char>(i), 32);
        p.mbBad = badEvery && (i % badEvery) == badEvery - 1;
        p.mnLastFrameSeen = F.mnId - 1;
        p.mbTrackInView = true;   // (so that the loop's mbTrackInView = false shows)
    }
    for (int i = 0; i < n; i++) {
        const int q = w.src[i];
        if (nullEvery && (i % nullEvery) == nullEvery - 1) continue;
        const bool wrong = wrongEvery && (i % wrongEvery) == wrongEvery - 1;
        MapPoint* p = &w.pts[wrong ? (i + n / 2) % n : i];
        kf.mvpMapPoints[q] = p;
        if (!wrong && !(unobsEvery && (i % unobsEvery) == unobsEvery - 1)) p->mObservations[&kf] = (size_t)q;
    }
    w.trk.mpReferenceKF = &kf;
    // mLastFrame.mTcw: the true pose turned by a milliradian and moved by a few millimetres; the frame's own mTcw is the identity
    const float b = a + 0.001f, cb = std::cos(b), sb = std::sin(b);
    const float Rs[9] = {cb, 0.f, sb, 0.f, 1.f, 0.f, -sb, 0.f, cb};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) w.trk.mLastTcw.at<float>(r, c) = Rs[3 * r + c]; w.trk.mLastTcw.at<float>(r, 3) = t[r] + 0.002f * (r - 1); }
    w.trk.mLastTcw.at<float>(3, 3) = 1.f;
    for (int r = 0; r < 4; r++) F.mTcw.at<float>(r, r) = 1.f;
    F.UpdatePoseMatrices();
}

static int transform(Device& d, const Mat& desc, int n, FeatureVector& fv)
{
    vector<uint32_t> word((size_t)n + 1), node((size_t)n + 1);
    vector<double> val((size_t)n + 1);
    vector<int32_t> start((size_t)n + 2), idx((size_t)n + 1);
    int nw = 0, nn = 0;
    OX(orbv_transform(d.voc, desc.ptr<unsigned char>(0), n, LEVELSUP, word.data(), val.data(), &nw, node.data(), start.data(), idx.data(), &nn));
    fv.node.assign(node.begin(), node.begin() + nn);
    fv.start.assign(start.begin(), start.begin() + nn + 1);
    fv.idx.assign(idx.begin(), idx.begin() + start[(size_t)nn]);
    return 0;
}

static int putSlot(Device& d, int slot, const vector<KeyPoint>& kp, const Mat& descs, int n)
{
    vector<OrbxKeyPoint> keys(n);
    for (int i = 0; i < n; i++) {
        const KeyPoint& k = kp[i];
        keys[i].x = k.pt.x; keys[i].y = k.pt.y; keys[i].size = k.size; keys[i].angle = k.angle; keys[i].response = k.response; keys[i].octave = k.octave; keys[i].class_id = k.class_id;
    }
    void *dk = nullptr, *dd = nullptr, *dn = nullptr;
    OX(orbx_device_alloc(d.ex, keys.size() * sizeof(OrbxKeyPoint), &dk));
    OX(orbx_device_alloc(d.ex, (size_t)n * 32, &dd));
    OX(orbx_device_alloc(d.ex, 4, &dn));
    d.mem.push_back(dk); d.mem.push_back(dd); d.mem.push_back(dn);
    const int32_t count = n;
    OX(orbx_upload(d.ex, dk, keys.data(), keys.size() * sizeof(OrbxKeyPoint)));
    OX(orbx_upload(d.ex, dd, descs.ptr<unsigned char>(0), (size_t)n * 32));
    OX(orbx_upload(d.ex, dn, &count, 4));
    OX(orbm_frameset_build(d.fs, slot, 1, (const OrbxKeyPoint*)dk, (const uint8_t*)dd, (const int32_t*)dn, n));
    return 0;
}

// the keyframe into slot 0 and the frame into slot 1 of a fresh frame set with their BoW, the points into a fresh pool, the keyframe's
// match list into a fresh store; both worlds get the FeatureVectors
static int load(Device& d, World& dev, World& ref)
{
    Frame& F = dev.trk.mCurrentFrame;
    const int n = F.N;
    const float K[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy}, D[5] = {0, 0, 0, 0, 0}, bounds[4] = {0.f, (float)W, 0.f, (float)H};
    OrbmGrid g; g.minX = 0.f; g.minY = 0.f; g.invW = Frame::mfGridElementWidthInv; g.invH = Frame::mfGridElementHeightInv; g.cols = 64; g.rows = 48;
    OX(orbm_frameset_create(d.m, 2, CAP, K, D, &g, bounds, F.mvScaleFactors.data(), NLEVELS, &d.fs));
    int rc;
    if ((rc = putSlot(d, 0, dev.kf.mvKeysUn, dev.kf.mDescriptors, n)) || (rc = putSlot(d, 1, F.mvKeysUn, F.mDescriptors, n))) return rc;
    OX(orbm_frameset_sync(d.fs));
    OX(orbm_frameset_compute_bow(d.fs, d.voc, 0, 2, LEVELSUP));
    if ((rc = transform(d, ref.kf.mDescriptors, n, ref.kf.mFeatVec)) || (rc = transform(d, ref.trk.mCurrentFrame.mDescriptors, n, ref.trk.mCurrentFrame.mFeatVec))) return rc;
    const int npts = (int)dev.pts.size();
    OX(orbw_pool_create(d.m, npts, &d.pool));
    vector<int32_t> ids(npts);
    vector<OrbwPoint> recs(npts);
    for (int i = 0; i < npts; i++) {
        MapPoint& p = dev.pts[i];
        ids[i] = p.poolId;
        OrbwPoint& r = recs[i];
        for (int c = 0; c < 3; c++) { r.pos[c] = p.mWorldPos.at<float>(c); r.normal[c] = p.mNormalVector.at<float>(c); }
        r.min_distance = p.mfMinDistance; r.max_distance = p.mfMaxDistance;
        memcpy(r.desc, p.mDescriptor.ptr<unsigned char>(0), 32);
        r.flags = (uint8_t)((p.isBad() ? ORBW_FLAG_BAD : 0) | (p.Observations() > 0 ? ORBW_FLAG_OBSERVED : 0));
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
    }
    OX(orbw_pool_set(d.pool, ids.data(), recs.data(), npts));
    OX(orbu_store_create(d.pool, 1, n, 0, npts, &d.store));
    typedef iORB_SLAM::UpdateLocalMapT<Frame, qmock::KeyFrame, MapPoint> ULM;
    try {
        ULM::SyncKeyFrame(d.store, static_cast<qmock::KeyFrame*>(&dev.kf), [](MapPoint* p) { return p->poolId; }, [](qmock::KeyFrame* k) { return (int)k->mnId; });
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

static int compare(World& dev, World& ref, const char* tag)
{
    Frame &a = dev.trk.mCurrentFrame, &b = ref.trk.mCurrentFrame;
    for (int i = 0; i < a.N; i++) {
        const long pa = a.mvpMapPoints[i] ? (long)a.mvpMapPoints[i]->mnId : -1, pb = b.mvpMapPoints[i] ? (long)b.mvpMapPoints[i]->mnId : -1;
        if (pa != pb) { fprintf(stderr, "%s: feature %d holds %ld, want %ld\n", tag, i, pa, pb); return 1; }
        if (a.mvpMapPoints[i] && a.mvpMapPoints[i] != &dev.pts[(size_t)pa]) { fprintf(stderr, "%s: feature %d holds a pointer that is not the keyframe's\n", tag, i); return 1; }
        if (a.mvbOutlier[i] != b.mvbOutlier[i]) { fprintf(stderr, "%s: mvbOutlier[%d] = %d, want %d\n", tag, i, (int)a.mvbOutlier[i], (int)b.mvbOutlier[i]); return 1; }
    }
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++)
        if (memcmp(&a.mTcw.at<float>(r, c), &b.mTcw.at<float>(r, c), 4)) { fprintf(stderr, "%s: mTcw(%d, %d) = %.9g, want %.9g\n", tag, r, c, a.mTcw.at<float>(r, c), b.mTcw.at<float>(r, c)); return 1; }
    for (int r = 0; r < 3; r++)
        if (memcmp(&a.mOw.at<float>(r), &b.mOw.at<float>(r), 4)) { fprintf(stderr, "%s: mOw differs\n", tag); return 1; }
    if (a.setPoseCalls != b.setPoseCalls) { fprintf(stderr, "%s: %d SetPose calls, want %d\n", tag, a.setPoseCalls, b.setPoseCalls); return 1; }
    for (size_t i = 0; i < dev.pts.size(); i++) {
        const MapPoint &p = dev.pts[i], &q = ref.pts[i];
        if (p.mbTrackInView != q.mbTrackInView || p.mnLastFrameSeen != q.mnLastFrameSeen || p.mnFound != q.mnFound || p.mnVisible != q.mnVisible) {
            fprintf(stderr, "%s: point %zu inView %d/%d lastSeen %lu/%lu\n", tag, i, (int)p.mbTrackInView, (int)q.mbTrackInView, p.mnLastFrameSeen, q.mnLastFrameSeen);
            return 1;
        }
    }
    return 0;
}

typedef iORB_SLAM::TrackReferenceKeyFrameT<Frame, KeyFrame, MapPoint> TRK;

// edit: applied to both worlds after they are made (the worlds of exact counts); wantBow / wantMap < 0: not asked
template <class Edit>
static int one(Device& d, unsigned seed, int n, int nflip, int nullEvery, int badEvery, int wrongEvery, int unobsEvery, Edit edit, int wantBow, int wantMap,
               const char* tag, int* bowOut, int* mapOut)
{
    World ref, dev;
    makeWorld(ref, seed, n, nflip, nullEvery, badEvery, wrongEvery, unobsEvery, 0.6f);
    makeWorld(dev, seed, n, nflip, nullEvery, badEvery, wrongEvery, unobsEvery, 0.6f);
    edit(ref); edit(dev);
    int rc = load(d, dev, ref);
    if (rc) return rc;
    int nBow = 0, nMap = 0;
    const bool want = ref.trk.TrackReferenceKeyFrame(nBow, nMap);
    TRK::Result got;
    try {
        got = TRK::Run(d.m, d.fs, 0, 1, d.pool, d.store, 0, dev.trk.mCurrentFrame, &dev.kf, dev.trk.mLastTcw);
    } catch (const std::exception& e) { fprintf(stderr, "%s: Run threw: %s\n", tag, e.what()); return 2; }
    if (compare(dev, ref, tag)) return 1;
    if (got.ok != want || got.nBow != nBow || (got.status == ORBQ_REF_TRACKED && got.nmatchesMap != nMap) || (got.status == ORBQ_REF_TOO_FEW) != (nBow < 15)) {
        fprintf(stderr, "%s: ok %d (want %d), n_bow %d (want %d), nmatchesMap %d (want %d), status %d\n", tag, (int)got.ok, (int)want, got.nBow, nBow, got.nmatchesMap, nMap, got.status);
        return 1;
    }
    if (got.status == ORBQ_REF_TOO_FEW) {
        // the too-few frame is as it was before the call: no point, no flag, the identity pose, no SetPose
        const Frame& F = dev.trk.mCurrentFrame;
        for (int i = 0; i < F.N; i++) if (F.mvpMapPoints[i] || F.mvbOutlier[i]) { fprintf(stderr, "%s: the too-few frame was written\n", tag); return 1; }
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) if (F.mTcw.at<float>(r, c) != (r == c ? 1.f : 0.f)) { fprintf(stderr, "%s: the too-few frame's pose was written\n", tag); return 1; }
        if (F.setPoseCalls != 0) { fprintf(stderr, "%s: SetPose on the too-few frame\n", tag); return 1; }
    }
    if ((wantBow >= 0 && nBow != wantBow) || (wantMap >= 0 && nMap != wantMap)) {
        fprintf(stderr, "%s: the world was built for %d matches and %d observed inliers, it gives %d and %d\n", tag, wantBow, wantMap, nBow, nMap);
        return 1;
    }
    if (bowOut) *bowOut = nBow;
    if (mapOut) *mapOut = nMap;
    return unload(d);
}

static void noEdit(World&) {}

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    Device d;
    OX(orbm_create(0, &d.m));
    OrbxParams prm; prm.nfeatures = 1000; prm.scaleFactor = 1.2f; prm.nlevels = NLEVELS; prm.iniThFAST = 20; prm.minThFAST = 7;
    OX(orbx_create(&prm, W, H, 1, 0, &d.ex));
    // a vocabulary of depth 2, six children a node: 6 FeatureVector nodes at level 1, 36 words
    {
        mt19937 rng(11);
        const int nn = VOC_K + VOC_K * VOC_K;
        vector<int32_t> parent(nn);
        vector<uint8_t> leaf(nn), desc((size_t)nn * 32);
        vector<double> weight(nn, 1.0);
        for (int i = 0; i < nn; i++) {
            parent[i] = i < VOC_K ? 0 : 1 + (i - VOC_K) / VOC_K;
            leaf[i] = i >= VOC_K;
            for (int b = 0; b < 32; b++) desc[(size_t)i * 32 + b] = (uint8_t)(rng() & 255);
        }
        OX(orbv_create(0, VOC_K, 2, 0, 0, nn, parent.data(), leaf.data(), desc.data(), weight.data(), &d.voc));
    }
    int rc, nBow = 0, nMap = 0, total = 0;
    // ---- rich worlds: null, bad, wrong and unobserved entries
    for (unsigned seed = 1; seed <= 3; seed++) {
        char tag[64];
        snprintf(tag, sizeof tag, "rich, seed %u", seed);
        if ((rc = one(d, 700 + seed, 400, 6, 9, 11, 13, 7, noEdit, -1, -1, tag, &nBow, &nMap))) return rc;
        if (nBow < 200 || nMap < 150 || nMap >= nBow) { fprintf(stderr, "%s: %d matches, %d observed inliers: the scene does not exercise the function\n", tag, nBow, nMap); return 1; }
        total += nMap;
    }
    // ---- the gate at 15 and 14 matches: a clean world of 40 features, every match the right one; keyframe features lose their point
    // (in the order of the frame's features) until the serial search counts `target`
    for (int target = 15; target >= 14; target--) {
        int found = -1;
        for (int drop = 0; drop <= 40 && found < 0; drop++) {
            World probe;
            makeWorld(probe, 800, 40, 6, 0, 0, 0, 0, 0.05f);
            for (int i = 0; i < drop; i++) probe.kf.mvpMapPoints[probe.src[i]] = nullptr;
            Device& dd = d;
            if (transform(dd, probe.kf.mDescriptors, 40, probe.kf.mFeatVec) || transform(dd, probe.trk.mCurrentFrame.mDescriptors, 40, probe.trk.mCurrentFrame.mFeatVec)) return 2;
            vector<MapPoint*> m;
            if (Tracking::SearchByBoW(&probe.kf, probe.trk.mCurrentFrame, m, 0.7f, true) == target) found = drop;
        }
        if (found < 0) { fprintf(stderr, "no world of %d matches\n", target); return 1; }
        char tag[64];
        snprintf(tag, sizeof tag, "%d matches", target);
        const int drop = found;
        auto edit = [drop](World& w) { for (int i = 0; i < drop; i++) { MapPoint* p = w.kf.mvpMapPoints[w.src[i]]; w.kf.mvpMapPoints[w.src[i]] = nullptr; if (p) p->mObservations.clear(); } };
        if ((rc = one(d, 800, 40, 6, 0, 0, 0, 0, edit, target, -1, tag, nullptr, nullptr))) return rc;
    }
    // ---- the verdict at 10 and 9 observed inliers: a clean world whose first `keep` inliers alone are observed
    for (int keep = 10; keep >= 9; keep--) {
        char tag[64];
        snprintf(tag, sizeof tag, "%d observed inliers", keep);
        // the inliers of the clean world, from the serial side
        World probe;
        makeWorld(probe, 900, 64, 6, 0, 0, 0, 0, 0.05f);
        if (transform(d, probe.kf.mDescriptors, 64, probe.kf.mFeatVec) || transform(d, probe.trk.mCurrentFrame.mDescriptors, 64, probe.trk.mCurrentFrame.mFeatVec)) return 2;
        int b0 = 0, m0 = 0;
        probe.trk.TrackReferenceKeyFrame(b0, m0);
        vector<int> inl;
        for (int i = 0; i < 64; i++) if (probe.trk.mCurrentFrame.mvpMapPoints[i]) inl.push_back((int)probe.trk.mCurrentFrame.mvpMapPoints[i]->mnId);
        if ((int)inl.size() < 20) { fprintf(stderr, "%s: only %zu inliers in the clean world\n", tag, inl.size()); return 1; }
        auto edit = [&inl, keep](World& w) { for (size_t k = (size_t)keep; k < inl.size(); k++) w.pts[(size_t)inl[k]].mObservations.clear(); };
        if ((rc = one(d, 900, 64, 6, 0, 0, 0, 0, edit, -1, keep, tag, nullptr, nullptr))) return rc;
    }
    orbv_destroy(d.voc);
    orbx_destroy(d.ex);
    orbm_destroy(d.m);
    printf("trackref dropin ok: %d observed inliers over the rich worlds\n", total);
    return 0;
}
