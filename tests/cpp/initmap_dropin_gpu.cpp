// iORB_SLAM::InitialMapT (include/Tracking_hip.hpp) on mock keyframes and map points against Tracking.cc:728-758 written serially
// over the restatement (tools/initmap_ref.hpp, Defined mode): after the drop-in the mock map holds what the serial lines leave --
// both poses, the current keyframe's scaled pose, every point's position (scaled where the verdict is ORBB_OK), and the normals and
// distance bounds that the mock's own UpdateNormalAndDepth (the reference's member, here test infrastructure) computed from the
// adjusted poses and positions, which the device's records repeat.  Built and run by tests/dropin.py; prints its marker on success.
#include <map>
#include <vector>

#include "Tracking_hip.hpp"
#include "dropin_test.hpp"
#include "initmap_ref.hpp"

namespace imock {

struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
typedef Mat32 Mat;
struct MapPoint;

struct KeyFrame {
    long unsigned int mnId = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    Mat Tcw = Mat(4, 4, 5);
    float Ow[3] = {0.f, 0.f, 0.f};
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2, mvScaleFactors;
    std::vector<MapPoint*> mvpMapPoints;
    int nSetPose = 0;

    Mat GetPose() { return Tcw; }
    // KeyFrame::SetPose (src/KeyFrame.cc:99-106): the centre by the float arithmetic of gemm with alpha = -1
    void SetPose(const Mat& T)
    {
        Tcw = T;
        float rows[12];
        for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) rows[4 * r + c] = T.at<float>(r, c);
        initmap_ref::cameraCentre(rows, Ow);
        nSetPose++;
    }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};

struct MapPoint {
    Mat mWorldPos = Mat(3, 1, 5);
    float normal[3] = {0.f, 0.f, 0.f}, mfMinDistance = 0.f, mfMaxDistance = 0.f;
    std::vector<std::pair<KeyFrame*, size_t> > obs;   // in the DEFINED order: the initial keyframe, then the current one
    KeyFrame* mpRefKF = nullptr;
    int nUpdates = 0;

    bool isBad() { return false; }
    Mat GetWorldPos() { return mWorldPos; }
    void SetWorldPos(const Mat& P) { mWorldPos = P; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { for (size_t i = 0; i < obs.size(); i++) if (obs[i].first == pKF) return (int)obs[i].second; return -1; }
    // MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:330-371)
    void UpdateNormalAndDepth()
    {
        float P[3] = {mWorldPos.at<float>(0, 0), mWorldPos.at<float>(1, 0), mWorldPos.at<float>(2, 0)}, n[3] = {0.f, 0.f, 0.f};
        for (size_t o = 0; o < obs.size(); o++) {
            float v[3];
            for (int c = 0; c < 3; c++) v[c] = P[c] - obs[o].first->Ow[c];
            const float a = (float)(1. / cv_ref::norm(v, 3));
            for (int c = 0; c < 3; c++) { const float t = v[c] * a; n[c] = t + n[c]; }
        }
        float PC[3];
        for (int c = 0; c < 3; c++) PC[c] = P[c] - mpRefKF->Ow[c];
        const float dist = (float)cv_ref::norm(PC, 3);
        const int level = mpRefKF->mvKeysUn[(size_t)GetIndexInKeyFrame(mpRefKF)].octave;
        mfMaxDistance = dist * mpRefKF->mvScaleFactors[(size_t)level];
        mfMinDistance = mfMaxDistance / mpRefKF->mvScaleFactors.back();
        for (int c = 0; c < 3; c++) normal[c] = cv_ref::exprScale(n[c], 1. / (double)obs.size());
        nUpdates++;
    }
};

}  // namespace imock

using imock::KeyFrame;
using imock::MapPoint;

static bool sameBits(const float* a, const float* b, int n) { return memcmp(a, b, sizeof(float) * (size_t)n) == 0; }

// one two-view scene with n matched points among n1 / n2 features; `behind` puts the points behind the cameras (a negative median)
static int one(orbm_t* h, int n, unsigned seed, bool fixedFirst, bool behind)
{
    const int nlevels = 8, n1 = n + n / 4 + 3, n2 = n + 7;
    KeyFrame ini, cur;
    ini.mnId = fixedFirst ? 0 : 4; cur.mnId = ini.mnId + 1;
    KeyFrame* kfs[2] = {&ini, &cur};
    for (int s = 0; s < 2; s++) {
        kfs[s]->fx = 517.3f; kfs[s]->fy = 516.5f; kfs[s]->cx = 318.6f; kfs[s]->cy = 255.3f;
        float sf = 1.f;
        for (int l = 0; l < nlevels; l++) { kfs[s]->mvScaleFactors.push_back(sf); kfs[s]->mvInvLevelSigma2.push_back(1.f / (sf * sf)); sf *= 1.2f; }
    }
    unsigned st = seed;
    setPoseEuler(ini, 0.02, 0.2, -0.01, 0.1, -0.05, 0.2);
    setPoseEuler(cur, 0.03, 0.23, 0.01, -0.45, -0.02, 0.25);
    ini.mvKeysUn.resize((size_t)n1); cur.mvKeysUn.resize((size_t)n2);
    for (int s = 0; s < 2; s++)
        for (size_t i = 0; i < kfs[s]->mvKeysUn.size(); i++) {
            imock::KeyPoint k = {{(float)(640 * urand(st)), (float)(480 * urand(st))}, 31.f, 0.f, 1.f, (int)(urand(st) * nlevels), -1};
            kfs[s]->mvKeysUn[i] = k;
        }
    ini.mvpMapPoints.assign((size_t)n1, nullptr);
    std::vector<MapPoint> pool((size_t)n);
    std::vector<int> perm((size_t)n2);
    for (int i = 0; i < n2; i++) perm[(size_t)i] = i;
    for (int i = n2 - 1; i > 0; i--) { const int j = (int)(urand(st) * (i + 1)); std::swap(perm[(size_t)i], perm[(size_t)j]); }
    int k = 0;
    for (int i = 0; i < n1 && k < n; i++) {
        if ((n1 - i) > (n - k) && urand(st) < 0.2) continue;   // an unmatched feature
        MapPoint& mp = pool[(size_t)k];
        // a point in front of (or behind) the initial camera, observed by both with half a pixel of noise
        const double z = (behind ? -1.0 : 1.0) * (4.0 + 5.0 * urand(st)), xc = (urand(st) - 0.5) * 0.8 * z, yc = (urand(st) - 0.5) * 0.6 * z;
        double Xw[3];
        for (int c = 0; c < 3; c++) {
            const double d[3] = {xc - ini.Tcw.at<float>(0, 3), yc - ini.Tcw.at<float>(1, 3), z - ini.Tcw.at<float>(2, 3)};
            Xw[c] = ini.Tcw.at<float>(0, c) * d[0] + ini.Tcw.at<float>(1, c) * d[1] + ini.Tcw.at<float>(2, c) * d[2];
        }
        const int feat[2] = {i, perm[(size_t)k]};
        for (int s = 0; s < 2; s++) {
            double pc[3];
            for (int r = 0; r < 3; r++)
                pc[r] = kfs[s]->Tcw.at<float>(r, 0) * Xw[0] + kfs[s]->Tcw.at<float>(r, 1) * Xw[1] + kfs[s]->Tcw.at<float>(r, 2) * Xw[2] + kfs[s]->Tcw.at<float>(r, 3);
            imock::KeyPoint& kp = kfs[s]->mvKeysUn[(size_t)feat[s]];
            kp.pt.x = (float)(kfs[s]->fx * pc[0] / pc[2] + kfs[s]->cx + (urand(st) - 0.5));
            kp.pt.y = (float)(kfs[s]->fy * pc[1] / pc[2] + kfs[s]->cy + (urand(st) - 0.5));
            mp.obs.push_back(std::make_pair(kfs[s], (size_t)feat[s]));
        }
        for (int c = 0; c < 3; c++) mp.mWorldPos.at<float>(c, 0) = (float)(Xw[c] * (1.0 + 0.02 * (urand(st) - 0.5)));
        mp.mpRefKF = &cur;
        ini.mvpMapPoints[(size_t)i] = &mp;
        k++;
    }
    // the start: the current pose a little off
    cur.Tcw.at<float>(0, 3) += 0.02f; cur.Tcw.at<float>(2, 3) -= 0.015f;
    ini.SetPose(ini.Tcw); cur.SetPose(cur.Tcw);
    ini.nSetPose = cur.nSetPose = 0;

    // ---- the restatement on the same inputs, then Tracking.cc:728-758 written serially over its outputs
    initmap_ref::Problem pr;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { pr.Tcw1[4 * r + c] = ini.Tcw.at<float>(r, c); pr.Tcw2[4 * r + c] = cur.Tcw.at<float>(r, c); }
    pr.K[0] = ini.fx; pr.K[1] = ini.fy; pr.K[2] = ini.cx; pr.K[3] = ini.cy;
    pr.fixedFirst = ini.mnId == 0; pr.fixedSecond = 0; pr.iterations = 20; pr.robust = 1; pr.n1 = n1; pr.n2 = n2;
    std::vector<initmap_ref::Key> k1((size_t)n1), k2((size_t)n2);
    for (int i = 0; i < n1; i++) { initmap_ref::Key q = {ini.mvKeysUn[(size_t)i].pt.x, ini.mvKeysUn[(size_t)i].pt.y, ini.mvKeysUn[(size_t)i].octave}; k1[(size_t)i] = q; }
    for (int i = 0; i < n2; i++) { initmap_ref::Key q = {cur.mvKeysUn[(size_t)i].pt.x, cur.mvKeysUn[(size_t)i].pt.y, cur.mvKeysUn[(size_t)i].octave}; k2[(size_t)i] = q; }
    std::vector<int32_t> m12((size_t)n1, -1);
    std::vector<float> P3D(3 * (size_t)n1, 0.f);
    for (int i = 0; i < n1; i++)
        if (ini.mvpMapPoints[(size_t)i]) {
            m12[(size_t)i] = ini.mvpMapPoints[(size_t)i]->GetIndexInKeyFrame(&cur);
            for (int c = 0; c < 3; c++) P3D[3 * (size_t)i + c] = ini.mvpMapPoints[(size_t)i]->mWorldPos.at<float>(c, 0);
        }
    initmap_ref::Result want;
    std::vector<initmap_ref::Point> wpts((size_t)n1);
    initmap_ref::initialMap<initmap_ref::Defined>(pr, k1.data(), k2.data(), m12.data(), P3D.data(), ini.mvInvLevelSigma2.data(), ini.mvScaleFactors.data(),
                                                 nlevels, want, wpts.data(), nullptr);

    // ---- the drop-in
    const iORB_SLAM::InitialMapT<KeyFrame, MapPoint>::Result got = iORB_SLAM::InitialMapT<KeyFrame, MapPoint>::Run(h, &ini, &cur, ini.mnId == 0);
    CHECKF(got.verdict == want.verdict, "n %d seed %u: verdict %d, want %d", n, seed, got.verdict, want.verdict);
    CHECK(memcmp(&got.medianDepth, &want.medianDepth, 4) == 0 && memcmp(&got.invMedianDepth, &want.invMedianDepth, 4) == 0);
    CHECK(got.ba.n_points == n && want.nPoints == n && got.ba.iterations == want.iterations && got.ba.trials == want.trials && got.ba.stop == want.stop);
    const bool ok = want.verdict == initmap_ref::kOk;
    float rows[12];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) rows[4 * r + c] = ini.Tcw.at<float>(r, c);
    CHECK(sameBits(rows, want.Tcw1, 12) && sameBits(ini.Ow, want.Ow1, 3) && ini.nSetPose == 1);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) rows[4 * r + c] = cur.Tcw.at<float>(r, c);
    CHECK(sameBits(rows, ok ? want.Tcw2Scaled : want.Tcw2, 12) && cur.nSetPose == (ok ? 2 : 1));
    CHECK(cur.Tcw.at<float>(3, 3) == 1.f && cur.Tcw.at<float>(3, 0) == 0.f);
    int seen = 0;
    for (int i = 0; i < n1; i++) {
        MapPoint* mp = ini.mvpMapPoints[(size_t)i];
        CHECK((mp != nullptr) == (wpts[(size_t)i].matched != 0));
        if (!mp) continue;
        seen++;
        const initmap_ref::Point& w = wpts[(size_t)i];
        const float P[3] = {mp->mWorldPos.at<float>(0, 0), mp->mWorldPos.at<float>(1, 0), mp->mWorldPos.at<float>(2, 0)};
        CHECKF(sameBits(P, ok ? w.posScaled : w.pos, 3), "n %d seed %u: position of feature %d", n, seed, i);
        CHECKF(sameBits(mp->normal, w.normal, 3) && sameBits(&mp->mfMinDistance, &w.minDistance, 1) && sameBits(&mp->mfMaxDistance, &w.maxDistance, 1),
               "n %d seed %u: normal / bounds of feature %d", n, seed, i);
        CHECK(mp->nUpdates == 1 && w.status == initmap_ref::kStDone);
    }
    CHECK(seen == n);
    return 0;
}

int main()
{
    orbm_t* h = nullptr;
    OX(orbm_create(0, &h));
    const int sizes[5] = {130, 89, 64, 200, 1};
    for (int i = 0; i < 5; i++)
        for (unsigned seed = 1; seed <= 2; seed++) {
            if (one(h, sizes[i], 77u * seed + (unsigned)i, seed == 1, false)) return 1;
        }
    if (one(h, 150, 5u, true, true)) return 1;   // behind the cameras: the reset of a negative median, nothing rescaled
    // a refusal throws and touches nothing
    {
        KeyFrame a, b;
        a.mvScaleFactors.assign(8, 1.f); a.mvInvLevelSigma2.assign(8, 1.f);
        b.mvScaleFactors = a.mvScaleFactors; b.mvInvLevelSigma2 = a.mvInvLevelSigma2;
        a.Tcw.at<float>(0, 0) = NAN;
        bool threw = false;
        try { iORB_SLAM::InitialMapT<KeyFrame, MapPoint>::Run(h, &a, &b, true); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("InitialMap(HIP)") != std::string::npos; }
        CHECK(threw && a.nSetPose == 0 && b.nSetPose == 0);
    }
    orbm_destroy(h);
    if (!fails) printf("initmap dropin ok\n");
    return fails ? 1 : 0;
}
