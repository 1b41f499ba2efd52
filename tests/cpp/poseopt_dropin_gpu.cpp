// poseopt_dropin_gpu.cpp -- PoseOptimizationT (include/Optimizer_hip.hpp) on mock frames and mock map points
// (tests/cpp/mock_poseopt.hpp) against the restatement's Defined mode (tools/poseopt_ref.hpp) run on the same mocks: Run on
// one frame, RunAll on a relocalisation's candidates (a null entry, a frame below 3 observations, one below 10 among them),
// the return values, mvbOutlier and the pose SetPose got equal as bits; a stereo observation refused.  Needs a GPU; run by
// tests/test_gpu_poseopt.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "Optimizer_hip.hpp"
#include "mock_poseopt.hpp"
#include "dropin_test.hpp"
#include "../../tools/poseopt_ref.hpp"

typedef iORB_SLAM::PoseOptimizationT<pomock::Frame, mock::MapPoint> PoseOpt;


struct Scene {
    pomock::Frame F;
    std::vector<std::unique_ptr<mock::MapPoint> > pts;
};

// nkeys keys, every `every`-th of the first `limit` matched to a map point seen under a true pose; a share of them wrong
static void makeScene(Scene& S, unsigned seed, int nkeys, int every, int limit, double wrong)
{
    unsigned s = seed;
    pomock::Frame& F = S.F;
    F.N = nkeys;
    F.mvKeysUn.resize(nkeys);
    F.mvuRight.assign(nkeys, -1.f);
    F.mvpMapPoints.assign(nkeys, nullptr);
    F.mvbOutlier.assign(nkeys, true);   // (stale flags: the function clears those of its observations)
    float s2 = 1.f;
    for (int l = 0; l < 8; l++) { F.mvInvLevelSigma2.push_back(1.f / s2); s2 *= 1.44f; }
    const double ax = 0.05 + 0.1 * urand(s), ay = -0.2, az = 0.03, t[3] = {0.3, -0.1, 0.4};
    double R[9];
    eulerR(ax, ay, az, R);
    for (int i = 0; i < nkeys; i++) {
        const double z = 3 + 5 * urand(s), Xc[3] = {(-0.4 + 0.8 * urand(s)) * z, (-0.3 + 0.6 * urand(s)) * z, z};
        F.mvKeysUn[i].octave = (int)(urand(s) * 8) % 8;
        F.mvKeysUn[i].pt.x = (float)(517.3 * Xc[0] / z + 318.6 + 0.8 * (urand(s) - 0.5));
        F.mvKeysUn[i].pt.y = (float)(516.5 * Xc[1] / z + 255.3 + 0.8 * (urand(s) - 0.5));
        if (i % every || i >= limit) continue;
        S.pts.emplace_back(new mock::MapPoint());
        const bool bad = urand(s) < wrong;
        for (int r = 0; r < 3; r++) {
            double v = 0;
            for (int c = 0; c < 3; c++) v += R[3 * c + r] * (Xc[c] - t[c]);
            S.pts.back()->mWorldPos.at<float>(r, 0) = (float)(bad ? v + 1.0 + urand(s) : v);
        }
        F.mvpMapPoints[i] = S.pts.back().get();
    }
    // the start pose: the true one, a little off
    double Rs[9];
    eulerR(ax + 0.02, ay - 0.015, az, Rs);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) F.mTcw.at<float>(r, c) = (float)Rs[3 * r + c];
        F.mTcw.at<float>(r, 3) = (float)(t[r] + 0.03 * (r - 1));
    }
    F.mTcw.at<float>(3, 3) = 1.f;
}

// the restatement on the same mock, by the reference's walk
static int refRun(const pomock::Frame& F, poseopt_ref::Result& res, std::vector<uint8_t>& outlier, std::vector<int>& feature)
{
    std::vector<poseopt_ref::Edge> edges;
    feature.clear();
    for (int i = 0; i < F.N; i++) {
        mock::MapPoint* p = F.mvpMapPoints[i];
        if (!p) continue;
        poseopt_ref::Edge e;
        e.u = F.mvKeysUn[i].pt.x; e.v = F.mvKeysUn[i].pt.y;
        e.invSigma2 = F.mvInvLevelSigma2[F.mvKeysUn[i].octave];
        for (int r = 0; r < 3; r++) e.Xw[r] = p->mWorldPos.at<float>(r, 0);
        edges.push_back(e);
        feature.push_back(i);
    }
    poseopt_ref::Frame rf;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) rf.Tcw[4 * r + c] = F.mTcw.at<float>(r, c);
    rf.K[0] = mock::Frame::fx; rf.K[1] = mock::Frame::fy; rf.K[2] = mock::Frame::cx; rf.K[3] = mock::Frame::cy;
    outlier.assign(edges.size() + 1, 0);
    poseopt_ref::poseOptimization<poseopt_ref::Defined>(rf, edges.data(), (int)edges.size(), res, outlier.data(), nullptr);
    return res.nGood;
}

static void compare(pomock::Frame& F, int ret, int wantRet, const poseopt_ref::Result& res, const std::vector<uint8_t>& outlier,
                    const std::vector<int>& feature, const std::vector<bool>& before)
{
    CHECK(ret == wantRet);
    float T[16];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[4 * r + c] = F.mTcw.at<float>(r, c);
    CHECK(memcmp(T, res.Tcw, 64) == 0);
    CHECK(F.setPoseCalls == (res.rounds > 0 ? 1 : 0));
    std::vector<bool> want = before;
    for (size_t k = 0; k < feature.size(); k++) want[feature[k]] = outlier[k] != 0;
    CHECK(F.mvbOutlier == want);   // (the flags of unmatched features stay as they were)
}

int main()
{
    mock::Frame::fx = 517.3f; mock::Frame::fy = 516.5f; mock::Frame::cx = 318.6f; mock::Frame::cy = 255.3f;
    // ---- Run: one frame, 500 keys, 250 observations, a fifth wrong
    {
        Scene S;
        makeScene(S, 77, 500, 2, 500, 0.2);
        poseopt_ref::Result res;
        std::vector<uint8_t> outl;
        std::vector<int> feat;
        const int want = refRun(S.F, res, outl, feat);
        const std::vector<bool> before = S.F.mvbOutlier;
        const int got = PoseOpt::Run(&S.F);
        compare(S.F, got, want, res, outl, feat, before);
        CHECK(res.rounds == 4 && want > 150 && want < 250);
        printf("Run: %d observations, %d good\n", (int)feat.size(), got);
    }
    // ---- RunAll: relocalisation's candidates -- good, a null entry, 2 observations, 8 observations, hopeless
    {
        std::vector<std::unique_ptr<Scene> > scenes;
        const int every[4] = {3, 1, 1, 2}, limit[4] = {600, 2, 8, 400};
        const double wrong[4] = {0.1, 0.0, 0.0, 1.0};
        std::vector<pomock::Frame*> list;
        for (int c = 0; c < 4; c++) {
            scenes.emplace_back(new Scene());
            makeScene(*scenes.back(), 100 + c, 600, every[c], limit[c], wrong[c]);
            list.push_back(&scenes.back()->F);
        }
        list.insert(list.begin() + 1, nullptr);
        std::vector<poseopt_ref::Result> res(5);
        std::vector<std::vector<uint8_t> > outl(5);
        std::vector<std::vector<int> > feat(5);
        std::vector<std::vector<bool> > before(5);
        std::vector<int> want(5, 0);
        for (int k = 0; k < 5; k++) if (list[k]) { want[k] = refRun(*list[k], res[k], outl[k], feat[k]); before[k] = list[k]->mvbOutlier; }
        std::vector<OrboResult> raw;
        const std::vector<int> got = PoseOpt::RunAll(list, 0, &raw);
        CHECK(got.size() == 5 && got[1] == 0);
        for (int k = 0; k < 5; k++) {
            if (!list[k]) continue;
            compare(*list[k], got[k], want[k], res[k], outl[k], feat[k], before[k]);
            CHECK(raw[k].rounds == res[k].rounds && raw[k].n_initial == res[k].nInitial);
            CHECK(memcmp(raw[k].iterations, res[k].iterations, 16) == 0 && memcmp(raw[k].trials, res[k].trials, 16) == 0);
            CHECK(memcmp(raw[k].lambda, res[k].lambda, 32) == 0 && memcmp(raw[k].chi2, res[k].chi2, 32) == 0);
        }
        CHECK(res[2].rounds == 0 && got[2] == 0 && res[3].rounds == 1 && res[0].rounds == 4 && res[4].rounds == 4);
        printf("RunAll: good %d %d %d %d\n", got[0], got[2], got[3], got[4]);
    }
    // ---- a stereo observation is refused, and says so
    {
        Scene S;
        makeScene(S, 5, 60, 1, 60, 0.0);
        S.F.mvuRight[40] = 123.f;
        const std::vector<bool> before = S.F.mvbOutlier;
        bool threw = false;
        try { PoseOpt::Run(&S.F); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("stereo") != std::string::npos; }
        CHECK(threw && S.F.setPoseCalls == 0);
        CHECK(S.F.mvbOutlier == before);   // (the flags of the features before the offending one included)
        // RunAll: a good frame ahead of a refused one is left as it came, too
        Scene G, B;
        makeScene(G, 6, 60, 1, 60, 0.0);
        makeScene(B, 7, 60, 1, 60, 0.0);
        B.F.mvInvLevelSigma2[3] *= 2.f;   // another level table
        const std::vector<bool> gBefore = G.F.mvbOutlier;
        std::vector<pomock::Frame*> two;
        two.push_back(&G.F); two.push_back(&B.F);
        threw = false;
        try { PoseOpt::RunAll(two); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && G.F.setPoseCalls == 0 && B.F.setPoseCalls == 0 && G.F.mvbOutlier == gBefore);
    }
    if (fails) { printf("poseopt dropin: %d checks FAILED\n", fails); return 1; }
    printf("poseopt dropin ok\n");
    return 0;
}
