// sim3opt_dropin_gpu.cpp -- OptimizeSim3T (include/Optimizer_hip.hpp) on mock keyframes, map points (tests/cpp/mock_slam.hpp)
// and a mock g2o::Sim3 (tests/cpp/mock_sim3opt.hpp) against the restatement's Defined mode (tools/sim3opt_ref.hpp) run on the
// same mocks: Run on one candidate, RunAll on a ComputeSim3's candidates (a good one, one that returns early, one without a
// match among them), the return values, the nulled entries of vpMatches1 and the Sim3 equal as bits; the early-return job's Sim3
// object untouched; a stereo observation refused.  Needs a GPU; run by tests/test_gpu_sim3opt.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "Optimizer_hip.hpp"
#include "mock_sim3opt.hpp"
#include "dropin_test.hpp"
#include "../../tools/sim3opt_ref.hpp"

typedef iORB_SLAM::OptimizeSim3T<mock::KeyFrame, mock::MapPoint, s3mock::Sim3> OptSim3;

static bool refOnly = false;   // --ref-only: print the restatement's figures for the scenes and touch no GPU

struct Scene {
    mock::KeyFrame K1, K2;
    std::vector<std::unique_ptr<mock::MapPoint> > pts;
    std::vector<mock::MapPoint*> matches;   // vpMatches1
    s3mock::Sim3 S12;
};

static void setPose(mock::KeyFrame& K, const double R[9], const double t[3])
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) K.Tcw.at<float>(r, c) = (float)R[3 * r + c];
        K.Tcw.at<float>(r, 3) = (float)t[r];
    }
    K.Tcw.at<float>(3, 3) = 1.f;
}

// nkeys features in pKF1, every `every`-th of the first `limit` with a map point of its own AND a match to a map point of pKF2;
// a share of the matches wrong; a few entries the walk has to skip (a bad point, a match pKF2 does not observe)
static void makeScene(Scene& S, unsigned seed, int nkeys, int every, int limit, double wrong)
{
    unsigned s = seed;
    mock::KeyFrame &A = S.K1, &B = S.K2;
    A.N = B.N = nkeys;
    A.mvKeysUn.resize(nkeys); B.mvKeysUn.resize(nkeys);
    A.mvuRight.assign(nkeys, -1.f); B.mvuRight.assign(nkeys, -1.f);
    A.mvpMapPoints.assign(nkeys, nullptr); B.mvpMapPoints.assign(nkeys, nullptr);
    S.matches.assign(nkeys, nullptr);
    A.fx = 517.3f; A.fy = 516.5f; A.cx = 318.6f; A.cy = 255.3f;
    B.fx = 458.7f; B.fy = 457.3f; B.cx = 367.2f; B.cy = 248.4f;
    float s2 = 1.f, s3 = 1.f;
    for (int l = 0; l < 8; l++) { A.mvInvLevelSigma2.push_back(1.f / s2); B.mvInvLevelSigma2.push_back(1.f / s3); s2 *= 1.44f; s3 *= 1.69f; }
    double R1[9], R2[9], Rt[9];
    const double t1[3] = {0.3, -0.1, 0.4}, t2[3] = {-0.2, 0.15, 0.1}, tt[3] = {0.1, -0.05, 0.08};
    eulerR(0.05 + 0.1 * urand(s), -0.2, 0.03, R1);
    eulerR(-0.1, 0.15 + 0.1 * urand(s), 0.2, R2);
    eulerR(0.04, -0.06, 0.03, Rt);   // the truth: P1c = Rt P2c + tt, scale 1
    setPose(A, R1, t1);
    setPose(B, R2, t2);
    std::vector<mock::KeyPoint> seen2((size_t)nkeys);   // what pKF2 sees of point i; placed at its own feature index below
    for (int i = 0; i < nkeys; i++) {
        const double z = 3 + 5 * urand(s), P1[3] = {(-0.3 + 0.6 * urand(s)) * z, (-0.25 + 0.5 * urand(s)) * z, z};
        double P2[3];
        for (int r = 0; r < 3; r++) { P2[r] = 0; for (int c = 0; c < 3; c++) P2[r] += Rt[3 * c + r] * (P1[c] - tt[c]); }
        A.mvKeysUn[i].octave = (int)(urand(s) * 8) % 8;
        B.mvKeysUn[i].octave = (int)(urand(s) * 8) % 8;
        A.mvKeysUn[i].pt.x = (float)(517.3 * P1[0] / P1[2] + 318.6 + 0.8 * (urand(s) - 0.5));
        A.mvKeysUn[i].pt.y = (float)(516.5 * P1[1] / P1[2] + 255.3 + 0.8 * (urand(s) - 0.5));
        const bool bad = urand(s) < wrong;
        B.mvKeysUn[i].pt.x = bad ? (float)(640.0 * urand(s)) : (float)(458.7 * P2[0] / P2[2] + 367.2 + 0.8 * (urand(s) - 0.5));
        B.mvKeysUn[i].pt.y = bad ? (float)(480.0 * urand(s)) : (float)(457.3 * P2[1] / P2[2] + 248.4 + 0.8 * (urand(s) - 0.5));
        seen2[(size_t)i] = B.mvKeysUn[i];
        if (i % every || i >= limit) continue;
        S.pts.emplace_back(new mock::MapPoint());
        mock::MapPoint* m1 = S.pts.back().get();
        S.pts.emplace_back(new mock::MapPoint());
        mock::MapPoint* m2 = S.pts.back().get();
        for (int r = 0; r < 3; r++) {
            double v1 = 0, v2 = 0;
            for (int c = 0; c < 3; c++) { v1 += R1[3 * c + r] * (P1[c] - t1[c]); v2 += R2[3 * c + r] * (P2[c] - t2[c]); }
            m1->mWorldPos.at<float>(r, 0) = (float)v1;
            m2->mWorldPos.at<float>(r, 0) = (float)v2;
        }
        A.mvpMapPoints[i] = m1;
        const int i2 = nkeys - 1 - i;   // (pKF2 sees the point at another feature index)
        B.mvpMapPoints[i2] = m2;
        m2->AddObservation(&B, (size_t)i2);
        S.matches[i] = m2;
    }
    for (int i = 0; i < nkeys; i++) if (S.matches[i]) B.mvKeysUn[nkeys - 1 - i] = seen2[(size_t)i];
    // what the walk skips: a bad point of pKF1, a match that pKF2 does not observe, a match without a point in pKF1
    if (limit > 40 * every) {
        A.mvpMapPoints[2 * every]->mbBad = true;
        S.matches[4 * every]->mObservations.clear();
        A.mvpMapPoints[6 * every] = nullptr;
    }
    // the start: the truth a little off
    double Rs[9];
    eulerR(0.05, -0.05, 0.035, Rs);
    double q[4];
    poseopt_ref::quatFromMatrix(Rs, q);
    s3mock::Quaterniond Q;
    s3mock::Vector3d T;
    for (int c = 0; c < 4; c++) Q.coeffs()[c] = q[c];
    for (int c = 0; c < 3; c++) T[c] = tt[c] + 0.02 * (c - 1);
    S.S12 = s3mock::Sim3(Q, T, 1.03);
    S.S12.constructed = 0;
}

// the restatement on the same mocks, by the reference's walk
static int refRun(Scene& S, float th2, bool fix, sim3opt_ref::Result& res, std::vector<uint8_t>& removed, std::vector<int>& idx)
{
    sim3opt_ref::Problem P;
    memset(&P, 0, sizeof P);
    for (int c = 0; c < 4; c++) P.q[c] = S.S12.rotation().coeffs()[c];
    for (int c = 0; c < 3; c++) P.t[c] = S.S12.translation()[c];
    P.s = S.S12.scale();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { P.R1w[3 * r + c] = S.K1.Tcw.at<float>(r, c); P.R2w[3 * r + c] = S.K2.Tcw.at<float>(r, c); }
        P.t1w[r] = S.K1.Tcw.at<float>(r, 3); P.t2w[r] = S.K2.Tcw.at<float>(r, 3);
    }
    P.K1[0] = S.K1.fx; P.K1[1] = S.K1.fy; P.K1[2] = S.K1.cx; P.K1[3] = S.K1.cy;
    P.K2[0] = S.K2.fx; P.K2[1] = S.K2.fy; P.K2[2] = S.K2.cx; P.K2[3] = S.K2.cy;
    P.th2 = th2; P.fixScale = fix ? 1 : 0;
    std::vector<sim3opt_ref::Corr> corrs;
    idx.clear();
    for (size_t i = 0; i < S.matches.size(); i++) {
        mock::MapPoint* m2 = S.matches[i];
        if (!m2) continue;
        mock::MapPoint* m1 = S.K1.mvpMapPoints[i];
        const int i2 = m2->GetIndexInKeyFrame(&S.K2);
        if (!m1 || m1->isBad() || m2->isBad() || i2 < 0) continue;
        sim3opt_ref::Corr c;
        c.obs1[0] = S.K1.mvKeysUn[i].pt.x; c.obs1[1] = S.K1.mvKeysUn[i].pt.y; c.invSigma2_1 = S.K1.mvInvLevelSigma2[S.K1.mvKeysUn[i].octave];
        c.obs2[0] = S.K2.mvKeysUn[i2].pt.x; c.obs2[1] = S.K2.mvKeysUn[i2].pt.y; c.invSigma2_2 = S.K2.mvInvLevelSigma2[S.K2.mvKeysUn[i2].octave];
        for (int r = 0; r < 3; r++) { c.X1w[r] = m1->mWorldPos.at<float>(r, 0); c.X2w[r] = m2->mWorldPos.at<float>(r, 0); }
        corrs.push_back(c);
        idx.push_back((int)i);
    }
    removed.assign(corrs.size() + 1, 0);
    sim3opt_ref::optimizeSim3<sim3opt_ref::Defined>(P, corrs.data(), (int)corrs.size(), res, removed.data(), nullptr);
    return res.nIn;
}

static void compare(Scene& S, int ret, int wantRet, const sim3opt_ref::Result& res, const std::vector<uint8_t>& removed, const std::vector<int>& idx,
                    const std::vector<mock::MapPoint*>& before, const s3mock::Sim3& start)
{
    CHECK(ret == wantRet);
    std::vector<mock::MapPoint*> want = before;
    for (size_t k = 0; k < idx.size(); k++) if (removed[k]) want[idx[k]] = nullptr;
    CHECK(S.matches == want);   // (entries the walk skipped stay as they were)
    double got[8], ref[8], was[8];
    for (int c = 0; c < 4; c++) { got[c] = S.S12.rotation().coeffs()[c]; ref[c] = res.q[c]; was[c] = start.rotation().coeffs()[c]; }
    for (int c = 0; c < 3; c++) { got[4 + c] = S.S12.translation()[c]; ref[4 + c] = res.t[c]; was[4 + c] = start.translation()[c]; }
    got[7] = S.S12.scale(); ref[7] = res.s; was[7] = start.scale();
    CHECK(memcmp(got, ref, sizeof got) == 0);
    CHECK(S.S12.constructed == (res.written ? 1 : 0));   // the early return leaves the object untouched
    if (!res.written) CHECK(memcmp(got, was, sizeof got) == 0);
}

int main(int argc, char** argv)
{
    refOnly = argc > 1 && std::string(argv[1]) == "--ref-only";
    // ---- Run: one candidate, 600 keys, 200 matches, a fifth wrong; free scale, then fixed scale
    for (int fix = 0; fix < 2; fix++) {
        Scene S;
        makeScene(S, 77 + fix, 600, 3, 600, 0.2);
        sim3opt_ref::Result res;
        std::vector<uint8_t> rem;
        std::vector<int> idx;
        const int want = refRun(S, 10.f, fix != 0, res, rem, idx);
        const std::vector<mock::MapPoint*> before = S.matches;
        const s3mock::Sim3 start = S.S12;
        const int got = refOnly ? want : OptSim3::Run(&S.K1, &S.K2, S.matches, S.S12, 10.f, fix != 0);
        if (!refOnly) compare(S, got, want, res, rem, idx, before, start);
        CHECK(res.written == 1 && (int)idx.size() == 197 && want > 100 && want < 190);
        if (fix) CHECK(S.S12.scale() == start.scale());
        printf("Run (fix_scale %d): %d correspondences, %d bad, %d in\n", fix, (int)idx.size(), res.nBad, got);
    }
    // ---- RunAll: the candidates of one ComputeSim3 -- good, hopeless (returns early), no match at all, 8 matches
    {
        std::vector<std::unique_ptr<Scene> > scenes;
        const int every[4] = {2, 2, 1, 1}, limit[4] = {400, 400, 0, 8};
        const double wrong[4] = {0.1, 1.0, 0.0, 0.0};
        std::vector<OptSim3::Job> jobs;
        for (int c = 0; c < 4; c++) {
            scenes.emplace_back(new Scene());
            makeScene(*scenes.back(), 100 + c, 400, every[c], limit[c], wrong[c]);
            Scene& S = *scenes.back();
            OptSim3::Job j;
            j.pKF1 = &S.K1; j.pKF2 = &S.K2; j.vpMatches1 = &S.matches; j.g2oS12 = &S.S12; j.th2 = 10.f; j.bFixScale = c == 3;
            jobs.push_back(j);
        }
        std::vector<sim3opt_ref::Result> res(4);
        std::vector<std::vector<uint8_t> > rem(4);
        std::vector<std::vector<int> > idx(4);
        std::vector<std::vector<mock::MapPoint*> > before(4);
        std::vector<s3mock::Sim3> start(4);
        std::vector<int> want(4, 0);
        for (int k = 0; k < 4; k++) {
            want[k] = refRun(*scenes[k], 10.f, k == 3, res[k], rem[k], idx[k]);
            before[k] = scenes[k]->matches;
            start[k] = scenes[k]->S12;
        }
        std::vector<OrbzResult> raw;
        const std::vector<int> got = refOnly ? want : OptSim3::RunAll(jobs, 0, &raw);
        CHECK(got.size() == 4);
        for (int k = 0; k < 4 && !refOnly; k++) {
            compare(*scenes[k], got[k], want[k], res[k], rem[k], idx[k], before[k], start[k]);
            CHECK(raw[k].written == res[k].written && raw[k].n_corr == res[k].nCorr && raw[k].n_bad == res[k].nBad && raw[k].n_in == res[k].nIn);
            CHECK(memcmp(raw[k].iterations, res[k].iterations, 8) == 0 && memcmp(raw[k].trials, res[k].trials, 8) == 0);
            CHECK(memcmp(raw[k].lambda, res[k].lambda, 16) == 0 && memcmp(raw[k].chi2, res[k].chi2, 16) == 0);
        }
        CHECK(res[0].written == 1 && got[0] >= 20);
        CHECK(res[1].written == 0 && res[1].nBad > 0 && got[1] == 0);   // the early return, with matches nulled
        CHECK(res[2].nCorr == 0 && got[2] == 0 && res[3].nCorr == 8 && res[3].written == 0);
        printf("RunAll: in %d %d %d %d\n", got[0], got[1], got[2], got[3]);
    }
    // ---- a stereo observation is refused, and says so; a job ahead of a refused one is left as it came
    if (!refOnly) {
        Scene G, B;
        makeScene(G, 6, 120, 1, 120, 0.0);
        makeScene(B, 7, 120, 1, 120, 0.0);
        B.K2.mvuRight[119 - 40] = 123.f;   // the feature of pKF2 that match 40 uses
        const std::vector<mock::MapPoint*> gBefore = G.matches, bBefore = B.matches;
        bool threw = false;
        try { OptSim3::Run(&B.K1, &B.K2, B.matches, B.S12, 10.f, false); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("stereo") != std::string::npos; }
        CHECK(threw && B.matches == bBefore && B.S12.constructed == 0);
        std::vector<OptSim3::Job> two(2);
        two[0].pKF1 = &G.K1; two[0].pKF2 = &G.K2; two[0].vpMatches1 = &G.matches; two[0].g2oS12 = &G.S12; two[0].th2 = 10.f; two[0].bFixScale = false;
        two[1].pKF1 = &B.K1; two[1].pKF2 = &B.K2; two[1].vpMatches1 = &B.matches; two[1].g2oS12 = &B.S12; two[1].th2 = 10.f; two[1].bFixScale = false;
        threw = false;
        try { OptSim3::RunAll(two); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && G.matches == gBefore && G.S12.constructed == 0 && B.matches == bBefore);
    }
    if (fails) { printf("sim3opt dropin: %d checks FAILED\n", fails); return 1; }
    printf("sim3opt dropin ok\n");
    return 0;
}
