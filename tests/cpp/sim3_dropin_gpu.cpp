// sim3_dropin_gpu.cpp -- Sim3SolverT (include/Sim3Solver_hip.hpp) on mock keyframes (tests/cpp/mock_slam.hpp) through
// MultiMapper::Run's round-robin loop (iterate(5) over the candidates in turn, here until all have run out) against the
// restatement (tools/sim3_ref.hpp): every iterate's outputs equal as bits, and the process's rand() stream after RunAll
// sits where INTEGRATION.md §4f says: behind ALL mRansacMaxIts sets of every solver.  Needs a GPU; run by tests/test_gpu_sim3.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "Sim3Solver_hip.hpp"
#include "mock_slam.hpp"
#include "dropin_test.hpp"
#include "../../tools/sim3_ref.hpp"

typedef iORB_SLAM::Sim3SolverT<mock::KeyFrame, mock::MapPoint, Mat32, Random> Solver;

struct World {
    std::vector<std::unique_ptr<mock::MapPoint> > pts;
    std::vector<std::unique_ptr<mock::KeyFrame> > kfs;
};

static mock::KeyFrame* newKF(World& w, int nkeys, unsigned& s)
{
    w.kfs.emplace_back(new mock::KeyFrame());
    mock::KeyFrame* kf = w.kfs.back().get();
    kf->fx = 517.3f; kf->fy = 516.5f; kf->cx = 318.6f; kf->cy = 255.3f;
    kf->N = nkeys;
    kf->mvKeysUn.resize(nkeys);
    for (int i = 0; i < nkeys; i++) { kf->mvKeysUn[i].octave = (int)(urand(s) * 8) % 8; kf->mvKeysUn[i].pt.x = (float)(640 * urand(s)); kf->mvKeysUn[i].pt.y = (float)(480 * urand(s)); }
    float s2 = 1.f;
    for (int l = 0; l < 8; l++) { kf->mvLevelSigma2.push_back(s2); s2 *= 1.44f; }
    kf->mvpMapPoints.assign(nkeys, nullptr);
    return kf;
}
static mock::MapPoint* newMP(World& w, const double X[3])
{
    w.pts.emplace_back(new mock::MapPoint());
    mock::MapPoint* p = w.pts.back().get();
    for (int r = 0; r < 3; r++) p->mWorldPos.at<float>(r, 0) = (float)X[r];
    return p;
}

// the restatement's solver from the same keyframes, by the reference's walk
static sim3_ref::Sim3Solver* refSolver(mock::KeyFrame* k1, mock::KeyFrame* k2, const std::vector<mock::MapPoint*>& m12, bool fix)
{
    std::vector<int32_t> idx1;
    std::vector<float> X1, X2, s1, s2;
    std::vector<mock::MapPoint*> mp1 = k1->GetMapPointMatches();
    for (int i = 0; i < (int)m12.size(); i++) {
        if (!m12[i] || !mp1[i] || mp1[i]->isBad() || m12[i]->isBad()) continue;
        const int i1 = mp1[i]->GetIndexInKeyFrame(k1), i2 = m12[i]->GetIndexInKeyFrame(k2);
        if (i1 < 0 || i2 < 0) continue;
        idx1.push_back(i);
        s1.push_back(k1->mvLevelSigma2[k1->mvKeysUn[i1].octave]);
        s2.push_back(k2->mvLevelSigma2[k2->mvKeysUn[i2].octave]);
        for (int r = 0; r < 3; r++) { X1.push_back(mp1[i]->mWorldPos.at<float>(r, 0)); X2.push_back(m12[i]->mWorldPos.at<float>(r, 0)); }
    }
    float R1[9], t1[3], R2[9], t2[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { R1[3 * r + c] = k1->Tcw.at<float>(r, c); R2[3 * r + c] = k2->Tcw.at<float>(r, c); }
        t1[r] = k1->Tcw.at<float>(r, 3); t2[r] = k2->Tcw.at<float>(r, 3);
    }
    const float K1[4] = {k1->fx, k1->fy, k1->cx, k1->cy}, K2[4] = {k2->fx, k2->fy, k2->cx, k2->cy};
    return new sim3_ref::Sim3Solver((int)m12.size(), idx1.data(), (int)idx1.size(), X1.data(), X2.data(), R1, t1, R2, t2, K1, K2, s1.data(), s2.data(), fix);
}

int main()
{
    unsigned s = 12345;
    World w;
    const int nkeys = 400;
    mock::KeyFrame* cur = newKF(w, nkeys, s);
    setPoseEuler(*cur, 0.05, -0.1, 0.02, 0.3, -0.2, 0.5);
    // the current keyframe sees nkeys points of map A; each candidate keyframe lives in map B = a similarity of map A
    std::vector<double> XA((size_t)nkeys * 3);
    for (int i = 0; i < nkeys; i++) {
        const double Xc[3] = {-2 + 4 * urand(s), -1.5 + 3 * urand(s), 4 + 5 * urand(s)};
        // world = R^T (Xc - t)
        for (int r = 0; r < 3; r++) {
            double v = 0;
            for (int c = 0; c < 3; c++) v += cur->Tcw.at<float>(c, r) * (Xc[c] - cur->Tcw.at<float>(c, 3));
            XA[(size_t)i * 3 + r] = v;
        }
        mock::MapPoint* p = newMP(w, &XA[(size_t)i * 3]);
        cur->mvpMapPoints[i] = p;
        p->AddObservation(cur, i);
    }
    const int nCand = 4;
    const double scaleB = 1.7, tB[3] = {5.0, -2.0, 1.0};
    std::vector<mock::KeyFrame*> cands;
    std::vector<std::vector<mock::MapPoint*> > matched(nCand);
    for (int c = 0; c < nCand; c++) {
        mock::KeyFrame* kf = newKF(w, nkeys, s);
        setPoseEuler(*kf, 0.02 * c, 0.3 - 0.1 * c, -0.05, -8.0 + c, 3.0, -1.0 + 0.5 * c);
        cands.push_back(kf);
        matched[c].assign(nkeys, nullptr);
        // candidate c matches 60 + 50 c of the current keyframe's points; the share of wrong matches grows with c; candidate 0
        // is hopeless (all wrong), candidate 3 has too few usable matches after bad / unobserved points
        const int nm = c == 3 ? 12 : 60 + 50 * c;
        for (int k = 0; k < nm; k++) {
            const int i = (int)(urand(s) * nkeys) % nkeys;
            if (matched[c][i]) continue;
            int src = i;
            if (c == 0 || urand(s) < 0.15 * c) src = (int)(urand(s) * nkeys) % nkeys;
            double XB[3];
            for (int r = 0; r < 3; r++) XB[r] = scaleB * XA[(size_t)src * 3 + r] + tB[r] + 0.002 * (urand(s) - 0.5);
            mock::MapPoint* p = newMP(w, XB);
            const int slot = (int)(urand(s) * nkeys) % nkeys;
            if (urand(s) < 0.9) { kf->mvpMapPoints[slot] = p; p->AddObservation(kf, slot); }   // (else: not observed in the candidate -> skipped)
            if (urand(s) < 0.05) p->mbBad = true;
            matched[c][i] = p;
        }
    }

    // (the first use of the device in a process initialises the HIP runtime, which may itself call rand(): do it before seeding)
    { Solver warm(cur, cands[1], matched[1], true); }
    for (int fix = 0; fix < 2; fix++) {
        const unsigned seed = 77 + fix;
        // ---- the adapter, as MultiMapper::Run uses it
        srand(seed);
        std::vector<std::unique_ptr<Solver> > solvers;
        std::vector<Solver*> list;
        for (int c = 0; c < nCand; c++) {
            solvers.emplace_back(new Solver(cur, cands[c], matched[c], fix != 0));
            solvers.back()->SetRansacParameters(0.99, 20, 300);
            list.push_back(solvers.back().get());
        }
        Solver::RunAll(list);
        const int after = rand();
        // the documented position: behind 3 draws for each of ALL mRansacMaxIts sets of every solver that can draw
        srand(seed);
        long draws = 0;
        for (int c = 0; c < nCand; c++) if (list[c]->correspondences() >= 20) draws += 3L * list[c]->maxIterations();
        for (long k = 0; k < draws; k++) (void)rand();
        CHECK(rand() == after);
        // ---- the restatement with the sets drawn the same way
        srand(seed);
        std::vector<std::unique_ptr<sim3_ref::Sim3Solver> > refs;
        std::vector<std::vector<int32_t> > rsets(nCand);
        for (int c = 0; c < nCand; c++) {
            refs.emplace_back(refSolver(cur, cands[c], matched[c], fix != 0));
            refs.back()->SetRansacParameters(0.99, 20, 300);
            CHECK(refs.back()->size() == list[c]->correspondences());
            CHECK(refs.back()->maxIterations() == list[c]->maxIterations());
            if (refs.back()->size() >= 20) {
                rsets[c] = sim3_ref::drawSets(refs.back()->size(), refs.back()->maxIterations());
                CHECK(rsets[c] == list[c]->sets());
            }
        }
        // ---- MultiMapper::Run's loop (MultiMapper.cc: while(nCandidates>0 && !bMatch) over iterate(5))
        std::vector<bool> discarded(nCand, false);
        int nCandidates = nCand, calls = 0, returns = 0;
        bool bMatch = false;
        while (nCandidates > 0) {   // (the reference also stops at bMatch; here every candidate is driven until it runs out)
            for (int i = 0; i < nCand; i++) {
                if (discarded[i]) continue;
                int nInliers = -1;
                bool bNoMore = false;
                std::vector<bool> vbInliers;
                Mat32 Scm = list[i]->iterate(5, bNoMore, vbInliers, nInliers);
                sim3_ref::Result rr;
                std::vector<uint8_t> rin(nkeys, 0);
                refs[i]->iterate(5, rsets[i].data(), rr, rin.data(), nullptr);
                calls++;
                CHECK(bNoMore == (rr.noMore != 0));
                CHECK(nInliers == rr.nInliers);
                CHECK(Scm.empty() == (rr.returned == 0));
                CHECK((int)vbInliers.size() == nkeys);
                for (int k = 0; k < nkeys; k++) CHECK(vbInliers[k] == (rin[k] != 0));
                if (!Scm.empty()) CHECK(memcmp(Scm.d.data(), rr.T12, 64) == 0);
                const Mat32 R = list[i]->GetEstimatedRotation(), t = list[i]->GetEstimatedTranslation();
                CHECK(R.empty() == (rr.hasBest == 0));
                if (!R.empty()) {
                    CHECK(memcmp(R.d.data(), rr.bestR, 36) == 0 && memcmp(t.d.data(), rr.bestT, 12) == 0 && t.rows == 3 && t.cols == 1);
                    const float sc = list[i]->GetEstimatedScale();
                    CHECK(memcmp(&sc, &rr.bestS, 4) == 0);
                }
                if (bNoMore) { discarded[i] = true; nCandidates--; }
                if (!Scm.empty()) {
                    returns++;
                    // (the reference would now run SearchBySim3 and OptimizeSim3; a candidate with over 50 inliers ends the loop here)
                    if (nInliers >= 50) bMatch = true;
                }
            }
        }
        CHECK(calls > nCand);
        if (!fix) CHECK(bMatch && returns >= 1);   // (map B is map A at scale 1.7: a fixed-scale solver finds nothing, as the restatement agrees)
        CHECK(discarded[3]);   // too few correspondences: bNoMore at its first iterate
        printf("fix %d: %d iterate calls, %d returns, sizes %d %d %d %d\n", fix, calls, returns, list[0]->correspondences(), list[1]->correspondences(),
               list[2]->correspondences(), list[3]->correspondences());
    }
    // without RunAll the first iterate runs the solver's own
    {
        srand(5);
        Solver a(cur, cands[2], matched[2], false);
        a.SetRansacParameters(0.99, 20, 300);
        std::vector<bool> in;
        int n = 0;
        Mat32 T = a.find(in, n);
        srand(5);
        std::unique_ptr<sim3_ref::Sim3Solver> r(refSolver(cur, cands[2], matched[2], false));
        r->SetRansacParameters(0.99, 20, 300);
        const std::vector<int32_t> st = sim3_ref::drawSets(r->size(), r->maxIterations());
        sim3_ref::Result rr;
        std::vector<uint8_t> rin(nkeys, 0);
        r->find(st.data(), rr, rin.data(), nullptr);
        CHECK(!T.empty() && rr.returned && memcmp(T.d.data(), rr.T12, 64) == 0 && n == rr.nInliers);
    }
    if (fails) { printf("sim3 dropin: %d checks FAILED\n", fails); return 1; }
    printf("sim3 dropin ok\n");
    return 0;
}
