// pnp_dropin_gpu.cpp -- PnPsolverT (include/PnPsolver_hip.hpp) on a mock frame and mock map points (tests/cpp/mock_slam.hpp)
// through Tracking::Relocalization's round-robin loop (iterate(5) over the live candidates in turn, here until each has run
// out or reached mRansacMaxIts) against the restatement (tools/pnp_ref.hpp): every iterate's outputs equal as bits, and
// the process's rand() stream after RunAll sits where INTEGRATION.md §4g says: behind ALL mRansacMaxIts + 4 sets of every
// solver that can draw.  Needs a GPU; run by tests/test_gpu_pnp.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "PnPsolver_hip.hpp"
#include "mock_slam.hpp"
#include "dropin_test.hpp"
#include "../../tools/pnp_ref.hpp"

namespace pmock {
// mock::Frame has no mvLevelSigma2 (Frame.h:150); the template binds to it
struct Frame : mock::Frame {
    std::vector<float> mvLevelSigma2;
};
}  // namespace pmock

typedef iORB_SLAM::PnPsolverT<pmock::Frame, mock::MapPoint, Mat32, Random> Solver;

// the restatement's solver from the same frame, by the reference's walk
static pnp_ref::PnPsolver* refSolver(const pmock::Frame& F, const std::vector<mock::MapPoint*>& m)
{
    std::vector<int32_t> idx;
    std::vector<float> p2d, s2, p3d;
    for (int i = 0; i < (int)m.size(); i++) {
        if (!m[i] || m[i]->isBad()) continue;
        idx.push_back(i);
        p2d.push_back(F.mvKeysUn[i].pt.x); p2d.push_back(F.mvKeysUn[i].pt.y);
        s2.push_back(F.mvLevelSigma2[F.mvKeysUn[i].octave]);
        for (int r = 0; r < 3; r++) p3d.push_back(m[i]->mWorldPos.at<float>(r, 0));
    }
    const float K[4] = {F.fx, F.fy, F.cx, F.cy};
    return new pnp_ref::PnPsolver((int)m.size(), idx.data(), (int)idx.size(), p2d.data(), s2.data(), p3d.data(), K);
}

int main()
{
    unsigned s = 4242;
    const int nkeys = 500;
    pmock::Frame F;
    mock::Frame::fx = 517.3f; mock::Frame::fy = 516.5f; mock::Frame::cx = 318.6f; mock::Frame::cy = 255.3f;
    F.N = nkeys;
    F.mvKeysUn.resize(nkeys);
    float s2 = 1.f;
    for (int l = 0; l < 8; l++) { F.mvLevelSigma2.push_back(s2); s2 *= 1.44f; }
    // the frame's true pose and the map points its keys see
    const double ax = 0.05, ay = -0.2, az = 0.03, t[3] = {0.3, -0.1, 0.4};
    double R[9];
    eulerR(ax, ay, az, R);
    std::vector<std::unique_ptr<mock::MapPoint> > pts;
    std::vector<mock::MapPoint*> seen(nkeys);
    for (int i = 0; i < nkeys; i++) {
        const double z = 4 + 5 * urand(s), Xc[3] = {(-0.4 + 0.8 * urand(s)) * z, (-0.3 + 0.6 * urand(s)) * z, z};
        pts.emplace_back(new mock::MapPoint());
        for (int r = 0; r < 3; r++) {
            double v = 0;
            for (int c = 0; c < 3; c++) v += R[3 * c + r] * (Xc[c] - t[c]);
            pts.back()->mWorldPos.at<float>(r, 0) = (float)v;
        }
        seen[i] = pts.back().get();
        F.mvKeysUn[i].octave = (int)(urand(s) * 8) % 8;
        F.mvKeysUn[i].pt.x = (float)(517.3 * Xc[0] / z + 318.6 + 0.6 * (urand(s) - 0.5));
        F.mvKeysUn[i].pt.y = (float)(516.5 * Xc[1] / z + 255.3 + 0.6 * (urand(s) - 0.5));
    }
    // four candidates' vpMapPointMatches: 0 hopeless (all wrong), 1 and 2 good with 15 / 30 % wrong, 3 too few matches
    const int nCand = 4;
    std::vector<std::vector<mock::MapPoint*> > matches(nCand, std::vector<mock::MapPoint*>(nkeys, nullptr));
    for (int c = 0; c < nCand; c++) {
        const int nm = c == 3 ? 8 : 60 + 40 * c;
        for (int k = 0; k < nm; k++) {
            const int i = (int)(urand(s) * nkeys) % nkeys;
            int src = i;
            if (c == 0 || urand(s) < 0.15 * c) src = (int)(urand(s) * nkeys) % nkeys;
            matches[c][i] = seen[src];
        }
    }
    seen[7]->mbBad = true;

    // (the first use of the device in a process initialises the HIP runtime, which may itself call rand(): do it before seeding)
    { Solver warm(F, matches[1]); }
    const unsigned seed = 91;
    // ---- the adapter, as Tracking::Relocalization uses it (a discarded candidate leaves a null entry)
    srand(seed);
    std::vector<std::unique_ptr<Solver> > solvers;
    std::vector<Solver*> list;
    for (int c = 0; c < nCand; c++) {
        solvers.emplace_back(new Solver(F, matches[c]));
        solvers.back()->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        list.push_back(solvers.back().get());
    }
    std::vector<Solver*> withNull = list;
    withNull.insert(withNull.begin() + 1, nullptr);
    Solver::RunAll(withNull);
    const int after = rand();
    srand(seed);
    long draws = 0;
    for (int c = 0; c < nCand; c++)
        if (list[c]->correspondences() >= list[c]->minInliers()) draws += 4L * (list[c]->maxIterations() + Solver::kExtraSets);
    for (long k = 0; k < draws; k++) (void)rand();
    CHECK(rand() == after);
    // ---- the restatement with the sets drawn the same way
    srand(seed);
    std::vector<std::unique_ptr<pnp_ref::PnPsolver> > refs;
    std::vector<std::vector<int32_t> > rsets(nCand);
    for (int c = 0; c < nCand; c++) {
        refs.emplace_back(refSolver(F, matches[c]));
        refs.back()->SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
        CHECK(refs.back()->size() == list[c]->correspondences());
        CHECK(refs.back()->maxIterations() == list[c]->maxIterations() && refs.back()->minInliers() == list[c]->minInliers());
        if (refs.back()->size() >= refs.back()->minInliers()) {
            rsets[c] = pnp_ref::drawSets(refs.back()->size(), refs.back()->maxIterations() + Solver::kExtraSets);
            CHECK(rsets[c] == list[c]->sets());
        }
    }
    // ---- Tracking::Relocalization's loop (Tracking.cc:1467-1550: while(nCandidates>0 && !bMatch) over iterate(5))
    std::vector<bool> discarded(nCand, false);
    int nCandidates = nCand, calls = 0, returns = 0;
    while (nCandidates > 0) {   // (the reference also stops at bMatch; here every candidate is driven to its end)
        for (int i = 0; i < nCand; i++) {
            if (discarded[i]) continue;
            int nInliers = -1;
            bool bNoMore = false;
            std::vector<bool> vbInliers;
            Mat32 Tcw = list[i]->iterate(5, bNoMore, vbInliers, nInliers);
            pnp_ref::Result rr;
            std::vector<uint8_t> rin(nkeys, 0);
            const int rc = refs[i]->iterate(5, rsets[i].data(), (int)rsets[i].size() / 4, rr, rin.data(), nullptr);
            calls++;
            CHECK(rc == 0);
            CHECK(bNoMore == (rr.no_more != 0));
            CHECK(nInliers == rr.n_inliers);
            CHECK(Tcw.empty() == (rr.returned == 0));
            if (!Tcw.empty()) {
                CHECK((int)vbInliers.size() == nkeys);
                for (int k = 0; k < nkeys && k < (int)vbInliers.size(); k++) CHECK(vbInliers[k] == (rin[k] != 0));
                CHECK(memcmp(Tcw.d.data(), rr.Tcw, 64) == 0);
                returns++;
            } else
                CHECK(vbInliers.empty());
            CHECK(list[i]->lastResult().iterations == rr.iterations && list[i]->lastResult().best_inliers == rr.best_inliers);
            if (bNoMore || rr.iterations >= refs[i]->maxIterations()) { discarded[i] = true; nCandidates--; }
        }
    }
    CHECK(calls > nCand && returns >= 2);
    CHECK(list[3]->correspondences() < list[3]->minInliers());   // too few correspondences: bNoMore at its first iterate
    printf("%d iterate calls, %d returns, sizes %d %d %d %d\n", calls, returns, list[0]->correspondences(), list[1]->correspondences(),
           list[2]->correspondences(), list[3]->correspondences());
    // without RunAll the first iterate runs the solver's own; find is iterate(mRansacMaxIts)
    {
        srand(5);
        Solver a(F, matches[2]);
        a.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        std::vector<bool> in;
        int n = 0;
        Mat32 T = a.find(in, n);
        srand(5);
        std::unique_ptr<pnp_ref::PnPsolver> r(refSolver(F, matches[2]));
        r->SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
        const std::vector<int32_t> st = pnp_ref::drawSets(r->size(), r->maxIterations() + Solver::kExtraSets);
        pnp_ref::Result rr;
        std::vector<uint8_t> rin(nkeys, 0);
        r->iterate(r->maxIterations(), st.data(), (int)st.size() / 4, rr, rin.data(), nullptr);
        CHECK(!T.empty() && rr.returned && memcmp(T.d.data(), rr.Tcw, 64) == 0 && n == rr.n_inliers);
    }
    // a candidate whose Refine returns the caller rejects (PoseOptimization's nGood < 10: `continue`, Tracking.cc:1494-1501)
    // stays live: a Refine return never sets bNoMore, so iterate(5) is called on and on, far past mRansacMaxIts and past
    // the sets drawn up front.  The adapter draws more and the device continues the table; then find() asks for
    // mRansacMaxIts more.  The restatement gets the sets the adapter ended up with.
    {
        srand(17);
        Solver a(F, matches[1]);
        a.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        struct Out { bool noMore; int n; std::vector<bool> in; std::vector<float> T; int its; };
        std::vector<Out> outs;
        for (int call = 0; call < 41; call++) {
            Out o;
            Mat32 T = call < 40 ? a.iterate(5, o.noMore, o.in, o.n) : a.find(o.in, o.n);
            if (call == 40) o.noMore = a.lastResult().no_more != 0;
            o.T = T.d; o.its = a.lastResult().iterations;
            outs.push_back(o);
        }
        CHECK(outs[39].its > a.maxIterations() + Solver::kExtraSets);
        CHECK((int)a.sets().size() / 4 >= outs[40].its && outs[40].its > outs[39].its);
        std::unique_ptr<pnp_ref::PnPsolver> r(refSolver(F, matches[1]));
        r->SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
        int refined = 0;
        for (int call = 0; call < 41; call++) {
            pnp_ref::Result rr;
            std::vector<uint8_t> rin(nkeys, 0);
            const int rc = r->iterate(call < 40 ? 5 : r->maxIterations(), a.sets().data(), (int)a.sets().size() / 4, rr, rin.data(), nullptr);
            const Out& o = outs[call];
            CHECK(rc == 0 && o.noMore == (rr.no_more != 0) && o.n == rr.n_inliers && o.its == rr.iterations && o.T.empty() == (rr.returned == 0));
            if (!o.T.empty()) {
                CHECK(memcmp(o.T.data(), rr.Tcw, 64) == 0);
                for (int k = 0; k < nkeys; k++) CHECK(o.in[k] == (rin[k] != 0));
                refined += rr.refined;
            }
        }
        CHECK(refined >= 30);
        printf("rejected returns: %d calls to iteration %d of %d, %d sets drawn\n", 41, outs[40].its, a.maxIterations(), (int)a.sets().size() / 4);
    }
    if (fails) { printf("pnp dropin: %d checks FAILED\n", fails); return 1; }
    printf("pnp dropin ok\n");
    return 0;
}
