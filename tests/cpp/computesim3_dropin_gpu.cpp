// computesim3_dropin_gpu.cpp -- ComputeSim3T::RunAll (include/LoopClosing_hip.hpp) on mock keyframes, map points and a mock g2o::Sim3
// (tests/cpp/mock_computesim3.hpp) against the existing class-typed members run per candidate on copies of the same mocks:
// ORBmatcherT::SearchBySim3 followed by OptimizeSim3T::Run.  Three candidates in one call: one with 40 entering matches, one with
// none and a fixed scale, one whose current keyframe holds 8 points (the early return of Optimizer.cc:1514: its Sim3 object
// untouched).  vpMapPointMatches equal pointer for pointer, nFound, nInliers and the Sim3 equal as bits.  Needs a GPU; run by
// tests/test_gpu_computesim3.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "LoopClosing_hip.hpp"
#include "ORBmatcher_hip.hpp"
#include "Optimizer_hip.hpp"
#include "mock_computesim3.hpp"
#include "../../tools/sim3opt_ref.hpp"

typedef mock::KeyFrame KeyFrame;
typedef mock::MapPoint MapPoint;
typedef iORB_SLAM::ORBmatcherT<mock::Frame, KeyFrame, MapPoint> ORBmatcher;
typedef iORB_SLAM::OptimizeSim3T<KeyFrame, MapPoint, s3mock::Sim3> OptSim3;
typedef iORB_SLAM::ComputeSim3T<KeyFrame, MapPoint, s3mock::Sim3> ComputeSim3;

static const int N = 300, CAP = 320, NPAIR = 3;

static s3mock::Sim3 startSim3(const cmock::Pair& P)
{
    double R[9], q[4];
    for (int k = 0; k < 9; k++) R[k] = (double)P.R12[k];
    poseopt_ref::quatFromMatrix(R, q);   // Converter::toMatrix3d(R) into g2o::Sim3's Quaterniond(R)
    s3mock::Quaterniond Q;
    s3mock::Vector3d T;
    for (int c = 0; c < 4; c++) Q.coeffs()[c] = q[c];
    for (int c = 0; c < 3; c++) T[c] = (double)P.t12[c];
    s3mock::Sim3 S(Q, T, (double)P.s12);
    S.constructed = 0;
    return S;
}

int main()
{
    std::vector<std::unique_ptr<cmock::Pair> > pairs;
    const int holds[NPAIR] = {N, N, 8};
    for (int k = 0; k < NPAIR; k++) {
        pairs.emplace_back(new cmock::Pair());
        cmock::makePair(*pairs.back(), 31 + k, N, holds[k], 2 * N * k);
    }
    // what enters: candidate 0 carries 40 inliers of the solver
    std::vector<std::vector<MapPoint*> > entering(NPAIR, std::vector<MapPoint*>(N, nullptr));
    for (int i = 0; i < 40; i++) entering[0][(size_t)(5 * i)] = pairs[0]->K2.mvpMapPoints[(size_t)pairs[0]->true2[(size_t)(5 * i)]];
    // a bad point on either side among candidate 1's
    pairs[1]->K1.mvpMapPoints[10]->mbBad = true;
    pairs[1]->K2.mvpMapPoints[20]->mbBad = true;

    // ---- the device side: six slots, one pool, one store
    orbm_t* m = nullptr;
    orbx_t* ex = nullptr;
    OX(orbm_create(0, &m));
    OrbxParams prm; prm.nfeatures = 1000; prm.scaleFactor = cmock::SCALE; prm.nlevels = cmock::NLEVELS; prm.iniThFAST = 20; prm.minThFAST = 7;
    OX(orbx_create(&prm, cmock::W, cmock::H, 1, 0, &ex));
    orbm_frameset_t* fs = nullptr;
    {
        const KeyFrame& K = pairs[0]->K1;
        const float Kc[4] = {K.fx, K.fy, K.cx, K.cy}, D[5] = {0, 0, 0, 0, 0}, bounds[4] = {0.f, (float)cmock::W, 0.f, (float)cmock::H};
        OrbmGrid g; g.minX = 0.f; g.minY = 0.f; g.invW = K.mfGridElementWidthInv; g.invH = K.mfGridElementHeightInv; g.cols = 64; g.rows = 48;
        OX(orbm_frameset_create(m, 2 * NPAIR, CAP, Kc, D, &g, bounds, K.mvScaleFactors.data(), cmock::NLEVELS, &fs));
    }
    std::vector<void*> mem;
    for (int k = 0; k < NPAIR; k++)
        for (int side = 0; side < 2; side++) {
            KeyFrame& K = side ? pairs[(size_t)k]->K2 : pairs[(size_t)k]->K1;
            void *dk = nullptr, *dd = nullptr, *dn = nullptr;
            OX(orbx_device_alloc(ex, (size_t)N * sizeof(OrbxKeyPoint), &dk));
            OX(orbx_device_alloc(ex, (size_t)N * 32, &dd));
            OX(orbx_device_alloc(ex, 4, &dn));
            mem.push_back(dk); mem.push_back(dd); mem.push_back(dn);
            const int32_t count = N;
            OX(orbx_upload(ex, dk, K.mvKeysUn.data(), (size_t)N * sizeof(OrbxKeyPoint)));
            OX(orbx_upload(ex, dd, K.mDescriptors.ptr<unsigned char>(0), (size_t)N * 32));
            OX(orbx_upload(ex, dn, &count, 4));
            OX(orbm_frameset_build(fs, 2 * k + side, 1, (const OrbxKeyPoint*)dk, (const uint8_t*)dd, (const int32_t*)dn, N));
        }
    OX(orbm_frameset_sync(fs));
    const int npool = 2 * N * NPAIR;
    orbw_pool_t* pool = nullptr;
    orbu_store_t* store = nullptr;
    OX(orbw_pool_create(m, npool, &pool));
    {
        std::vector<int32_t> ids;
        std::vector<OrbwPoint> recs;
        for (int k = 0; k < NPAIR; k++)
            for (size_t i = 0; i < pairs[(size_t)k]->pts.size(); i++) {
                cmock::MapPoint* p = pairs[(size_t)k]->pts[i].get();
                OrbwPoint r;
                memset(&r, 0, sizeof r);
                for (int c = 0; c < 3; c++) r.pos[c] = p->mWorldPos.at<float>(c, 0);
                r.min_distance = p->mfMinDistance; r.max_distance = p->mfMaxDistance;
                memcpy(r.desc, p->mDescriptor.ptr<unsigned char>(0), 32);
                r.flags = (uint8_t)((p->mbBad ? 1 : 0) | 2);
                ids.push_back(p->poolId);
                recs.push_back(r);
            }
        OX(orbw_pool_set(pool, ids.data(), recs.data(), (int)ids.size()));
    }
    OX(orbu_store_create(pool, 2 * NPAIR, N, 0, 16, &store));
    {
        const int nkf = 2 * NPAIR;
        std::vector<int32_t> slot, n, entries, neigh((size_t)nkf * 10, -1), parent((size_t)nkf, -1), nch((size_t)nkf, 0), children(1, 0);
        std::vector<uint8_t> flags((size_t)nkf, 0);
        for (int k = 0; k < NPAIR; k++)
            for (int side = 0; side < 2; side++) {
                KeyFrame& K = side ? pairs[(size_t)k]->K2 : pairs[(size_t)k]->K1;
                slot.push_back(2 * k + side);
                n.push_back(N);
                for (int i = 0; i < N; i++) entries.push_back(K.mvpMapPoints[(size_t)i] ? K.mvpMapPoints[(size_t)i]->id : -1);
            }
        OrbuKeyFrames rec;
        rec.nkf = nkf; rec.slot = slot.data(); rec.flags = flags.data(); rec.n = n.data(); rec.entries = entries.data(); rec.neigh = neigh.data();
        rec.parent = parent.data(); rec.nchildren = nch.data(); rec.children = children.data();
        OX(orbu_kf_set(store, &rec));
    }

    // ---- the existing path, per candidate, on copies of what enters
    std::vector<std::vector<MapPoint*> > want = entering;
    std::vector<s3mock::Sim3> wantS(NPAIR), gotS(NPAIR);
    std::vector<int> wantFound(NPAIR), wantIn(NPAIR);
    for (int k = 0; k < NPAIR; k++) {
        cmock::Pair& P = *pairs[(size_t)k];
        mock::Mat R = mock::Mat::f32(3, 3), t = mock::Mat::f32(3, 1);
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R.at<float>(r, c) = P.R12[3 * r + c]; t.at<float>(r, 0) = P.t12[r]; }
        ORBmatcher matcher(0.75f, true);
        wantFound[(size_t)k] = matcher.SearchBySim3(&P.K1, &P.K2, want[(size_t)k], P.s12, R, t, 7.5f);
        wantS[(size_t)k] = startSim3(P);
        wantIn[(size_t)k] = OptSim3::Run(&P.K1, &P.K2, want[(size_t)k], wantS[(size_t)k], 10.f, k == 1);
        gotS[(size_t)k] = startSim3(P);
    }

    // ---- ONE call
    std::vector<std::vector<MapPoint*> > got = entering;
    std::vector<ComputeSim3::Job> jobs((size_t)NPAIR);
    for (int k = 0; k < NPAIR; k++) {
        cmock::Pair& P = *pairs[(size_t)k];
        ComputeSim3::Job& J = jobs[(size_t)k];
        J.fs = fs; J.slot1 = 2 * k; J.slot2 = 2 * k + 1; J.kf1 = 2 * k; J.kf2 = 2 * k + 1;
        J.pKF1 = &P.K1; J.pKF2 = &P.K2; J.vpMapPointMatches = &got[(size_t)k];
        for (int c = 0; c < 9; c++) J.R12[c] = P.R12[c];
        for (int c = 0; c < 3; c++) J.t12[c] = P.t12[c];
        J.s12 = P.s12;
        J.gScm = &gotS[(size_t)k]; J.bFixScale = k == 1; J.th = 7.5f; J.th2 = 10.f;
    }
    std::vector<ComputeSim3::Result> res;
    try { res = ComputeSim3::RunAll(m, pool, store, jobs, [](MapPoint* p) { return p->id; }); }
    catch (const std::exception& e) { printf("RunAll threw: %s\n", e.what()); return 1; }
    for (int k = 0; k < NPAIR; k++) {
        CHECK(res[(size_t)k].nFound == wantFound[(size_t)k]);
        CHECK(res[(size_t)k].nInliers == wantIn[(size_t)k]);
        CHECK(got[(size_t)k] == want[(size_t)k]);
        double a[8], b[8];
        for (int c = 0; c < 4; c++) { a[c] = gotS[(size_t)k].rotation().coeffs()[c]; b[c] = wantS[(size_t)k].rotation().coeffs()[c]; }
        for (int c = 0; c < 3; c++) { a[4 + c] = gotS[(size_t)k].translation()[c]; b[4 + c] = wantS[(size_t)k].translation()[c]; }
        a[7] = gotS[(size_t)k].scale(); b[7] = wantS[(size_t)k].scale();
        CHECK(memcmp(a, b, sizeof a) == 0);
        CHECK(gotS[(size_t)k].constructed == wantS[(size_t)k].constructed);
        printf("candidate %d: found %d (want %d), inliers %d (want %d), written %d\n", k, res[(size_t)k].nFound, wantFound[(size_t)k], res[(size_t)k].nInliers,
               wantIn[(size_t)k], res[(size_t)k].opt.written);
    }
    CHECK(wantFound[0] >= 50 && wantIn[0] >= 20 && wantFound[1] >= 50 && wantIn[1] >= 20);
    CHECK(wantIn[2] == 0 && res[2].opt.written == 0 && gotS[2].constructed == 0 && res[2].opt.n_corr > 0 && res[2].opt.n_corr < 10);
    CHECK(gotS[1].scale() == (double)pairs[1]->s12);
    // a refusal throws with everything as it came: a keyframe slot the store does not hold
    {
        std::vector<std::vector<MapPoint*> > again = entering;
        std::vector<ComputeSim3::Job> two(jobs.begin(), jobs.begin() + 2);
        std::vector<s3mock::Sim3> S(2);
        for (int k = 0; k < 2; k++) { S[(size_t)k] = startSim3(*pairs[(size_t)k]); two[(size_t)k].gScm = &S[(size_t)k]; two[(size_t)k].vpMapPointMatches = &again[(size_t)k]; }
        two[1].kf2 = 2 * NPAIR;
        bool threw = false;
        try { ComputeSim3::RunAll(m, pool, store, two, [](MapPoint* p) { return p->id; }); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw && again[0] == entering[0] && again[1] == entering[1] && S[0].constructed == 0 && S[1].constructed == 0);
    }
    orbu_store_destroy(store);
    orbw_pool_destroy(pool);
    orbm_frameset_destroy(fs);
    for (void* p : mem) orbx_device_free(ex, p);
    orbx_destroy(ex);
    orbm_destroy(m);
    if (fails) { printf("computesim3 dropin: %d checks FAILED\n", fails); return 1; }
    printf("computesim3 dropin ok\n");
    return 0;
}
