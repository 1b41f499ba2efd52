// fuse_dropin_gpu.cpp -- SearchInNeighborsT (include/LocalMapping_hip.hpp) on mock keyframes and map points
// (tests/cpp/mock_fuse.hpp, whose Replace and ComputeDistinctiveDescriptors are the reference's own) against the reference's
// loop written out over the restatement's serial map model (tools/fuse_ref.hpp), every window search of which is also put to
// the C oracle's window_best: the same observations, keyframe slots, bad flags, replaced pointers and descriptors, and the
// same Replace and AddObservation sequences.  The scene (tests/fuse_cases.py, argv[1]) lists second neighbours repeatedly
// and holds points that survive a Replace and are searched again: the program counts the dirty re-scores and fails without
// one.  Needs a GPU; run by tests/test_gpu_fuse.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "LocalMapping_hip.hpp"
#include "mock_fuse.hpp"
#include "dropin_test.hpp"
#include "../../oracle/orb_oracle.h"
#include "../../tools/fuse_ref.hpp"

typedef iORB_SLAM::SearchInNeighborsT<fmock::KeyFrame, fmock::MapPoint, fmock::Mat> Neighbors;



struct KfData { fuse_ref::Target rec; std::vector<fuse_ref::KeyPt> keys; std::vector<uint8_t> desc; std::vector<int32_t> covis; };

// the C oracle's opinion of every window search the model makes
static std::map<int, std::pair<std::vector<int32_t>, std::vector<int32_t> > > g_grids;
static long g_windowChecks = 0;
static void oracleWindow(const fuse_ref::Model& m, int kf, const fuse_ref::Point& P, const fuse_ref::Result& r)
{
    const fuse_ref::Model::KF& K = m.kfs[kf];
    const fuse_ref::Grid& g = K.rec.grid;
    const OrcGridParams gp = {g.minX, g.minY, g.invW, g.invH, g.cols, g.rows};
    const int n = (int)K.keys.size();
    if (!g_grids.count(kf)) {
        std::pair<std::vector<int32_t>, std::vector<int32_t> >& c = g_grids[kf];
        c.first.assign((size_t)g.cols * g.rows + 1, 0); c.second.assign(n ? n : 1, 0);
        orc_grid_build(&gp, (const OrcKeyPoint*)K.keys.data(), n, c.first.data(), c.second.data());
    }
    const std::pair<std::vector<int32_t>, std::vector<int32_t> >& c = g_grids[kf];
    const float uvr[3] = {r.u, r.v, m.th * m.sf[r.level]};
    const int8_t pred = r.level;
    int32_t bi = -1, bd = 256;
    orc_window_best(uvr, nullptr, &pred, P.desc, nullptr, 1, &gp, (const OrcKeyPoint*)K.keys.data(), c.first.data(), c.second.data(), K.desc.data(),
                    nullptr, n, m.invSigma2.data(), 1, &bi, &bd);
    CHECK(bi == r.bestIdx && bd == r.bestDist);
    g_windowChecks++;
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: fuse_dropin_gpu scene.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t counts[3];
    float sf[8], invSigma2[8], logSf;
    rd(f, counts, 3); rd(f, sf, 8); rd(f, invSigma2, 8); rd(f, &logSf, 1);
    const int nKF = counts[0], nMP = counts[1], nObs = counts[2];
    std::vector<KfData> kd((size_t)nKF);
    for (KfData& k : kd) {
        int32_t n, nc;
        rd(f, &k.rec, 1); rd(f, &n, 1);
        k.keys.resize(n); k.desc.resize((size_t)n * 32);
        rd(f, k.keys.data(), n); rd(f, k.desc.data(), (size_t)n * 32);
        rd(f, &nc, 1);
        k.covis.resize(nc);
        rd(f, k.covis.data(), nc);
    }
    std::vector<fuse_ref::Point> pts((size_t)nMP);
    std::vector<int32_t> obs((size_t)nObs * 3);
    rd(f, pts.data(), nMP); rd(f, obs.data(), obs.size());
    fclose(f);

    // the reference loop on the restatement's model
    fuse_ref::Model model;
    model.th = 3.0f; model.sf.assign(sf, sf + 8); model.invSigma2.assign(invSigma2, invSigma2 + 8); model.logScaleFactor = logSf;
    model.windowCheck = oracleWindow;
    for (const KfData& k : kd) model.kfs[model.addKeyFrame(k.rec, k.keys.data(), k.desc.data(), (int)k.keys.size())].covis.assign(k.covis.begin(), k.covis.end());
    for (const fuse_ref::Point& p : pts) model.addMapPoint(p);
    for (int i = 0; i < nObs; i++) { model.addObservation(obs[3 * i], obs[3 * i + 1], obs[3 * i + 2]); model.kfs[obs[3 * i + 1]].slot[obs[3 * i + 2]] = obs[3 * i]; }
    std::vector<int> wantTargets;
    model.searchInNeighbors(0, wantTargets);

    // the same world as mock objects
    std::vector<std::unique_ptr<fmock::KeyFrame> > kfs;
    std::vector<std::unique_ptr<fmock::MapPoint> > mps;
    std::map<void*, int> idOf;
    for (int k = 0; k < nKF; k++) {
        const KfData& d = kd[k];
        std::unique_ptr<fmock::KeyFrame> kf(new fmock::KeyFrame());
        kf->mnId = k; kf->N = (int)d.keys.size();
        kf->mvKeysUn.resize(kf->N);
        kf->mDescriptors = mock::Mat::u8(kf->N ? kf->N : 1, 32);
        kf->mvpMapPoints.assign(kf->N, nullptr);
        for (int i = 0; i < kf->N; i++) {
            const fuse_ref::KeyPt& p = d.keys[i];
            kf->mvKeysUn[i] = mock::KeyPoint{{p.x, p.y}, p.size, p.angle, p.response, p.octave, p.class_id};
            memcpy(kf->mDescriptors.ptr<uint8_t>(i), &d.desc[(size_t)i * 32], 32);
        }
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) kf->Tcw.at<float>(r, c) = d.rec.Rcw[3 * r + c];
            kf->Tcw.at<float>(r, 3) = d.rec.tcw[r];
            kf->Ow.at<float>(r, 0) = d.rec.Ow[r];
        }
        kf->Tcw.at<float>(3, 3) = 1.f;
        kf->fx = d.rec.K[0]; kf->fy = d.rec.K[1]; kf->cx = d.rec.K[2]; kf->cy = d.rec.K[3];
        kf->mnMinX = (int)d.rec.minX; kf->mnMaxX = (int)d.rec.maxX; kf->mnMinY = (int)d.rec.minY; kf->mnMaxY = (int)d.rec.maxY;
        CHECK((float)kf->mnMinX == d.rec.minX && (float)kf->mnMaxX == d.rec.maxX && (float)kf->mnMinY == d.rec.grid.minY && d.rec.grid.minX == d.rec.minX);
        kf->mnGridCols = d.rec.grid.cols; kf->mnGridRows = d.rec.grid.rows;
        kf->mfGridElementWidthInv = d.rec.grid.invW; kf->mfGridElementHeightInv = d.rec.grid.invH;
        kf->mvScaleFactors.assign(sf, sf + 8); kf->mvInvLevelSigma2.assign(invSigma2, invSigma2 + 8); kf->mfLogScaleFactor = logSf;
        kf->AssignFeaturesToGrid();
        idOf[kf.get()] = k;
        kfs.push_back(std::move(kf));
    }
    for (int k = 0; k < nKF; k++) for (int32_t c : kd[k].covis) kfs[k]->covisible.push_back(kfs[c].get());
    for (int i = 0; i < nMP; i++) {
        std::unique_ptr<fmock::MapPoint> p(new fmock::MapPoint());
        p->mnId = i;
        for (int r = 0; r < 3; r++) { p->mWorldPos.at<float>(r, 0) = pts[i].pos[r]; p->mNormalVector.at<float>(r, 0) = pts[i].normal[r]; }
        p->mfMinDistance = pts[i].minDistance; p->mfMaxDistance = pts[i].maxDistance;
        memcpy(p->mDescriptor.ptr<uint8_t>(0), pts[i].desc, 32);
        idOf[p.get()] = i;
        mps.push_back(std::move(p));
    }
    for (int i = 0; i < nObs; i++) {
        mps[obs[3 * i]]->AddObservation(kfs[obs[3 * i + 1]].get(), obs[3 * i + 2], false);
        kfs[obs[3 * i + 1]]->mvpMapPoints[obs[3 * i + 2]] = mps[obs[3 * i]].get();
    }
    Neighbors::Stats st;
    Neighbors::Run(kfs[0].get(), 0, &st);

    // the target list: repeats included
    CHECK(st.targets == (int)wantTargets.size());
    std::map<int, int> seen;
    int repeats = 0;
    for (int t : wantTargets) repeats += seen[t]++ > 0;
    CHECK(repeats >= 3 && st.distinctTargets == (int)seen.size() && st.distinctTargets < st.targets);
    // the Replace and AddObservation sequences
    CHECK(fmock::g_events.size() == model.events.size());
    int nReplace = 0, nAdd = 0, firstBad = -1;
    for (size_t e = 0; e < fmock::g_events.size() && e < model.events.size(); e++) {
        const fmock::Event& g = fmock::g_events[e];
        const fuse_ref::Event& w = model.events[e];
        const bool same = g.type == w.type && idOf[g.a] == w.a && idOf[g.b] == w.b && (g.type == fuse_ref::EV_REPLACE || g.c == w.c);
        if (!same && firstBad < 0) firstBad = (int)e;
        nReplace += w.type == fuse_ref::EV_REPLACE; nAdd += w.type == fuse_ref::EV_ADD;
    }
    if (firstBad >= 0) printf("the sequences part at event %d of %d\n", firstBad, (int)model.events.size());
    CHECK(firstBad < 0);
    CHECK(nReplace >= 20 && nAdd >= 50 && st.replaced == nReplace && st.added == nAdd);
    // the object graph
    for (int k = 0; k < nKF; k++)
        for (int i = 0; i < kfs[k]->N; i++) {
            fmock::MapPoint* have = kfs[k]->mvpMapPoints[i];
            CHECK((have ? idOf[have] : -1) == model.kfs[k].slot[i]);
        }
    int badPoints = 0, changedDescriptors = 0;
    for (int i = 0; i < nMP; i++) {
        const fuse_ref::Model::MP& w = model.mps[i];
        fmock::MapPoint* p = mps[i].get();
        CHECK(p->mbBad == w.bad && (p->mpReplaced ? idOf[p->mpReplaced] : -1) == w.replaced);
        CHECK(memcmp(p->mDescriptor.ptr<uint8_t>(0), w.rec.desc, 32) == 0);
        CHECK(p->mObservations.size() == w.obs.size() && (w.bad || p->nObs == (int)w.obs.size()));   // (Replace leaves the replaced point's nObs as it was)
        for (size_t o = 0; o < w.obs.size() && o < p->mObservations.size(); o++)
            CHECK(idOf[p->mObservations[o].first] == w.obs[o].first && (int)p->mObservations[o].second == w.obs[o].second);
        badPoints += w.bad;
        changedDescriptors += memcmp(w.rec.desc, pts[i].desc, 32) != 0;
    }
    CHECK(badPoints == nReplace && changedDescriptors >= 5);
    // the update loop ran on the current keyframe's good points, and UpdateConnections once
    CHECK(kfs[0]->nUpdateConnections == 1);
    for (int i = 0; i < kfs[0]->N; i++) if (kfs[0]->mvpMapPoints[i] && !kfs[0]->mvpMapPoints[i]->mbBad) CHECK(kfs[0]->mvpMapPoints[i]->nUpdateNormal == 1);
    // the dirty path was taken, and both phases searched
    CHECK(st.dirtyRescored > 0);
    CHECK(st.pairs1 > 0 && st.pairs2 > 0 && st.fused1 > 0 && st.fused2 > 0 && g_windowChecks > 0);
    printf("targets %d (%d distinct), pairs %d + %d, fused %d + %d, replace %d, add %d, dirty re-scores %d, descriptors changed %d, oracle windows %ld\n",
           st.targets, st.distinctTargets, st.pairs1, st.pairs2, st.fused1, st.fused2, nReplace, nAdd, st.dirtyRescored, changedDescriptors, g_windowChecks);
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("fuse dropin ok\n");
    return 0;
}
