// loopfuse_dropin_gpu.cpp -- SearchAndFuseT (include/LoopClosing_hip.hpp) on mock keyframes and map points
// (tests/cpp/mock_loopfuse.hpp over mock_fuse.hpp, whose Replace and ComputeDistinctiveDescriptors are the reference's own)
// against the reference's loop written out over the restatement's serial map model (tools/loopfuse_ref.hpp): the same
// observations, keyframe slots, bad flags, replaced pointers and descriptors, the same Replace and AddObservation sequences
// and the same total of nFused.  The scene (tests/loopfuse_cases.py, argv[1]) gives every corrected keyframe an Scw of scale
// 0.5, 2 or 1 and the records the Python mirror decomposed from it: the drop-in's own decomposition must give the same bits.
// It holds loop points that survive a Replace and are searched again at later targets with another descriptor: the program
// runs the drop-in a second time on a fresh copy of the world with the stale re-score DISABLED and fails unless that run goes
// wrong.  It prints the share of pairs re-scored on the host.  Needs a GPU; run by tests/test_gpu_loopfuse.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "LoopClosing_hip.hpp"
#include "mock_loopfuse.hpp"
#include "dropin_test.hpp"
#include "../../tools/loopfuse_ref.hpp"

typedef iORB_SLAM::SearchAndFuseT<lmock::KeyFrame, lmock::MapPoint, lmock::Mat> LoopFuse;
namespace lr = loopfuse_ref;



struct KfData { lr::Target rec; std::vector<lr::KeyPt> keys; std::vector<uint8_t> desc; };
struct Scene {
    int nKF, nCorrected, nMP, nObs, nLoop;
    float sf[8], logSf, th;
    std::vector<float> scw;
    std::vector<KfData> kd;
    std::vector<lr::Point> pts;
    std::vector<int32_t> obs, loop;
};

// the scene as mock objects
struct World {
    std::vector<std::unique_ptr<lmock::KeyFrame> > kfs;
    std::vector<std::unique_ptr<lmock::MapPoint> > mps;
    std::map<void*, int> idOf;
    std::vector<std::pair<lmock::KeyFrame*, lmock::Mat> > corrected;
    std::vector<lmock::MapPoint*> loop;
    explicit World(const Scene& s)
    {
        for (int k = 0; k < s.nKF; k++) {
            const KfData& d = s.kd[k];
            std::unique_ptr<lmock::KeyFrame> kf(new lmock::KeyFrame());
            kf->mnId = k; kf->N = (int)d.keys.size();
            kf->mvKeysUn.resize(kf->N);
            kf->mDescriptors = mock::Mat::u8(kf->N ? kf->N : 1, 32);
            kf->mvpMapPoints.assign(kf->N, nullptr);
            for (int i = 0; i < kf->N; i++) {
                const lr::KeyPt& p = d.keys[i];
                kf->mvKeysUn[i] = mock::KeyPoint{{p.x, p.y}, p.size, p.angle, p.response, p.octave, p.class_id};
                memcpy(kf->mDescriptors.ptr<uint8_t>(i), &d.desc[(size_t)i * 32], 32);
            }
            // (the keyframe's own pose is NOT the corrected one and is never read by SearchAndFuse: left at zero)
            kf->fx = d.rec.K[0]; kf->fy = d.rec.K[1]; kf->cx = d.rec.K[2]; kf->cy = d.rec.K[3];
            kf->mnMinX = (int)d.rec.minX; kf->mnMaxX = (int)d.rec.maxX; kf->mnMinY = (int)d.rec.minY; kf->mnMaxY = (int)d.rec.maxY;
            CHECK((float)kf->mnMinX == d.rec.minX && (float)kf->mnMaxX == d.rec.maxX && (float)kf->mnMinY == d.rec.grid.minY && d.rec.grid.minX == d.rec.minX);
            kf->mnGridCols = d.rec.grid.cols; kf->mnGridRows = d.rec.grid.rows;
            kf->mfGridElementWidthInv = d.rec.grid.invW; kf->mfGridElementHeightInv = d.rec.grid.invH;
            kf->mvScaleFactors.assign(s.sf, s.sf + 8); kf->mfLogScaleFactor = s.logSf;
            kf->AssignFeaturesToGrid();
            idOf[kf.get()] = k;
            kfs.push_back(std::move(kf));
        }
        for (int i = 0; i < s.nMP; i++) {
            std::unique_ptr<lmock::MapPoint> p(new lmock::MapPoint());
            p->mnId = i;
            for (int r = 0; r < 3; r++) { p->mWorldPos.at<float>(r, 0) = s.pts[i].pos[r]; p->mNormalVector.at<float>(r, 0) = s.pts[i].normal[r]; }
            p->mfMinDistance = s.pts[i].minDistance; p->mfMaxDistance = s.pts[i].maxDistance;
            memcpy(p->mDescriptor.ptr<uint8_t>(0), s.pts[i].desc, 32);
            idOf[p.get()] = i;
            mps.push_back(std::move(p));
        }
        for (int i = 0; i < s.nObs; i++) {
            mps[s.obs[3 * i]]->AddObservation(kfs[s.obs[3 * i + 1]].get(), s.obs[3 * i + 2], false);
            kfs[s.obs[3 * i + 1]]->mvpMapPoints[s.obs[3 * i + 2]] = mps[s.obs[3 * i]].get();
        }
        for (int t = 0; t < s.nCorrected; t++) {
            lmock::Mat S = lmock::Mat::f32(4, 4);
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) S.at<float>(r, c) = s.scw[(size_t)t * 16 + 4 * r + c];
            corrected.push_back(std::make_pair(kfs[t].get(), S));
        }
        for (int i = 0; i < s.nLoop; i++) loop.push_back(mps[s.loop[i]].get());
    }
};

// the mock world against the model: the differences (0: the same map)
static int differences(const Scene& s, World& w, const lr::Model& model, const std::vector<fmock::Event>& got)
{
    int diff = got.size() != model.events.size();
    for (size_t e = 0; e < got.size() && e < model.events.size(); e++) {
        const fmock::Event& g = got[e];
        const lr::Event& m = model.events[e];
        diff += !(g.type == m.type && w.idOf[g.a] == m.a && w.idOf[g.b] == m.b && (g.type == lr::EV_REPLACE || g.c == m.c));
    }
    for (int k = 0; k < s.nKF; k++)
        for (int i = 0; i < w.kfs[k]->N; i++) {
            fmock::MapPoint* have = w.kfs[k]->mvpMapPoints[i];
            diff += (have ? w.idOf[have] : -1) != model.kfs[k].slot[i];
        }
    for (int i = 0; i < s.nMP; i++) {
        const lr::Model::MP& m = model.mps[i];
        fmock::MapPoint* p = w.mps[i].get();
        diff += !(p->mbBad == m.bad && (p->mpReplaced ? w.idOf[p->mpReplaced] : -1) == m.replaced);
        diff += memcmp(p->mDescriptor.ptr<uint8_t>(0), m.rec.desc, 32) != 0;
        diff += p->mObservations.size() != m.obs.size();
        for (size_t o = 0; o < m.obs.size() && o < p->mObservations.size(); o++)
            diff += !(w.idOf[p->mObservations[o].first] == m.obs[o].first && (int)p->mObservations[o].second == m.obs[o].second);
    }
    return diff;
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: loopfuse_dropin_gpu scene.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Scene s;
    int32_t counts[5];
    float tail[2];
    rd(f, counts, 5); rd(f, s.sf, 8); rd(f, tail, 2);
    s.nKF = counts[0]; s.nCorrected = counts[1]; s.nMP = counts[2]; s.nObs = counts[3]; s.nLoop = counts[4];
    s.logSf = tail[0]; s.th = tail[1];
    s.scw.resize((size_t)s.nCorrected * 16);
    rd(f, s.scw.data(), s.scw.size());
    s.kd.resize((size_t)s.nKF);
    for (KfData& k : s.kd) {
        int32_t n;
        rd(f, &k.rec, 1); rd(f, &n, 1);
        k.keys.resize(n); k.desc.resize((size_t)n * 32);
        rd(f, k.keys.data(), n); rd(f, k.desc.data(), (size_t)n * 32);
    }
    s.pts.resize((size_t)s.nMP); s.obs.resize((size_t)s.nObs * 3); s.loop.resize((size_t)s.nLoop);
    rd(f, s.pts.data(), s.nMP); rd(f, s.obs.data(), s.obs.size()); rd(f, s.loop.data(), s.nLoop);
    fclose(f);

    // the reference loop on the restatement's model, under the records the scene file carries
    lr::Model model;
    model.sf.assign(s.sf, s.sf + 8); model.logScaleFactor = s.logSf;
    for (const KfData& k : s.kd) model.addKeyFrame(k.rec.grid, k.keys.data(), k.desc.data(), (int)k.keys.size());
    for (const lr::Point& p : s.pts) model.addMapPoint(p);
    for (int i = 0; i < s.nObs; i++) { model.addObservation(s.obs[3 * i], s.obs[3 * i + 1], s.obs[3 * i + 2]); model.kfs[s.obs[3 * i + 1]].slot[s.obs[3 * i + 2]] = s.obs[3 * i]; }
    std::vector<lr::Model::Corrected> corrected((size_t)s.nCorrected);
    for (int t = 0; t < s.nCorrected; t++) { corrected[t].kf = t; corrected[t].rec = s.kd[t].rec; }
    const std::vector<int> loop(s.loop.begin(), s.loop.end());
    const int wantFused = model.searchAndFuse(corrected, loop, s.th);

    // the drop-in's decomposition of every Scw gives the record's bits
    {
        World w(s);
        for (int t = 0; t < s.nCorrected; t++) {
            iORB_SLAM::cvsem::Mat33 R; iORB_SLAM::cvsem::Vec3 tc, O;
            iORB_SLAM::cvsem::decomposeSim3(w.corrected[t].second, R, tc, O);
            CHECK(memcmp(R.m, s.kd[t].rec.Rcw, 36) == 0 && memcmp(tc.v, s.kd[t].rec.tcw, 12) == 0 && memcmp(O.v, s.kd[t].rec.Ow, 12) == 0);
        }
    }

    // the drop-in
    World w(s);
    fmock::g_events.clear();
    LoopFuse::Stats st;
    int locks = 0;
    const int gotFused = LoopFuse::Run(w.corrected, w.loop, s.th, [&locks] { return ++locks; }, &st);
    const std::vector<fmock::Event> events = fmock::g_events;
    CHECK(gotFused == wantFused && st.fused == wantFused);
    CHECK(locks == s.nCorrected);
    const int diff = differences(s, w, model, events);
    if (diff) printf("%d differences between the drop-in's map and the serial loop's\n", diff);
    CHECK(diff == 0);
    int nReplace = 0, nAdd = 0, badPoints = 0, changedDescriptors = 0;
    for (const lr::Event& e : model.events) { nReplace += e.type == lr::EV_REPLACE; nAdd += e.type == lr::EV_ADD; }
    for (int i = 0; i < s.nMP; i++) { badPoints += model.mps[i].bad; changedDescriptors += memcmp(model.mps[i].rec.desc, s.pts[i].desc, 32) != 0; }
    CHECK(nReplace >= 20 && nAdd >= 50 && st.replaced == nReplace && st.added == nAdd && badPoints > 0 && changedDescriptors >= 5);
    CHECK(st.targets == s.nCorrected && st.distinctTargets == s.nCorrected && st.points == s.nLoop && st.pairs == (long)s.nCorrected * s.nLoop);
    CHECK(st.hits > 0 && st.rescored > 0);

    // the same with the stale re-score disabled: it must go wrong on this scene
    World w2(s);
    fmock::g_events.clear();
    LoopFuse::Options off;
    off.rescoreStale = false;
    LoopFuse::Stats st2;
    (void)LoopFuse::Run(w2.corrected, w2.loop, s.th, &st2, off);
    const int diffOff = differences(s, w2, model, fmock::g_events);
    CHECK(diffOff > 0 && st2.rescored == 0);

    printf("targets %d, loop points %d, pairs %ld, device hits %d, fused %d, replace %d, add %d, descriptors changed %d\n", st.targets, st.points, st.pairs,
           st.hits, gotFused, nReplace, nAdd, changedDescriptors);
    printf("pairs re-scored on the host: %ld of %ld, share %.4f; without the re-score %d differences\n", st.rescored, st.pairs,
           (double)st.rescored / (double)st.pairs, diffOff);
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("loopfuse dropin ok\n");
    return 0;
}
