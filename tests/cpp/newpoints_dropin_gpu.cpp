// newpoints_dropin_gpu.cpp -- CreateNewMapPointsT (include/LocalMapping_hip.hpp) on mock keyframes and map points
// (tests/cpp/mock_localmap.hpp) against the reference's loop written out here over the C oracle's SearchForTriangulation and
// the restatement (tools/newpoints_ref.hpp), neighbour after neighbour: the same mvpMapPoints, observations and positions,
// the same order in the map and in the recent-points list; and with the CheckNewKeyFrames predicate firing at neighbour 3,
// exactly what neighbours 0..2 leave.  The scene comes from tests/newpoints_cases.py as a file (argv[1]).  Needs a GPU; run
// by tests/test_gpu_newpoints.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "LocalMapping_hip.hpp"
#include "mock_localmap.hpp"
#include "dropin_test.hpp"
#include "../../oracle/orb_oracle.h"
#include "../../tools/newpoints_ref.hpp"

typedef iORB_SLAM::CreateNewMapPointsT<lmock::KeyFrame, lmock::MapPoint, lmock::Map, lmock::Mat> NewPoints;


struct SideData {
    int n = 0;
    std::vector<newpoints_ref::KeyPt> keys;
    std::vector<uint8_t> desc, skip;
    std::vector<uint32_t> node;
    std::vector<int32_t> start, idx;
    newpoints_ref::KeyFrame kf;
};


static void readSide(FILE* f, SideData& s)
{
    int32_t n, nn;
    rd(f, &n, 1);
    s.n = n;
    s.keys.resize(n); s.desc.resize((size_t)n * 32); s.skip.resize(n);
    rd(f, s.keys.data(), n); rd(f, s.desc.data(), (size_t)n * 32); rd(f, s.skip.data(), n);
    rd(f, &nn, 1);
    s.node.resize(nn); s.start.resize(nn + 1);
    rd(f, s.node.data(), nn); rd(f, s.start.data(), nn + 1);
    s.idx.resize(s.start[nn]);
    rd(f, s.idx.data(), s.idx.size());
    rd(f, &s.kf, 1);
}

// a world of mock objects from the scene; a feature with a skip flag holds an old map point
struct World {
    std::vector<std::unique_ptr<lmock::KeyFrame> > kfs;      // [0] the current keyframe
    std::vector<std::unique_ptr<lmock::MapPoint> > old;
    lmock::Map map;
    std::list<lmock::MapPoint*> recent;
    ~World() { for (lmock::MapPoint* p : map.points) delete p; }
};

static void build(const std::vector<SideData>& sides, const float* sf, const float* sigma2, World& w)
{
    for (size_t s = 0; s < sides.size(); s++) {
        const SideData& d = sides[s];
        std::unique_ptr<lmock::KeyFrame> kf(new lmock::KeyFrame());
        kf->id = (int)s; kf->N = d.n;
        kf->mvKeysUn.resize(d.n);
        kf->mDescriptors = mock::Mat::u8(d.n, 32);
        kf->mvpMapPoints.assign(d.n, nullptr);
        for (int i = 0; i < d.n; i++) {
            const newpoints_ref::KeyPt& k = d.keys[i];
            kf->mvKeysUn[i] = mock::KeyPoint{{k.x, k.y}, k.size, k.angle, k.response, k.octave, k.class_id};
            memcpy(kf->mDescriptors.ptr<uint8_t>(i), &d.desc[(size_t)i * 32], 32);
            if (d.skip[i]) { w.old.emplace_back(new lmock::MapPoint(lmock::Mat(3, 1, 5), kf.get(), &w.map)); kf->mvpMapPoints[i] = w.old.back().get(); }
        }
        for (size_t a = 0; a < d.node.size(); a++)
            for (int j = d.start[a]; j < d.start[a + 1]; j++) kf->mFeatVec[d.node[a]].push_back((unsigned)d.idx[j]);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) kf->Tcw.at<float>(r, c) = d.kf.Rcw[3 * r + c];
            kf->Tcw.at<float>(r, 3) = d.kf.tcw[r];
            kf->Ow.at<float>(r, 0) = d.kf.Ow[r];
        }
        kf->Tcw.at<float>(3, 3) = 1.f;
        kf->fx = d.kf.K[0]; kf->fy = d.kf.K[1]; kf->cx = d.kf.K[2]; kf->cy = d.kf.K[3];
        kf->mvScaleFactors.assign(sf, sf + 8); kf->mvLevelSigma2.assign(sigma2, sigma2 + 8);
        kf->medianDepth = d.kf.medianDepth;
        w.kfs.push_back(std::move(kf));
    }
    for (size_t s = 1; s < w.kfs.size(); s++) w.kfs[0]->covisible.push_back(w.kfs[s].get());
}

// CreateNewMapPoints as the reference runs it, on the flattened scene: what each accepted pair leaves, neighbour by neighbour
static std::vector<newpoints_ref::NewPoint> referenceLoop(const std::vector<SideData>& sides, const float* sf, const float* sigma2, int stopAt)
{
    const SideData& A = sides[0];
    std::vector<uint8_t> skip1 = A.skip;
    std::vector<newpoints_ref::NewPoint> all;
    const OrcFeatVec fv1 = {(int)A.node.size(), A.node.data(), A.start.data(), A.idx.data()};
    for (size_t k = 0; k + 1 < sides.size(); k++) {
        if ((int)k == stopAt) break;      // `if(i>0 && CheckNewKeyFrames()) return;`
        const SideData& B = sides[k + 1];
        std::vector<int32_t> m12(A.n, -1);
        const bool gated = newpoints_ref::baselineTooShort(A.kf, B.kf);
        if (!gated && A.n && B.n) {
            float F[9], e[2];
            newpoints_ref::computeF12(A.kf, B.kf, F, e);
            const OrcFeatVec fv2 = {(int)B.node.size(), B.node.data(), B.start.data(), B.idx.data()};
            orc_search_for_triangulation((const OrcKeyPoint*)A.keys.data(), A.desc.data(), skip1.data(), nullptr, A.n, &fv1,
                                         (const OrcKeyPoint*)B.keys.data(), B.desc.data(), B.skip.data(), nullptr, B.n, &fv2, F, e[0], e[1], sf, sigma2,
                                         0, 0, m12.data());
        }
        std::vector<newpoints_ref::NewPoint> out(A.n ? A.n : 1);
        std::vector<uint8_t> st(A.n ? A.n : 1);
        const int n = newpoints_ref::neighbour((int)k, A.kf, B.kf, A.keys.data(), A.n, B.keys.data(), gated ? nullptr : m12.data(), skip1.data(), sf, sigma2,
                                               8, 1.2f, out.data(), st.data());
        all.insert(all.end(), out.begin(), out.begin() + n);
    }
    return all;
}

static void compare(World& w, const std::vector<SideData>& sides, const std::vector<newpoints_ref::NewPoint>& want, int nnew)
{
    CHECK(nnew == (int)want.size());
    CHECK(w.map.points.size() == want.size() && w.recent.size() == want.size());
    // the expected object graph: old points where the scene had them, then every record in order (a later record of a
    // neighbour may overwrite its idx2, as pKF2->AddMapPoint does)
    std::vector<std::vector<int> > expect(sides.size());
    for (size_t s = 0; s < sides.size(); s++) { expect[s].assign(sides[s].n, -1); for (int i = 0; i < sides[s].n; i++) if (sides[s].skip[i]) expect[s][i] = -2; }
    for (size_t r = 0; r < want.size(); r++) { expect[0][want[r].idx1] = (int)r; expect[(size_t)want[r].neighbour + 1][want[r].idx2] = (int)r; }
    std::list<lmock::MapPoint*>::iterator it = w.recent.begin();
    for (size_t r = 0; r < want.size() && r < w.map.points.size(); r++, ++it) {
        lmock::MapPoint* p = w.map.points[r];
        CHECK(*it == p);
        CHECK(memcmp(&p->mWorldPos.at<float>(0, 0), want[r].pos, 12) == 0);
        CHECK(p->mpRefKF == w.kfs[0].get() && p->mpMap == &w.map);
        CHECK(p->mObservations.size() == 2);
        CHECK(p->mObservations.count(w.kfs[0].get()) && (int)p->mObservations[w.kfs[0].get()] == want[r].idx1);
        lmock::KeyFrame* k2 = w.kfs[(size_t)want[r].neighbour + 1].get();
        CHECK(p->mObservations.count(k2) && (int)p->mObservations[k2] == want[r].idx2);
        CHECK(p->nDistinctive == 1 && p->nUpdateNormal == 1 && p->observationsAtDistinctive == 2);
    }
    for (size_t s = 0; s < sides.size(); s++)
        for (int i = 0; i < sides[s].n; i++) {
            mock::MapPoint* have = w.kfs[s]->mvpMapPoints[i];
            const int e = expect[s][i];
            if (e == -1) CHECK(have == nullptr);
            else if (e == -2) CHECK(have != nullptr && have->mObservations.empty());
            else CHECK(e < (int)w.map.points.size() && have == w.map.points[e]);
        }
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: newpoints_dropin_gpu scene.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t K;
    float sf[8], sigma2[8];
    rd(f, &K, 1); rd(f, sf, 8); rd(f, sigma2, 8);
    std::vector<SideData> sides((size_t)K + 1);
    for (SideData& s : sides) readSide(f, s);
    fclose(f);
    CHECK(K >= 5);

    // the whole loop
    {
        World w;
        build(sides, sf, sigma2, w);
        std::vector<uint8_t> status;
        int polls = 0;
        const int nnew = NewPoints::Run(w.kfs[0].get(), &w.map, w.recent, [&] { polls++; return false; }, 0, &status);
        const std::vector<newpoints_ref::NewPoint> want = referenceLoop(sides, sf, sigma2, -1);
        compare(w, sides, want, nnew);
        CHECK(polls == K - 1);
        CHECK(want.size() >= 100);
        int neighboursWithPoints = 0;
        for (int k = 0; k < K; k++) { bool any = false; for (const newpoints_ref::NewPoint& p : want) any |= p.neighbour == k; neighboursWithPoints += any; }
        CHECK(neighboursWithPoints >= 4);
        size_t accepted = 0;
        for (uint8_t s : status) accepted += s == ORBL_ST_ACCEPTED;
        CHECK(status.size() == (size_t)K * sides[0].n && accepted == want.size());
        printf("full loop: %d new points over %d neighbours\n", nnew, K);
    }
    // CheckNewKeyFrames fires at neighbour 3: exactly neighbours 0..2
    {
        World w;
        build(sides, sf, sigma2, w);
        int polls = 0;
        const int nnew = NewPoints::Run(w.kfs[0].get(), &w.map, w.recent, [&] { polls++; return polls >= 3; });
        const std::vector<newpoints_ref::NewPoint> want = referenceLoop(sides, sf, sigma2, 3);
        compare(w, sides, want, nnew);
        CHECK(polls == 3);
        for (const newpoints_ref::NewPoint& p : want) CHECK(p.neighbour <= 2);
        const std::vector<newpoints_ref::NewPoint> all = referenceLoop(sides, sf, sigma2, -1);
        CHECK(want.size() < all.size() && !want.empty());
        printf("early return: %d of %d new points\n", nnew, (int)all.size());
    }
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("newpoints dropin ok\n");
    return 0;
}
