// KeyFrameDatabaseT<KeyFrame, Frame> (include/KeyFrameDatabase_hip.hpp) on mock keyframes that carry the reference's
// member names, against the C++ restatement (tools/kfdb_ref.hpp) on a twin world: two databases over one pool, random
// add / erase / clear / relocalisation / loop queries with repeated ids, covisibility that changes between queries.
// Every candidate list must be equal, in order; ORBVocabulary::score's shim must equal the restatement's double bit for bit.
// Then the reference's threads at once on two databases over a fresh pool: one adds and erases, one adds and runs loop
// queries, one runs relocalisation queries; every candidate must be a keyframe of the world and the sizes must add up.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <thread>
#include <vector>

#include "KeyFrameDatabase_hip.hpp"
#include "dropin_test.hpp"
#include "../../tools/kfdb_ref.hpp"

namespace kfmock {

typedef std::map<unsigned int, double> BowVector;

struct World;
struct KeyFrame {
    typedef kfmock::BowVector BowVector;
    long unsigned int mnId = 0;
    BowVector mBowVec;
    long unsigned int mnLoopQuery = 0; int mnLoopWords = 0; float mLoopScore = 0.f;
    long unsigned int mnRelocQuery = 0; int mnRelocWords = 0; float mRelocScore = 0.f;
    World* w = nullptr;
    int idx = 0;
    std::set<KeyFrame*> GetConnectedKeyFrames();
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N);
};
struct Frame {
    long unsigned int mnId = 0;
    BowVector mBowVec;
};
struct World {
    std::vector<KeyFrame> kfs;
    std::vector<std::vector<int> >* covis = nullptr;
    std::vector<std::vector<int> >* conn = nullptr;
};
std::set<KeyFrame*> KeyFrame::GetConnectedKeyFrames()
{
    std::set<KeyFrame*> s;
    for (size_t i = 0; i < (*w->conn)[idx].size(); i++) s.insert(&w->kfs[(*w->conn)[idx][i]]);
    return s;
}
std::vector<KeyFrame*> KeyFrame::GetBestCovisibilityKeyFrames(const int& N)
{
    std::vector<KeyFrame*> v;
    for (size_t i = 0; i < (*w->covis)[idx].size() && (int)i < N; i++) v.push_back(&w->kfs[(*w->covis)[idx][i]]);
    return v;
}

}  // namespace kfmock

template class orbslamm_hip::KeyFrameDatabaseT<kfmock::KeyFrame, kfmock::Frame>;
template class orbslamm_hip::ORBVocabularyScoreT<kfmock::BowVector>;


static std::vector<int> idx_of(const std::vector<kfmock::KeyFrame*>& v)
{
    std::vector<int> r;
    for (size_t i = 0; i < v.size(); i++) r.push_back(v[i]->idx);
    return r;
}

int main()
{
    const int NW = 600, NKF = 400, PLACES = 40;
    std::mt19937 rng(1234);
    std::vector<int32_t> parent(NW, 0);
    std::vector<uint8_t> leaf(NW, 1), desc((size_t)NW * 32, 0);
    std::vector<double> weight(NW, 1.0);
    orbv_t* voc = nullptr;
    orbslamm_hip::kfdb_check(orbv_create(0, 10, 1, 0, 0, NW, parent.data(), leaf.data(), desc.data(), weight.data(), &voc), "orbv_create");

    // the scene: keyframes of a place share words
    std::vector<std::vector<unsigned> > placeWords(PLACES);
    for (int p = 0; p < PLACES; p++) for (int i = 0; i < 50; i++) placeWords[p].push_back(rng() % NW);
    std::vector<int> place(NKF);
    std::vector<kfmock::BowVector> bows(NKF);
    auto make_bow = [&](int p) {
        kfmock::BowVector b;
        for (int i = 0; i < 24; i++) b[placeWords[p][rng() % 50]] = 0;
        for (int i = 0; i < 6; i++) b[rng() % NW] = 0;
        double s = 0;
        for (auto& e : b) { e.second = 0.05 + (rng() % 1000) / 400.0; s += e.second; }
        for (auto& e : b) e.second /= s;
        return b;
    };
    for (int i = 0; i < NKF; i++) { place[i] = rng() % PLACES; bows[i] = make_bow(place[i]); }
    std::vector<std::vector<int> > covis(NKF), conn(NKF);
    auto reshuffle = [&](int i) {
        covis[i].clear();
        for (int t = 0; t < 12 && (int)covis[i].size() < 10; t++) {
            const int j = rng() % NKF;
            if (j != i && (place[j] == place[i] || rng() % 4 == 0)) covis[i].push_back(j);
        }
        conn[i].assign(covis[i].begin(), covis[i].begin() + std::min<size_t>(4, covis[i].size()));
    };
    for (int i = 0; i < NKF; i++) reshuffle(i);

    kfmock::World dev, ref;
    for (kfmock::World* w : {&dev, &ref}) {
        w->kfs.resize(NKF);
        w->covis = &covis; w->conn = &conn;
        for (int i = 0; i < NKF; i++) { w->kfs[i].w = w; w->kfs[i].idx = i; w->kfs[i].mnId = 1000 + i; w->kfs[i].mBowVec = bows[i]; }
    }

    typedef orbslamm_hip::KeyFrameDatabaseT<kfmock::KeyFrame, kfmock::Frame> DB;
    DB::Pool pool(voc);
    DB db0(&pool), db1(&pool);
    DB* dbs[2] = {&db0, &db1};
    kfdb_ref::Database<kfmock::KeyFrame, kfmock::Frame> r0(NW), r1(NW);
    kfdb_ref::Database<kfmock::KeyFrame, kfmock::Frame>* rdbs[2] = {&r0, &r1};

    int nReloc = 0, nLoop = 0, nCand = 0;
    for (int step = 0; step < 3000; step++) {
        const int d = rng() % 2, k = rng() % NKF, op = rng() % 100;
        if (op < 45) { dbs[d]->add(&dev.kfs[k]); rdbs[d]->add(&ref.kfs[k]); }
        else if (op < 52) { dbs[d]->erase(&dev.kfs[k]); rdbs[d]->erase(&ref.kfs[k]); }
        else if (op < 53) { dbs[d]->clear(); rdbs[d]->clear(); }
        else if (op < 60) reshuffle(k);   // the covisibility graph changes between queries
        else if (op < 80) {
            kfmock::Frame F;
            F.mnId = 1 + rng() % 40;         // few ids: same-id re-queries are common
            F.mBowVec = make_bow(rng() % PLACES);
            const std::vector<int> a = idx_of(dbs[d]->DetectRelocalizationCandidates(&F));
            const std::vector<int> b = idx_of(rdbs[d]->DetectRelocalizationCandidates(&F));
            CHECKF(a == b, "step %d: relocalisation candidates differ (%zu vs %zu)", step, a.size(), b.size());
            nReloc++; nCand += (int)b.size();
        } else {
            const float minScore = (rng() % 100) / 1000.f;
            const long unsigned int id = 1 + rng() % 40;
            dev.kfs[k].mnId = ref.kfs[k].mnId = id;
            const std::vector<int> a = idx_of(dbs[d]->DetectLoopCandidates(&dev.kfs[k], minScore));
            const std::vector<int> b = idx_of(rdbs[d]->DetectLoopCandidates(&ref.kfs[k], minScore));
            CHECKF(a == b, "step %d: loop candidates differ (%zu vs %zu)", step, a.size(), b.size());
            nLoop++; nCand += (int)b.size();
        }
        CHECKF(dbs[d]->size() == rdbs[d]->size() && dbs[d]->empty() == rdbs[d]->empty(), "step %d: size", step);
        if (fails > 10) break;
    }
    orbslamm_hip::ORBVocabularyScoreT<kfmock::BowVector> sc(voc);
    for (int i = 0; i < 200; i++) {
        const kfmock::BowVector& a = bows[rng() % NKF];
        const kfmock::BowVector& b = bows[rng() % NKF];
        const double x = sc.score(a, b), y = kfdb_ref::l1_score(a, b);
        CHECKF(memcmp(&x, &y, 8) == 0, "score %d: %.17g vs %.17g", i, x, y);
    }
    {
        DB::Pool cpool(voc);
        DB c0(&cpool), c1(&cpool);
        std::atomic<int> foreign(0), nConc(0), nConcCand(0);
        auto check = [&](const std::vector<kfmock::KeyFrame*>& v) {
            for (size_t i = 0; i < v.size(); i++) if (v[i] < &dev.kfs[0] || v[i] >= &dev.kfs[0] + NKF) foreign++;
            nConc++;
            nConcCand += (int)v.size();
        };
        std::thread ta([&] {
            for (int i = 0; i < 200; i++) c0.add(&dev.kfs[i]);
            for (int i = 0; i < 200; i += 2) c0.erase(&dev.kfs[i]);
        });
        std::thread tb([&] {
            for (int i = 200; i < 400; i++) {
                c1.add(&dev.kfs[i]);
                if (i % 8 == 0) { dev.kfs[i].mnId = 100000 + i; check(c1.DetectLoopCandidates(&dev.kfs[i], 0.f)); }
            }
        });
        std::thread tc([&] {
            std::mt19937 r(5);
            for (int q = 0; q < 150; q++) {
                kfmock::Frame F;
                F.mnId = 200000 + q;
                F.mBowVec = bows[r() % NKF];
                check((q % 2 ? c0 : c1).DetectRelocalizationCandidates(&F));
            }
        });
        ta.join(); tb.join(); tc.join();
        CHECKF(foreign == 0, "%d candidates outside the world", foreign.load());
        CHECKF(c0.size() == 100 && c1.size() == 200, "concurrent sizes %d %d", c0.size(), c1.size());
        printf("concurrent: %d queries, %d candidates\n", nConc.load(), nConcCand.load());
    }
    orbv_destroy(voc);
    printf("%d relocalisation and %d loop queries, %d candidates\n", nReloc, nLoop, nCand);
    if (fails) { printf("kfdb_dropin_gpu FAILED (%d)\n", fails); return 1; }
    printf("kfdb_dropin_gpu ok\n");
    return 0;
}
