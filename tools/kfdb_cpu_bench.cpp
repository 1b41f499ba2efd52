// kfdb_cpu_bench.cpp -- the CPU side of tools/kfdb_bench.py: the same scene and the same query sequence on the C++
// restatement (tools/kfdb_ref.hpp), one host core.  Reads the scene file the script wrote, writes one line per query:
// "<kind> <microseconds> <candidate slots...>".
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "kfdb_ref.hpp"

struct KF;
static std::vector<KF>* g_kfs;
static std::vector<std::vector<int32_t> > g_covis, g_conn;
struct KF {
    typedef std::map<unsigned int, double> BowVector;
    long unsigned int mnId = 0;
    BowVector mBowVec;
    long unsigned int mnLoopQuery = 0; int mnLoopWords = 0; float mLoopScore = 0.f;
    long unsigned int mnRelocQuery = 0; int mnRelocWords = 0; float mRelocScore = 0.f;
    int idx = 0;
    std::set<KF*> GetConnectedKeyFrames()
    {
        std::set<KF*> s;
        for (int32_t j : g_conn[idx]) s.insert(&(*g_kfs)[j]);
        return s;
    }
    std::vector<KF*> GetBestCovisibilityKeyFrames(const int& N)
    {
        std::vector<KF*> v;
        for (size_t i = 0; i < g_covis[idx].size() && (int)i < N; i++) v.push_back(&(*g_kfs)[g_covis[idx][i]]);
        return v;
    }
};
struct Frame {
    long unsigned int mnId = 0;
    KF::BowVector mBowVec;
};

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }
static KF::BowVector read_bow(FILE* f)
{
    int32_t n = 0;
    rd(f, &n, 4);
    std::vector<uint32_t> ids(n);
    std::vector<double> v(n);
    if (n) { rd(f, ids.data(), 4 * (size_t)n); rd(f, v.data(), 8 * (size_t)n); }
    KF::BowVector b;
    for (int i = 0; i < n; i++) b[ids[i]] = v[i];
    return b;
}
static std::vector<int32_t> read_list(FILE* f)
{
    int32_t n = 0;
    rd(f, &n, 4);
    std::vector<int32_t> v(n);
    if (n) rd(f, v.data(), 4 * (size_t)n);
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: kfdb_cpu_bench scene.bin out.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];   // keyframes, words, database members (slots [0, members))
    rd(f, hdr, 12);
    std::vector<KF> kfs((size_t)hdr[0]);
    g_kfs = &kfs;
    g_covis.resize(kfs.size()); g_conn.resize(kfs.size());
    for (size_t i = 0; i < kfs.size(); i++) { kfs[i].idx = (int)i; kfs[i].mnId = 1u << 30; kfs[i].mBowVec = read_bow(f); }
    for (size_t i = 0; i < kfs.size(); i++) g_covis[i] = read_list(f);
    kfdb_ref::Database<KF, Frame> db((size_t)hdr[1]);
    for (int i = 0; i < hdr[2]; i++) db.add(&kfs[(size_t)i]);
    FILE* o = fopen(argv[2], "w");
    int32_t kind = 0;
    while (rd(f, &kind, 4)) {
        uint64_t id = 0;
        rd(f, &id, 8);
        std::vector<KF*> c;
        double us = 0;
        if (kind == 0) {   // relocalisation: a frame's BowVector
            Frame F;
            F.mnId = id;
            F.mBowVec = read_bow(f);
            const auto t0 = std::chrono::steady_clock::now();
            c = db.DetectRelocalizationCandidates(&F);
            us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        } else {           // loop: slot, minScore, connected
            int32_t s = 0;
            float ms = 0;
            rd(f, &s, 4); rd(f, &ms, 4);
            g_conn[(size_t)s] = read_list(f);
            kfs[(size_t)s].mnId = id;
            const auto t0 = std::chrono::steady_clock::now();
            c = db.DetectLoopCandidates(&kfs[(size_t)s], ms);
            us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        }
        fprintf(o, "%d %.3f", kind, us);
        for (KF* k : c) fprintf(o, " %d", k->idx);
        fprintf(o, "\n");
    }
    fclose(o);
    fclose(f);
    return 0;
}
