// init_dropin_gpu.cpp -- InitializerT (include/Initializer_hip.hpp) on mock frames against the restatement
// (tools/init_ref.hpp): both scenarios, a general and a planar scene; results equal as bits, and the process's rand()
// stream after Initialize equals its state after the restatement's draws.  Needs a GPU; run by tests/test_gpu_init.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Initializer_hip.hpp"
#include "dropin_test.hpp"
#include "../../tools/init_ref.hpp"

namespace imock {
struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
struct Point3f { float x, y, z; Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
struct Frame { std::vector<KeyPoint> mvKeysUn; Mat32 mK; };
}  // namespace imock

static const float K4[4] = {517.3f, 516.5f, 318.6f, 255.3f};

// n1 / n2 keys, nm matched (30 % of them outliers), general or planar scene seen from two poses
static void scene(unsigned seed, bool planar, int n1, int n2, int nm, imock::Frame& f1, imock::Frame& f2, std::vector<int>& m12)
{
    unsigned s = seed;
    const double R[9] = {0.99675, -0.01160, -0.07969, 0.00997, 0.99973, -0.02080, 0.07991, 0.01993, 0.99660};
    const double t[3] = {0.6, 0.05, 0.1};
    f1.mvKeysUn.clear(); f2.mvKeysUn.clear();
    m12.assign((size_t)n1, -1);
    f1.mK = Mat32(3, 3, 5);
    f1.mK.at<float>(0, 0) = K4[0]; f1.mK.at<float>(1, 1) = K4[1]; f1.mK.at<float>(0, 2) = K4[2]; f1.mK.at<float>(1, 2) = K4[3]; f1.mK.at<float>(2, 2) = 1.f;
    f2.mK = f1.mK;
    auto key = [&](double x, double y) { imock::KeyPoint k = {(float)x, (float)y, 31.f, (float)(360 * urand(s)), 1.f, 0, -1}; return k; };
    while ((int)f1.mvKeysUn.size() < nm) {
        const double u = 20 + 600 * urand(s), v = 20 + 440 * urand(s);
        const double z = planar ? 4.0 + 0.3 * (u - K4[2]) / K4[0] + 0.2 * (v - K4[3]) / K4[1] : 3.0 + 6.0 * urand(s);
        const double X[3] = {(u - K4[2]) / K4[0] * z, (v - K4[3]) / K4[1] * z, z};
        double Y[3];
        for (int r = 0; r < 3; r++) Y[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
        const double u2 = K4[0] * Y[0] / Y[2] + K4[2] + (urand(s) - 0.5), v2 = K4[1] * Y[1] / Y[2] + K4[3] + (urand(s) - 0.5);
        if (u2 < 5 || u2 >= 635 || v2 < 5 || v2 >= 475) continue;
        m12[f1.mvKeysUn.size()] = urand(s) < 0.3 ? (int)(urand(s) * n2) % n2 : (int)f2.mvKeysUn.size();
        f1.mvKeysUn.push_back(key(u, v));
        f2.mvKeysUn.push_back(key(u2, v2));
    }
    while ((int)f1.mvKeysUn.size() < n1) f1.mvKeysUn.push_back(key(640 * urand(s), 480 * urand(s)));
    while ((int)f2.mvKeysUn.size() < n2) f2.mvKeysUn.push_back(key(640 * urand(s), 480 * urand(s)));
}

template <bool kHF>
static int run_case(unsigned seed, bool planar)
{
    imock::Frame f1, f2;
    std::vector<int> m12;
    scene(seed, planar, 900, 850, 400, f1, f2, m12);
    // the drop-in: its draws move the process's rand() stream
    srand(12345 + seed);
    Random::seeded() = false;                       // (a fresh process: SeedRandOnce(0) seeds)
    iORB_SLAM::InitializerT<imock::Frame, Mat32, imock::Point3f, Random, kHF> ini(f1, 1.0, 200);
    Mat32 R21, t21;
    std::vector<imock::Point3f> P;
    std::vector<bool> tri;
    const bool ok = ini.Initialize(f2, m12, R21, t21, P, tri);
    const int nextAfterDropin = rand();
    // the restatement, with its own DUtils over the same stream
    srand(12345 + seed);
    init_ref::alreadySeeded() = false;
    int N = 0;
    for (int m : m12) N += m >= 0;
    const std::vector<int32_t> sets = init_ref::drawSets(N, 200);
    const int nextAfterRef = rand();
    std::vector<init_ref::KeyPt> k1(f1.mvKeysUn.size()), k2(f2.mvKeysUn.size());
    std::memcpy(k1.data(), f1.mvKeysUn.data(), k1.size() * sizeof(init_ref::KeyPt));
    std::memcpy(k2.data(), f2.mvKeysUn.data(), k2.size() * sizeof(init_ref::KeyPt));
    init_ref::Initializer ref(k1, K4, 1.0f, 200, kHF);
    init_ref::Result res;
    std::vector<float> rP;
    std::vector<uint8_t> rT;
    const bool rok = ref.Initialize(k2, m12, sets, res, rP, rT);
    const int before = fails;
#define EXPECT(c) CHECKF(c, "seed %u planar %d hf %d", seed, (int)planar, (int)kHF)
    EXPECT(nextAfterDropin == nextAfterRef);
    EXPECT(ok == rok);
    EXPECT(std::memcmp(&ini.lastResult(), &res, sizeof res) == 0);
    if (rok) {
        EXPECT(R21.rows == 3 && t21.rows == 3);
        EXPECT(std::memcmp(R21.d.data(), res.R21, 36) == 0 && std::memcmp(t21.d.data(), res.t21, 12) == 0);
        EXPECT(P.size() == f1.mvKeysUn.size() && tri.size() == f1.mvKeysUn.size());
        for (size_t i = 0; i < P.size() && fails == before; i++) {
            EXPECT(std::memcmp(&P[i].x, &rP[3 * i], 4) == 0 && std::memcmp(&P[i].y, &rP[3 * i + 1], 4) == 0 && std::memcmp(&P[i].z, &rP[3 * i + 2], 4) == 0);
            EXPECT(tri[i] == (rT[i] != 0));
        }
    } else if (res.rtState == 1)
        EXPECT(R21.rows == 0 && t21.rows == 0);
    printf("seed %u planar %d hf %d: ok %d reconH %d nGood best %d\n", seed, (int)planar, (int)kHF, (int)ok, res.reconH, res.best >= 0 ? res.nGood[res.best] : -1);
    return fails - before;
#undef EXPECT
}

int main()
{
    static_assert(sizeof(init_ref::Result) == sizeof(OrbiResult), "OrbiResult layout");
    int bad = 0;
    for (unsigned seed = 1; seed <= 3; seed++) {
        bad += run_case<true>(seed, false);
        bad += run_case<true>(seed, true);
        bad += run_case<false>(seed, false);
    }
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("init dropin ok\n");
    return 0;
}
