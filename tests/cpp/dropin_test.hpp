// What the drop-in programs (tests/cpp/*_gpu.cpp, built and run by tests/dropin.py) share: the counting checks, the error
// return around a C-ABI call, the scene generators' random stream and rotation, and the smallest mocks of cv::Mat and
// DUtils::Random that the solver templates bind to.  Nothing here computes what the product computes.  Include it after the
// drop-in header under test: OX needs orbx_last_error() declared.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

// CHECK counts a failure and goes on; the first 20 are printed.  A program ends with `return fails ? 1 : 0` and prints its
// marker only when fails == 0.  CHECKF adds a printf-style context to the line.
static int fails __attribute__((unused)) = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) printf("FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); fails++; } } while (0)
#define CHECKF(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAILED %s (%s:%d): ", #c, __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } fails++; } } while (0)
// REQUIRE ends the calling function (which returns int) at the first failure, with the library's last error
#define REQUIRE(c) do { if (!(c)) { printf("FAILED %s (%s:%d): %s\n", #c, __FILE__, __LINE__, orbx_last_error()); return 1; } } while (0)
// a C-ABI call that must succeed, inside a function that returns int
#define OX(call) do { const int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, orbx_last_error()); return 2; } } while (0)

// the scene generators' uniform [0, 1): a 32-bit LCG, its top 24 bits
inline double urand(unsigned& s) { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; }

// n records of a scene file written by a *_cases.py
template <class T> inline void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { printf("short scene file\n"); exit(2); } }

inline int descriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// R = Rz(az) * Ry(ay) * Rx(ax), row-major
inline void eulerR(double ax, double ay, double az, double R[9])
{
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
    const double M[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx};
    for (int k = 0; k < 9; k++) R[k] = M[k];
}
// Tcw of a mock keyframe (a 4x4 whose last row is already 0 0 0 x) from Euler angles and a translation
template <class KeyFrame> inline void setPoseEuler(KeyFrame& kf, double ax, double ay, double az, double tx, double ty, double tz)
{
    double R[9];
    eulerR(ax, ay, az, R);
    const double t[3] = {tx, ty, tz};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) kf.Tcw.template at<float>(r, c) = (float)R[3 * r + c]; kf.Tcw.template at<float>(r, 3) = (float)t[r]; }
    kf.Tcw.template at<float>(3, 3) = 1.f;
}

// the cv::Mat the solver templates need: a dense CV_32F with the (rows, cols, type) constructor
struct Mat32 {
    int rows = 0, cols = 0;
    std::vector<float> d;
    Mat32() {}
    Mat32(int r, int c, int /*type*/) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    bool empty() const { return d.empty(); }
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
};
// Thirdparty/DBoW2/DUtils/Random.cpp's SeedRandOnce / RandomInt over the process's rand()
struct Random {
    static bool& seeded() { static bool s = false; return s; }
    static void SeedRandOnce(int seed) { if (!seeded()) { srand(seed); seeded() = true; } }
    static int RandomInt(int min, int max) { const int d = max - min + 1; return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min; }
};
