// g2o_core_check.hip -- the host instantiations of orbg_kernels.hip (and the two oplus functions, which stay with their kernels)
// against the restatements' Defined functions, as bits, on seeded inputs; no device, no HIP runtime call.  Prints a count per
// class, stops at the first mismatch (exit status 1) and asserts that no class is empty: several of the LDLT's paths (the cutoff
// break, a finite matrix that is not positive) are reached by no scene family of the optimizers' tests, so this is their check.
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -o g2o_core_check tests/cpp/g2o_core_check.hip && ./g2o_core_check
// A NaN equals a NaN here whatever its sign and payload: which operand's NaN an operation hands on is the compiler's choice of
// operand order, and the kernels canonicalise theirs on the way out.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/orbslamm_hip.h"
#include "../../orbslamm_amd/csrc/orbx_cvmath.hpp"
#include "../../orbslamm_amd/csrc/orbm_kernels.hip"   // orbm::KeyDev, which orbo's frame record points to
#include "../../orbslamm_amd/csrc/orbg_kernels.hip"
#include "../../orbslamm_amd/csrc/orbo_kernels.hip"
#include "../../orbslamm_amd/csrc/orbz_kernels.hip"
#include "../../tools/poseopt_ref.hpp"
#include "../../tools/sim3opt_ref.hpp"

namespace pr = poseopt_ref;
namespace sr = sim3opt_ref;

static uint64_t g_state;
static uint64_t next_u64()   // splitmix64
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
static double sym() { return 2.0 * uni() - 1.0; }                                          // [-1, 1)
static double log_uniform(double lo, double hi) { return std::exp(std::log(lo) + uni() * (std::log(hi) - std::log(lo))); }
static double signed_of(double v) { return (next_u64() & 1) ? -v : v; }

static bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, 8) == 0; }
static bool same_n(const double* a, const double* b, int n)
{
    for (int i = 0; i < n; i++) if (!same(a[i], b[i])) return false;
    return true;
}
static void fail(const char* what, long i)
{
    std::printf("MISMATCH %s at input %ld\n", what, i);
    std::exit(1);
}
static void need(bool ok, const char* what)
{
    if (!ok) { std::printf("EMPTY OR UNEXPECTED: %s\n", what); std::exit(1); }
}

// ------------------------------------------------------------------ the LDLT
template <int N> static bool ref_solve(double* M, const double* b, double* x);
template <> bool ref_solve<6>(double* M, const double* b, double* x) { return pr::ldltSolve6(M, b, x); }
template <> bool ref_solve<7>(double* M, const double* b, double* x) { return sr::ldltSolveN<7>(M, b, x); }

template <int N> struct Ldlt {
    long solvedCount = 0, refusedCount = 0;

    // returns what both returned; a mismatch ends the program
    bool one(const double* M, const char* what, long i)
    {
        double Ma[N * N], Mb[N * N], b[N], xa[N], xb[N], keep[N], tmp[N];
        int tr[N];
        for (int k = 0; k < N * N; k++) { Ma[k] = M[k]; Mb[k] = M[k]; }
        for (int k = 0; k < N; k++) { b[k] = sym() * 10.0; keep[k] = sym(); xa[k] = keep[k]; xb[k] = keep[k]; }
        const bool ra = ref_solve<N>(Ma, b, xa);
        const bool rb = orbg::ldlt_solve<N>(Mb, b, xb, tr, tmp);
        if (ra != rb || !same_n(xa, xb, N) || !same_n(Ma, Mb, N * N)) fail(what, i);
        if (!rb && std::memcmp(xb, keep, sizeof keep) != 0) fail("x survives a refused solve", i);   // x keeps its contents
        (rb ? solvedCount : refusedCount)++;
        return rb;
    }

    // J^T J + lambda I, J of N + 3 seeded rows with its columns scaled by colScale
    static void normal_matrix(double* M, const double* colScale)
    {
        double J[(N + 3) * N];
        for (int r = 0; r < N + 3; r++) for (int c = 0; c < N; c++) J[r * N + c] = sym() * colScale[c];
        double dmax = 0.0;
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) {
                double s = 0.0;
                for (int r = 0; r < N + 3; r++) s += J[r * N + i] * J[r * N + j];
                M[i * N + j] = s;
            }
        for (int i = 0; i < N; i++) for (int j = 0; j < i; j++) M[j * N + i] = M[i * N + j];
        for (int i = 0; i < N; i++) dmax = M[i * N + i] > dmax ? M[i * N + i] : dmax;
        const double lambda = 1e-5 * dmax * uni();
        for (int i = 0; i < N; i++) M[i * N + i] += lambda;
    }

    void run(int per)
    {
        double ones[N], M[N * N];
        for (int c = 0; c < N; c++) ones[c] = 1.0;
        long plain = 0, scaled = 0, swapped = 0, zeroed = 0, negated = 0, indefinite = 0, zero = 0, nanDiag = 0, nanOff = 0, inf = 0;
        for (int i = 0; i < per; i++, plain++) { normal_matrix(M, ones); need(one(M, "ldlt J^T J + lambda I", i), "J^T J + lambda I is solved"); }
        for (int i = 0; i < per; i++, scaled++) {
            double sc[N];
            for (int c = 0; c < N; c++) sc[c] = std::pow(10.0, -6.0 + 12.0 * c / (N - 1));
            for (int c = N - 1; c > 0; c--) { const int j = (int)(next_u64() % (uint64_t)(c + 1)); const double t = sc[c]; sc[c] = sc[j]; sc[j] = t; }
            normal_matrix(M, sc);
            int big = 0;
            for (int c = 1; c < N; c++) if (sc[c] > sc[big]) big = c;
            swapped += big != 0;   // the first pivot is not entry 0: rows and columns are exchanged
            need(one(M, "ldlt scaled columns", i), "the scaled matrix is solved");
        }
        for (int k = 1; k <= N - 1; k++)
            for (int i = 0; i < per / (N - 1) + 1; i++, zeroed++) {
                normal_matrix(M, ones);
                int idx[N];
                for (int c = 0; c < N; c++) idx[c] = c;
                for (int c = N - 1; c > 0; c--) { const int j = (int)(next_u64() % (uint64_t)(c + 1)); const int t = idx[c]; idx[c] = idx[j]; idx[j] = t; }
                for (int z = 0; z < k; z++) for (int c = 0; c < N; c++) { M[idx[z] * N + c] = 0.0; M[c * N + idx[z]] = 0.0; }
                // N - k pivots, then the largest remaining diagonal entry is exactly zero, below the cutoff: the break
                need(one(M, "ldlt zero rows and columns", zeroed), "a matrix with zero rows is solved (its first pivot is positive)");
            }
        for (int i = 0; i < per; i++, negated++) {
            normal_matrix(M, ones);
            for (int k = 0; k < N * N; k++) M[k] = -M[k];
            need(!one(M, "ldlt negated", i), "the negated matrix is refused");
        }
        for (int i = 0; i < per; i++, indefinite++) {
            normal_matrix(M, ones);
            double dmax = 0.0;
            for (int c = 0; c < N; c++) dmax = M[c * N + c] > dmax ? M[c * N + c] : dmax;
            const int at = (int)(next_u64() % N);
            M[at * N + at] = -(1.0 + uni()) * dmax;   // the largest diagonal entry in magnitude is negative: the sign is taken there
            need(!one(M, "ldlt indefinite", i), "the indefinite matrix is refused");
        }
        for (int k = 0; k < N * N; k++) M[k] = 0.0;
        need(!one(M, "ldlt zero matrix", 0), "the zero matrix is refused");
        zero++;
        for (int i = 0; i < per; i++) {
            const int a = (int)(next_u64() % N), b = (int)(next_u64() % (N - 1));
            const int r = b >= a ? b + 1 : b;   // r != a
            normal_matrix(M, ones); M[a * N + a] = NAN; one(M, "ldlt NaN on the diagonal", i); nanDiag++;
            normal_matrix(M, ones); M[a * N + r] = NAN; M[r * N + a] = NAN; one(M, "ldlt NaN off the diagonal", i); nanOff++;
            normal_matrix(M, ones);
            if (i & 1) M[a * N + a] = signed_of(INFINITY);
            else { M[a * N + r] = signed_of(INFINITY); M[r * N + a] = M[a * N + r]; }
            one(M, "ldlt one infinity", i); inf++;
        }
        std::printf("ldlt_solve<%d>: J^T J + lambda I %ld, scaled columns %ld (%ld with the first pivot exchanged), zero rows and columns %ld, negated %ld, "
                    "indefinite %ld, zero %ld, NaN on the diagonal %ld, NaN off it %ld, one infinity %ld; solved %ld, refused %ld\n",
                    N, plain, scaled, swapped, zeroed, negated, indefinite, zero, nanDiag, nanOff, inf, solvedCount, refusedCount);
        need(plain > 0 && scaled > 0 && swapped > 0 && zeroed >= N - 1 && negated > 0 && indefinite > 0 && zero == 1 && nanDiag > 0 && nanOff > 0 && inf > 0,
             "an LDLT class is empty");
        need(refusedCount >= negated + indefinite + zero && solvedCount >= plain + scaled + zeroed, "LDLT outcomes");
    }
};

// ------------------------------------------------------------------ sin / cos, exp, the canonical NaN
static long g_sincos, g_exp;
static void sincos_one(double x)
{
    double s0, c0, s1, c1;
    pr::definedSinCos(x, s0, c0);
    orbg::sincos_defined(x, s1, c1);
    if (!same(s0, s1) || !same(c0, c1)) { std::printf("x = %.17g\n", x); fail("sincos_defined", g_sincos); }
    g_sincos++;
}
static void exp_one(double x)
{
    if (!same(sr::definedExp(x), orbg::exp_defined(x))) { std::printf("x = %.17g\n", x); fail("exp_defined", g_exp); }
    g_exp++;
}

static void scalars()
{
    long tiny = 0, quarter = 0, general = 0, huge = 0, special = 0;
    for (int i = 0; i < 250000; i++, tiny++) sincos_one(signed_of(log_uniform(1e-300, 1e-5)));
    for (int i = 0; i < 250000; i++, quarter++) {
        const double k = (double)(next_u64() % 1048576ull), at = k * 1.5707963267948966;
        sincos_one(signed_of(at + sym() * ((i & 1) ? 1e-9 : 1e-15 * (1.0 + at))));
    }
    for (int i = 0; i < 300000; i++, general++) sincos_one(sym() * ((i & 1) ? 7.0 : 1048576.0));
    for (int i = 0; i < 250000; i++, huge++) sincos_one(signed_of(log_uniform(1048576.0, 1e300)));
    const double sp[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, -NAN, 1048576.0, -1048576.0, 4503599627370496.0, 1.7976931348623157e308, 4.9406564584124654e-324};
    for (double v : sp) { sincos_one(v); special++; }
    std::printf("sincos_defined: %ld arguments (below 1e-5 %ld, near multiples of pi/2 %ld, general %ld, beyond 2^20 %ld, special %ld)\n", g_sincos, tiny, quarter,
                general, huge, special);
    need(g_sincos >= 1000000 && tiny > 0 && quarter > 0 && huge > 0 && special > 0, "a sin / cos class is empty");

    long range = 0, border = 0, small = 0;
    for (int i = 0; i < 900000; i++, range++) exp_one(-750.0 + 1470.0 * uni());
    for (int i = 0; i < 100000; i++, small++) exp_one(signed_of(log_uniform(1e-300, 1.0)));
    const double edges[] = {709.782712893384, -745.1332191019412, 1023 * 0.6931471805599453, -1022 * 0.6931471805599453, -1023 * 0.6931471805599453,
                            1024 * 0.6931471805599453, -1074 * 0.6931471805599453, -1075 * 0.6931471805599453, 0.0};
    for (double e : edges) {
        double up = e, down = e;
        for (int i = 0; i < 2000; i++, border += 2) { exp_one(up); exp_one(down); up = std::nextafter(up, INFINITY); down = std::nextafter(down, -INFINITY); }
    }
    const double se[] = {NAN, -NAN, INFINITY, -INFINITY, -0.0, 1e300, -1e300, 720.0, -750.0};
    for (double v : se) { exp_one(v); border++; }
    std::printf("exp_defined: %ld arguments ([-750, 720] %ld, below 1 in magnitude %ld, the borders and specials %ld)\n", g_exp, range, small, border);
    need(g_exp >= 1000000 && range > 0 && border > 0, "an exp class is empty");

    for (int k = -1022; k <= 1023; k++) if (!same(sr::pow2Bits(k), orbg::pow2_bits(k))) fail("pow2_bits", k);
    const double nn[] = {NAN, -NAN, 0.0, -0.0, 1.5, INFINITY, -INFINITY, 1e-320, 3.5e38, -1e39};
    for (double v : nn) {
        const double a = pr::nanCanonical(v), b = orbg::nan_canon(v);
        const float fa = pr::nanCanonical((float)v), fb = orbg::nan_canon_f(v);
        if (std::memcmp(&a, &b, 8) != 0 || std::memcmp(&fa, &fb, 4) != 0) fail("nan_canon", 0);   // by bits: the pattern is the point
    }
    std::printf("pow2_bits: 2046 exponents; nan_canon, nan_canon_f: %d values by their exact bits\n", (int)(sizeof nn / sizeof nn[0]));
}

// ------------------------------------------------------------------ the quaternion of a matrix, the two oplus, the inverse
static void rotation(const double axisIn[3], double angle, double R[9])
{
    const double n = std::sqrt(axisIn[0] * axisIn[0] + axisIn[1] * axisIn[1] + axisIn[2] * axisIn[2]);
    const double x = axisIn[0] / n, y = axisIn[1] / n, z = axisIn[2] / n, c = std::cos(angle), s = std::sin(angle), t = 1.0 - c;
    const double M[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c, t * y * z - s * x,
                         t * x * z - s * y, t * y * z + s * x, t * z * z + c};
    for (int k = 0; k < 9; k++) R[k] = M[k];
}

static void random_quat(double q[4], bool unit)
{
    double n = 0.0;
    for (int i = 0; i < 4; i++) { q[i] = sym(); n += q[i] * q[i]; }
    n = std::sqrt(n) / (unit ? 1.0 : 0.5 + uni());
    for (int i = 0; i < 4; i++) q[i] /= n;
}

static void quaternions()
{
    long branch[4] = {0, 0, 0, 0};
    for (long i = 0; i < 200000; i++) {
        double R[9], axis[3] = {sym(), sym(), sym()};
        const int kind = (int)(i % 5);
        if (kind < 3) { axis[kind] += 4.0; rotation(axis, 3.141592653589793 - 0.3 * uni(), R); }   // a turn near pi about (nearly) one axis: that diagonal wins
        else if (kind == 3) rotation(axis, 3.0 * sym(), R);
        else for (int k = 0; k < 9; k++) R[k] = sym();                                              // not a rotation: taken as it is
        double q0[4];
        pr::quatFromMatrix(R, q0);
        const orbg::Quat q1 = orbg::quat_of_matrix(R);
        const double q1a[4] = {q1.x, q1.y, q1.z, q1.w};
        if (!same_n(q0, q1a, 4)) fail("quat_of_matrix", i);
        const double t = R[0] + R[4] + R[8];
        int b = 0;
        if (!(t > 0.0)) { int m = 0; if (R[4] > R[0]) m = 1; if (R[8] > R[m * 4]) m = 2; b = 1 + m; }
        branch[b]++;
        double n0[4] = {q0[0], q0[1], q0[2], q0[3]};
        orbg::Quat n1 = q1;
        pr::normalizeRotation(n0);
        orbg::normalize_rotation(n1);
        const double n1a[4] = {n1.x, n1.y, n1.z, n1.w};
        if (!same_n(n0, n1a, 4)) fail("normalize_rotation", i);
    }
    std::printf("quat_of_matrix, normalize_rotation: positive trace %ld, largest diagonal 0 / 1 / 2: %ld / %ld / %ld\n", branch[0], branch[1], branch[2], branch[3]);
    need(branch[0] > 0 && branch[1] > 0 && branch[2] > 0 && branch[3] > 0, "a quat_of_matrix branch is empty");
}

static double step_size(int cls) { return cls == 0 ? 0.0 : cls == 1 ? log_uniform(1e-12, 9e-6) / 2.0 : cls == 2 ? log_uniform(2e-5, 1e-2) : log_uniform(1e-2, 20.0); }

static void oplus_se3()
{
    long smallTheta = 0, largeTheta = 0;
    for (long i = 0; i < 200000; i++) {
        pr::SE3 est;
        random_quat(est.q, true);
        for (int k = 0; k < 3; k++) est.t[k] = sym() * 10.0;
        double x[6];
        const double mag = step_size((int)(i % 4));
        for (int k = 0; k < 3; k++) x[k] = sym() * mag;
        for (int k = 3; k < 6; k++) x[k] = sym() * ((i & 4) ? 1.0 : 1e-6);
        const pr::SE3 r = pr::se3Mul(pr::se3Exp<pr::Defined>(x), est);
        orbo::Pose P;
        P.q = {est.q[0], est.q[1], est.q[2], est.q[3]};
        P.tx = est.t[0]; P.ty = est.t[1]; P.tz = est.t[2];
        const orbo::Pose O = orbo::oplus(P, x[0], x[1], x[2], x[3], x[4], x[5]);
        const double a[7] = {r.q[0], r.q[1], r.q[2], r.q[3], r.t[0], r.t[1], r.t[2]}, b[7] = {O.q.x, O.q.y, O.q.z, O.q.w, O.tx, O.ty, O.tz};
        if (!same_n(a, b, 7)) fail("the SE3 oplus", i);
        (std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) < 0.00001 ? smallTheta : largeTheta)++;
    }
    // Converter::toSE3Quat, which opens every round
    for (long i = 0; i < 20000; i++) {
        double R[9], axis[3] = {sym(), sym(), sym()};
        rotation(axis, 3.2 * sym(), R);
        float T[16] = {0};
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r * 3 + c]; T[r * 4 + 3] = (float)(sym() * 5.0); }
        T[15] = 1.f;
        const pr::SE3 r = pr::toSE3Quat(T);
        const orbo::Pose P = orbo::pose_of_tcw(T);
        const double a[7] = {r.q[0], r.q[1], r.q[2], r.q[3], r.t[0], r.t[1], r.t[2]}, b[7] = {P.q.x, P.q.y, P.q.z, P.q.w, P.tx, P.ty, P.tz};
        if (!same_n(a, b, 7)) fail("pose_of_tcw", i);
    }
    std::printf("the SE3 oplus: theta below 1e-5 %ld, above %ld; pose_of_tcw 20000\n", smallTheta, largeTheta);
    need(smallTheta > 0 && largeTheta > 0, "an SE3 oplus branch is empty");
}

static void oplus_sim3()
{
    long cls[2][2] = {{0, 0}, {0, 0}}, fixed = 0;
    for (long i = 0; i < 400000; i++) {
        sr::Sim3 est;
        random_quat(est.q, (i & 8) != 0);   // Sim3's product does not normalise: the quaternion need not be a unit one
        for (int k = 0; k < 3; k++) est.t[k] = sym() * 10.0;
        est.s = log_uniform(0.1, 10.0);
        double x[7];
        const double mag = step_size((int)(i % 4));
        for (int k = 0; k < 3; k++) x[k] = sym() * mag;
        for (int k = 3; k < 6; k++) x[k] = sym() * ((i & 4) ? 1.0 : 1e-6);
        const int sc = (int)((i / 4) % 4);
        x[6] = sc == 0 ? 0.0 : sc == 1 ? signed_of(log_uniform(1e-12, 9e-6)) : sc == 2 ? signed_of(log_uniform(2e-5, 1e-2)) : sym() * 3.0;
        const bool fixScale = (i % 16) == 15;
        // oplusImpl writes the zero into the solver's x before the step is applied: the kernel's step hook does the same
        const double sigma = fixScale ? 0.0 : x[6];
        const sr::Sim3 r = sr::oplus<sr::Defined>(est, x, fixScale);
        if (!same(x[6], sigma)) fail("the zero of fix_scale in x", i);
        orbz::S3 P;
        P.q = {est.q[0], est.q[1], est.q[2], est.q[3]};
        P.tx = est.t[0]; P.ty = est.t[1]; P.tz = est.t[2]; P.s = est.s;
        const orbz::S3 O = orbz::oplus(P, x[0], x[1], x[2], x[3], x[4], x[5], sigma);
        const double a[8] = {r.q[0], r.q[1], r.q[2], r.q[3], r.t[0], r.t[1], r.t[2], r.s}, b[8] = {O.q.x, O.q.y, O.q.z, O.q.w, O.tx, O.ty, O.tz, O.s};
        if (!same_n(a, b, 8)) fail("the Sim3 oplus", i);
        const sr::Sim3 ri = sr::sim3Inverse(r);
        const orbz::S3 Oi = orbz::inverse(O);
        const double ai[8] = {ri.q[0], ri.q[1], ri.q[2], ri.q[3], ri.t[0], ri.t[1], ri.t[2], ri.s}, bi[8] = {Oi.q.x, Oi.q.y, Oi.q.z, Oi.q.w, Oi.tx, Oi.ty, Oi.tz, Oi.s};
        if (!same_n(ai, bi, 8)) fail("the Sim3 inverse", i);
        cls[std::fabs(sigma) < 0.00001 ? 0 : 1][std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) < 0.00001 ? 0 : 1]++;
        fixed += fixScale;
    }
    std::printf("the Sim3 oplus and inverse: |sigma| < 1e-5 with theta below / above 1e-5: %ld / %ld, |sigma| above with theta below / above: %ld / %ld; "
                "fix_scale %ld\n", cls[0][0], cls[0][1], cls[1][0], cls[1][1], fixed);
    need(cls[0][0] > 0 && cls[0][1] > 0 && cls[1][0] > 0 && cls[1][1] > 0 && fixed > 0, "a Sim3 oplus branch is empty");
}

int main(int argc, char** argv)
{
    g_state = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20240607ull;
    Ldlt<6> l6;
    l6.run(3000);
    Ldlt<7> l7;
    l7.run(3000);
    scalars();
    quaternions();
    oplus_se3();
    oplus_sim3();
    std::printf("g2o core: all equal\n");
    return 0;
}
