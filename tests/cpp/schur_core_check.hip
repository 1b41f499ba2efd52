// schur_core_check.hip -- the host instantiations of orbg_schur.hip's scalar pieces against the restatement's functions
// (tools/initmap_ref.hpp), as bits, on seeded inputs; no device, no HIP runtime call.  Prints a count per class, stops at the
// first mismatch (exit status 1) and asserts that no class is empty: the reduced solve's refusals (a zero pivot, a pivot that is
// not finite), a singular landmark block and the non-robust form of Hpl are reached by few or none of the scene families.
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -o schur_core_check tests/cpp/schur_core_check.hip && ./schur_core_check
// The same source is built once more with -Xarch_host -fsanitize=address,undefined and run as a stand-alone program.
// A NaN equals a NaN here whatever its sign and payload: the kernels canonicalise theirs on the way out.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../orbslamm_amd/csrc/orbg_schur.hip"
#include "../../tools/initmap_ref.hpp"

namespace ir = initmap_ref;

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

// ------------------------------------------------------------------ Eigen's 3 x 3 inverse
static void check_inverse3()
{
    long regular = 0, singular = 0;
    for (long i = 0; i < 200000; i++) {
        double M[9], a[9], b[9];
        const int kind = (int)(next_u64() % 8);
        for (int k = 0; k < 9; k++) M[k] = sym() * std::pow(10.0, 6.0 * sym());
        if (kind == 0) for (int k = 0; k < 3; k++) M[6 + k] = M[k] * 2.0;     // a rank deficit: det 0 or rounding's
        if (kind == 1) for (int k = 0; k < 9; k++) M[k] = 0.0;
        if (kind == 2) M[4] = INFINITY;
        orbg::inverse3(M, a);
        ir::inverse3(M, b);
        if (!same_n(a, b, 9)) fail("inverse3", i);
        if (a[0] - a[0] == 0.0) regular++; else singular++;
    }
    need(regular > 100000 && singular > 10000, "inverse3 classes");
    std::printf("inverse3: %ld regular, %ld not finite\n", regular, singular);
}

// ------------------------------------------------------------------ the reduced solve
template <int N> static void check_ldlt()
{
    long solved = 0, zeroPivot = 0, notFinite = 0;
    for (long i = 0; i < 60000; i++) {
        double A[N * N], Ma[144], Mb[144], rhs[12], xa[12], xb[12], w[12], y[12];
        const int kind = (int)(next_u64() % 10);
        // G G^T + shift on the lower triangle (what is above the diagonal is never read: it gets a NaN to show it)
        double G[N * N];
        for (int k = 0; k < N * N; k++) G[k] = sym();
        for (int r = 0; r < N; r++)
            for (int c = 0; c < N; c++) {
                double s = 0;
                for (int k = 0; k < N; k++) s += G[r * N + k] * G[c * N + k];
                A[r * N + c] = c <= r ? s + (r == c ? 0.1 : 0.0) : NAN;
            }
        if (kind == 0) A[0] = 0.0;                                            // a zero first pivot
        if (kind == 1) { for (int c = 0; c <= N / 2; c++) A[(N / 2) * N + c] = 0.0; for (int r = N / 2; r < N; r++) A[r * N + N / 2] = 0.0; }   // a zero pivot later
        if (kind == 2) A[(N - 1) * N + 1] = INFINITY;
        if (kind == 3) A[(N / 2) * N + N / 2] = NAN;
        if (kind == 4) for (int r = 0; r < N; r++) A[r * N + r] = -A[r * N + r];   // indefinite: unpivoted LDLt still runs
        for (int k = 0; k < N; k++) { rhs[k] = sym() * 10.0; xa[k] = xb[k] = 7.0 + k; }
        for (int k = 0; k < N * N; k++) { Ma[k] = A[k]; Mb[k] = A[k]; }
        const bool oa = orbg::ldlt_plain(N, Ma, rhs, xa, w, y), ob = ir::ldltPlain(N, Mb, rhs, xb);
        if (oa != ob || !same_n(xa, xb, N)) fail("ldlt_plain", i);
        if (oa) { solved++; for (int k = 0; k < N; k++) if (xa[k] != xa[k]) fail("ldlt_plain: a NaN behind a success", i); }
        else {
            for (int k = 0; k < N; k++) if (xa[k] != 7.0 + k) fail("ldlt_plain: x written by a refusal", i);
            if (kind == 0 || kind == 1) zeroPivot++; else notFinite++;
        }
    }
    need(solved > 30000 && zeroPivot > 5000 && notFinite > 5000, "ldlt_plain classes");
    std::printf("ldlt_plain<%d>: %ld solved, %ld zero pivots, %ld pivots not finite\n", N, solved, zeroPivot, notFinite);
}

// ------------------------------------------------------------------ the edge, a landmark's blocks, its Schur share, its step
static void check_point_pieces()
{
    long robustEdges = 0, plainEdges = 0, huberOn = 0, fixedPoses = 0, planePoints = 0, points = 0;
    const float deltaF = std::sqrt(5.99);
    const double delta = (double)deltaF, dsqr = delta * delta;
    for (long i = 0; i < 40000; i++) {
        const bool robust = (next_u64() & 3) != 0;
        bool fixed[2] = {(next_u64() % 3) == 0, false};
        if (!fixed[0]) fixed[1] = (next_u64() % 5) == 0;
        const orbg::Cam K = {500.0 + 50 * sym(), 500.0 + 50 * sym(), 320.0 + 5 * sym(), 240.0 + 5 * sym()};
        const ir::Cam Kr = {K.fx, K.fy, K.cx, K.cy};
        double X[3] = {2.0 * sym(), 2.0 * sym(), 4.0 + 3.0 * uni()};
        const bool plane = (next_u64() % 50) == 0;
        orbg::SE3Pose P[2];
        ir::SE3 Pr[2];
        double Da[9] = {0}, Db[9] = {0}, ba[3] = {0}, bb[3] = {0}, Bpa[2][18], Bpb[36], Ha[2][21], Hb[2][21], ta[2][6], tb[2][6];
        for (int s = 0; s < 2; s++) {
            double q[4] = {0.1 * sym(), 0.1 * sym(), 0.1 * sym(), 1.0};
            const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            for (int k = 0; k < 4; k++) q[k] /= nq;
            if (plane && s == 1) { q[0] = q[1] = q[2] = 0.0; q[3] = 1.0; }
            P[s].q = {q[0], q[1], q[2], q[3]};
            P[s].tx = 0.3 * sym(); P[s].ty = 0.3 * sym(); P[s].tz = plane && s == 1 ? -X[2] : 0.3 * sym();   // z = 0 in camera 1: the point ON its plane
            for (int k = 0; k < 4; k++) Pr[s].q[k] = q[k];
            Pr[s].t[0] = P[s].tx; Pr[s].t[1] = P[s].ty; Pr[s].t[2] = P[s].tz;
            ir::Obs o;
            const float w = (float)std::pow(1.2, -2.0 * (double)(next_u64() % 8)) * ((next_u64() % 40) == 0 ? 0.f : 1.f);
            const double big = (next_u64() % 4) == 0 ? 30.0 : 1.0;   // a gross observation: the Huber branch
            double x, y, z;
            orbg::se3_map(P[s], X[0], X[1], X[2], x, y, z);
            o.uv[0] = (double)(float)(K.fx * x / (z == 0 ? 1 : z) + K.cx + big * sym());
            o.uv[1] = (double)(float)(K.fy * y / (z == 0 ? 1 : z) + K.cy + big * sym());
            o.Om[0] = 1.0 * (double)w; o.Om[1] = 0.0 * (double)w; o.Om[2] = 0.0 * (double)w; o.Om[3] = 1.0 * (double)w;
            orbg::EdgeReg E = orbg::load_edge(make_float4(0.f, 0.f, 0.f, w), make_float2((float)o.uv[0], (float)o.uv[1]));
            E.X = X[0]; E.Y = X[1]; E.Z = X[2];
            double R[9];
            orbg::quat_to_matrix(P[s].q, R);
            orbg::EdgeLin L;
            orbg::linearize_xyz(P[s], R, K, E, L);
            double err[2], A[6], B[12];
            ir::computeError(Pr[s], Kr, X, o, err);
            ir::linearizeOplus(Pr[s], Kr, X, A, B);
            if (!same(L.e0, err[0]) || !same(L.e1, err[1]) || !same_n(L.A, A, 6) || !same_n(L.B, B, 12)) fail("linearize_xyz", i);
            for (int k = 0; k < 18; k++) { Bpa[s][k] = 0.0; Bpb[18 * s + k] = 0.0; }
            for (int k = 0; k < 21; k++) { Ha[s][k] = 0.5; Hb[s][k] = 0.5; }
            for (int k = 0; k < 6; k++) { ta[s][k] = 0.5; tb[s][k] = 0.5; }
            orbg::quadratic_form(E, L, robust, delta, dsqr, fixed[s], Da, ba, Bpa[s], Ha[s], ta[s]);
            const double c = ir::edgeQuadraticForm(Pr[s], Kr, X, o, robust, delta, dsqr, fixed[s], Db, bb, Bpb + 18 * s, Hb[s], tb[s]);
            if (!same_n(Bpa[s], Bpb + 18 * s, 18) || !same_n(Ha[s], Hb[s], 21) || !same_n(ta[s], tb[s], 6)) fail("quadratic_form: the pose's terms", i);
            if (robust) { robustEdges++; if (c > dsqr) huberOn++; } else plainEdges++;
            if (fixed[s]) fixedPoses++;
        }
        if (!same_n(Da, Db, 9) || !same_n(ba, bb, 3)) fail("quadratic_form: the point's block", i);
        if (plane) planePoints++;
        // the Schur share and the step
        const double lambda = (next_u64() % 20) == 0 ? 0.0 : std::pow(10.0, 4.0 * sym());
        double Dia[9], Dib[9], Ca[12], Cb[12], Sa[orbg::kSchurTerms], Sb[78];
        for (int k = 0; k < 12; k++) { Ca[k] = 0.25; Cb[k] = 0.25; }
        for (int k = 0; k < 78; k++) { Sa[k] = 0.25; Sb[k] = 0.25; }
        orbg::schur_point(Da, ba, Bpa[0], Bpa[1], fixed[0], fixed[1], lambda, Dia, Ca, Sa);
        ir::pointSchur(Db, bb, Bpb, fixed, lambda, Dib, Cb, Sb);
        if (!same_n(Dia, Dib, 9) || !same_n(Ca, Cb, 12) || !same_n(Sa, Sb, 78)) fail("schur_point", i);
        double xp[12], xla[3], xlb[3];
        for (int k = 0; k < 12; k++) xp[k] = 0.01 * sym();
        int freeOf[2], nFree = 0;
        for (int s = 0; s < 2; s++) if (!fixed[s]) freeOf[nFree++] = s;
        orbg::back_substitute(ba, Bpa[0], Bpa[1], fixed[0], fixed[1], xp, fixed[0] ? xp : xp + 6, Dia, xla);
        ir::pointBackSubstitute(bb, Bpb, freeOf, nFree, xp, Dib, xlb);
        if (!same_n(xla, xlb, 3)) fail("back_substitute", i);
        // the reduced system's assembly from arbitrary sums
        double S[78], bp[12], cf[12], Ma[144], Mb[144], bsa[12] = {0}, bsb[12] = {0};
        for (int k = 0; k < 78; k++) S[k] = sym();
        for (int k = 0; k < 12; k++) { bp[k] = sym(); cf[k] = sym(); }
        orbg::assemble_reduced(S, bp, cf, nFree, fixed[0] ? 1 : 0, Ma, bsa);
        ir::assembleReduced(S, bp, cf, freeOf, nFree, Mb, bsb);
        if (!same_n(Ma, Mb, 36 * nFree * nFree) || !same_n(bsa, bsb, 6 * nFree)) fail("assemble_reduced", i);
        points++;
    }
    need(robustEdges > 20000 && plainEdges > 5000 && huberOn > 2000 && fixedPoses > 5000 && planePoints > 200, "point classes");
    std::printf("points: %ld (%ld robust edges, %ld with the Huber branch, %ld plain, %ld on fixed poses, %ld points on a camera's plane)\n", points,
                robustEdges, huberOn, plainEdges, fixedPoses, planePoints);
}

int main()
{
    g_state = 0x5C4E5EEDull;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++)
            if (orbg::upper_index(i, j) != ir::upperIndex(i, j)) fail("upper_index", i * 6 + j);
    need(orbg::kSchurTerms == 78 && orbg::kS01 == 21 && orbg::kS11 == 57, "the Schur layout");
    check_inverse3();
    check_ldlt<6>();
    check_ldlt<12>();
    check_point_pieces();
    std::printf("schur core ok\n");
    return 0;
}
