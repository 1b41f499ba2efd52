// poseopt_ref.hpp -- an independent restatement of Optimizer::PoseOptimization (src/Optimizer.cc:261-473; `ref:LINE` cites
// it), monocular, for the tests and for tools/poseopt_bench.py: the motion-only Levenberg that Tracking runs on every frame,
// on the host, in plain C++11 with the standard library alone.  It shares no header with the library.  The g2o and Eigen
// pieces the reference calls are restated here on their own (`g2o:FILE:LINE` cites Thirdparty/g2o/g2o/FILE; Eigen is cited
// by function, as of Eigen 3.2.0: no Eigen is installed, so parity against g2o itself is UNPINNED, as DESIGN.md §2 says of
// OpenCV).  Build with -ffp-contract=off: one IEEE operation per source operation.
//
// Two arithmetic modes, chosen by the template parameter:
//   Serial   sums the edges' H, b and chi2 in edge order, calls libm's sin, cos and pow: the reading closest to the reference.
//   Defined  what the device is held to bit for bit:
//     THE SUMMATION TREE.  Every sum over edges (the 21 entries of H's lower triangle, the 6 of b, the robust chi2) is taken by
//       one tree that depends on the frame's edge count alone: edge e of the frame goes to partial e % 64; each of the 64
//       partials starts at +0.0 and takes its edges in ascending order (an edge at level 1 is skipped, it adds nothing); then
//       six exchange steps m = 32, 16, 8, 4, 2, 1 replace every partial l by p[l] + p[l ^ m] (all 64 at once), and
//       partial 0 is the sum.  b is built as p = p - term, and the exchange steps add.
//     x^3 is x * x * x, left to right.
//     sin / cos are definedSinCos below: + - * /, comparisons and integer conversion only, for every finite argument.
//     sqrt and / are the IEEE operations.
//     A NaN among the outputs (Tcw, lambda, chi2) leaves as x86's default NaN, whatever its sign and payload were (nanCanonical).
//
// Readings chosen where Eigen leaves a choice to the build (vectorisation): every inner product and redux is taken
// sequentially in index order; the quaternion product is the generic one.  LDLT reads the LOWER triangle of H, so the 21
// entries kept are (i, j), i >= j, of A^T W A as Eigen evaluates it: (A^T W)(i, :) . A(:, j).
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace poseopt_ref {

struct Serial {};
struct Defined {};

// ------------------------------------------------------------------ the Defined sin / cos
// |x| is reduced to r = |x| - k * (pi/2), k = (int64)(|x| * (2/pi) + 0.5), with pi/2 in three parts (P1, P2: 33 bits each,
// so k * P1 and k * P2 are exact for k < 2^20; P3: the rest, rounded), then sin r and cos r are Taylor polynomials on
// |r| <= pi/4 (to r^17 and r^16: the next terms are below 2^-62 relative) in Horner form, and the quadrant k & 3 picks and
// signs them.  An argument of 2^20 or more is first brought below 2^20 by x = x - trunc(x / 2pi) * 2pi, at most 24 times
// (defined and the same on both sides; not accurate, and no Levenberg step gets there); trunc is the int64 conversion below
// 2^52 and the identity above.  A NaN or an infinity gives NaN for both.
inline double truncDefined(double q)
{
    const double a = q < 0 ? -q : q;
    if (!(a < 4503599627370496.0)) return q;   // 2^52: already an integer (or NaN / inf)
    return (double)(int64_t)q;
}

inline void definedSinCos(double x, double& s, double& c)
{
    if (!(x - x == 0.0)) { s = x - x; c = x - x; return; }   // NaN, +-inf -> NaN
    const bool neg = x < 0;
    double a = neg ? -x : x;
    const double kBig = 1048576.0, kTwoPi = 6.283185307179586;
    for (int i = 0; i < 24; i++) {
        if (a < kBig) break;
        a = a - truncDefined(a / kTwoPi) * kTwoPi;
        if (a < 0) a = -a;
    }
    if (!(a < kBig)) a = 0.0;
    const double P1 = 1.5707963267341256, P2 = 6.077100506303966e-11, P3 = 2.0222662487959506e-21, kTwoOverPi = 0.6366197723675814;
    const int64_t k = (int64_t)(a * kTwoOverPi + 0.5);
    const double kd = (double)k;
    const double r = ((a - kd * P1) - kd * P2) - kd * P3;
    const double z = r * r;
    double ps = 1.0 / 355687428096000.0;                 // 1/17!
    ps = ps * z - 1.0 / 1307674368000.0;                 // 1/15!
    ps = ps * z + 1.0 / 6227020800.0;                    // 1/13!
    ps = ps * z - 1.0 / 39916800.0;                      // 1/11!
    ps = ps * z + 1.0 / 362880.0;                        // 1/9!
    ps = ps * z - 1.0 / 5040.0;                          // 1/7!
    ps = ps * z + 1.0 / 120.0;                           // 1/5!
    ps = ps * z - 1.0 / 6.0;                             // 1/3!
    const double sr = r + r * (z * ps);
    double pc = 1.0 / 20922789888000.0;                  // 1/16!
    pc = pc * z - 1.0 / 87178291200.0;                   // 1/14!
    pc = pc * z + 1.0 / 479001600.0;                     // 1/12!
    pc = pc * z - 1.0 / 3628800.0;                       // 1/10!
    pc = pc * z + 1.0 / 40320.0;                         // 1/8!
    pc = pc * z - 1.0 / 720.0;                           // 1/6!
    pc = pc * z + 1.0 / 24.0;                            // 1/4!
    pc = pc * z - 0.5;                                   // 1/2!
    const double cr = 1.0 + z * pc;
    const int n = (int)(k & 3);
    double ss, cc;
    if (n == 0) { ss = sr; cc = cr; }
    else if (n == 1) { ss = cr; cc = -sr; }
    else if (n == 2) { ss = -sr; cc = -cr; }
    else { ss = -cr; cc = sr; }
    s = neg ? -ss : ss;
    c = cc;
}

template <class Mode> struct Arith;
template <> struct Arith<Serial> {
    enum { kPartials = 1 };
    static void sincos(double x, double& s, double& c) { s = std::sin(x); c = std::cos(x); }
    static double cube(double x) { return std::pow(x, 3); }
};
template <> struct Arith<Defined> {
    enum { kPartials = 64 };
    static void sincos(double x, double& s, double& c) { definedSinCos(x, s, c); }
    static double cube(double x) { return x * x * x; }
};

// K sums over the edges of a frame, by the mode's rule (the header comment: THE SUMMATION TREE)
template <class Mode, int K> struct EdgeSums {
    enum { P = Arith<Mode>::kPartials };
    double p[P][K];
    EdgeSums() { for (int l = 0; l < P; l++) for (int k = 0; k < K; k++) p[l][k] = 0.0; }
    void add(int edge, int k, double v) { p[edge % P][k] = p[edge % P][k] + v; }
    void sub(int edge, int k, double v) { p[edge % P][k] = p[edge % P][k] - v; }
    void total(double out[K])
    {
        for (int m = P / 2; m >= 1; m /= 2) {
            double q[P][K];
            for (int l = 0; l < P; l++) for (int k = 0; k < K; k++) q[l][k] = p[l][k] + p[l ^ m][k];
            std::memcpy(p, q, sizeof q);
        }
        for (int k = 0; k < K; k++) out[k] = p[0][k];
    }
};

// ------------------------------------------------------------------ Eigen's quaternion, g2o's SE3Quat
struct SE3 { double q[4]; double t[3]; };   // q: x y z w, Eigen's coefficient order

// Quaterniond(R): Eigen quaternionbase_assign_impl<Matrix3d, 3, 3>::run; R row-major
inline void quatFromMatrix(const double R[9], double q[4])
{
    double t = R[0] + R[4] + R[8];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[2 * 3 + 1] - R[1 * 3 + 2]) * t;
        q[1] = (R[0 * 3 + 2] - R[2 * 3 + 0]) * t;
        q[2] = (R[1 * 3 + 0] - R[0 * 3 + 1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
        q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
        q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    }
}

// SE3Quat::normalizeRotation (g2o:types/se3quat.h:280-285) over Eigen's normalize(): coeffs /= sqrt(x^2 + y^2 + z^2 + w^2)
inline void normalizeRotation(double q[4])
{
    if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = q[i] * -1.0;
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] = q[i] / n;
}

// Eigen quat_product (the generic one)
inline void quatMul(const double a[4], const double b[4], double o[4])
{
    const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

// q * v: Eigen QuaternionBase::_transformVector
inline void quatRotate(const double q[4], const double v[3], double o[3])
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; i++) o[i] = (v[i] + q[3] * uv[i]) + c[i];
}

// Eigen QuaternionBase::toRotationMatrix, row-major out
inline void quatToMatrix(const double q[4], double R[9])
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// Converter::toSE3Quat (src/Converter.cc:37-47): the floats widened, SE3Quat(R, t) (g2o:types/se3quat.h:58-60)
inline SE3 toSE3Quat(const float T[16])
{
    double R[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R[r * 3 + c] = (double)T[r * 4 + c];
    SE3 s;
    quatFromMatrix(R, s.q);
    for (int r = 0; r < 3; r++) s.t[r] = (double)T[r * 4 + 3];
    normalizeRotation(s.q);
    return s;
}

// Converter::toCvMat(SE3Quat) (src/Converter.cc:49-71) over to_homogeneous_matrix (g2o:types/se3quat.h:270-278)
inline void toCvMat(const SE3& s, float T[16])
{
    double R[9];
    quatToMatrix(s.q, R);
    for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r * 3 + c];
        T[r * 4 + 3] = (float)s.t[r];
    }
}

// SE3Quat::map (g2o:types/se3quat.h:217-220)
inline void se3Map(const SE3& s, const double p[3], double o[3])
{
    double r[3];
    quatRotate(s.q, p, r);
    for (int i = 0; i < 3; i++) o[i] = r[i] + s.t[i];
}

// SE3Quat::operator* (g2o:types/se3quat.h:104-110)
inline SE3 se3Mul(const SE3& a, const SE3& b)
{
    SE3 o;
    double r[3];
    quatRotate(a.q, b.t, r);
    for (int i = 0; i < 3; i++) o.t[i] = a.t[i] + r[i];
    quatMul(a.q, b.q, o.q);
    normalizeRotation(o.q);
    return o;
}

inline void mat3Mul(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}

// SE3Quat::exp (g2o:types/se3quat.h:223-257); update = (omega, upsilon)
template <class Mode> inline SE3 se3Exp(const double u[6])
{
    const double theta = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double Om[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};   // skew (g2o:types/se3_ops.hpp:27-38)
    const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double Om2[9], R[9], V[9];
    mat3Mul(Om, Om, Om2);
    if (theta < 0.00001) {
        for (int k = 0; k < 9; k++) { R[k] = (I[k] + Om[k]) + Om2[k]; V[k] = R[k]; }
    } else {
        double s, c;
        Arith<Mode>::sincos(theta, s, c);
        const double a = s / theta, b = (1.0 - c) / (theta * theta), d = (theta - s) / Arith<Mode>::cube(theta);
        for (int k = 0; k < 9; k++) { R[k] = (I[k] + a * Om[k]) + b * Om2[k]; V[k] = (I[k] + b * Om[k]) + d * Om2[k]; }
    }
    SE3 o;
    quatFromMatrix(R, o.q);
    for (int i = 0; i < 3; i++) o.t[i] = (V[i * 3] * u[3] + V[i * 3 + 1] * u[4]) + V[i * 3 + 2] * u[5];
    normalizeRotation(o.q);   // SE3Quat(q, t)
    return o;
}

// ------------------------------------------------------------------ the edge (g2o:types/types_six_dof_expmap.h:145-173, .cpp:266-296)
struct Edge {       // after the pointer chasing of ref:302-341
    float u, v;     // mvKeysUn[i].pt
    float invSigma2;   // mvInvLevelSigma2[octave]
    float Xw[3];    // GetWorldPos()
};
struct EdgeD { double obs[2], Om[4], Xw[3]; };
struct Cam { double fx, fy, cx, cy; };

inline EdgeD widen(const Edge& e)
{
    EdgeD d;
    d.obs[0] = (double)e.u; d.obs[1] = (double)e.v;
    const double w = (double)e.invSigma2;   // Matrix2d::Identity() * invSigma2 (ref:322)
    d.Om[0] = 1.0 * w; d.Om[1] = 0.0 * w; d.Om[2] = 0.0 * w; d.Om[3] = 1.0 * w;
    for (int i = 0; i < 3; i++) d.Xw[i] = (double)e.Xw[i];
    return d;
}

// computeError: obs - cam_project(estimate.map(Xw))
inline void computeError(const SE3& est, const Cam& K, const EdgeD& e, double err[2])
{
    double p[3];
    se3Map(est, e.Xw, p);
    const double px = p[0] / p[2], py = p[1] / p[2];
    err[0] = e.obs[0] - (px * K.fx + K.cx);
    err[1] = e.obs[1] - (py * K.fy + K.cy);
}

// chi2 = e . (Omega e)  (g2o:core/base_edge.h)
inline double chi2Of(const double err[2], const double Om[4])
{
    const double t0 = Om[0] * err[0] + Om[1] * err[1], t1 = Om[2] * err[0] + Om[3] * err[1];
    return err[0] * t0 + err[1] * t1;
}

// RobustKernelHuber::robustify (g2o:core/robust_kernel_impl.cpp:78-91)
inline void huber(double e, double delta, double dsqr, double rho[3])
{
    if (e <= dsqr) { rho[0] = e; rho[1] = 1.; rho[2] = 0.; }
    else {
        const double root = std::sqrt(e);
        rho[0] = 2 * root * delta - dsqr;
        rho[1] = delta / root;
        rho[2] = -0.5 * rho[1] / e;
    }
}

inline void linearizeOplus(const SE3& est, const Cam& K, const EdgeD& e, double A[12])
{
    double p[3];
    se3Map(est, e.Xw, p);
    // (the operation order is the edge type's: x*y*iz2*fx is ((x*y)*iz2)*fx, -x*y*... negates x first, which gives -(x*y)'s bits)
    const double x = p[0], y = p[1], iz = 1.0 / p[2], iz2 = iz * iz, xy = x * y;
    A[0] = xy * iz2 * K.fx;
    A[1] = -(1.0 + x * x * iz2) * K.fx;
    A[2] = y * iz * K.fx;
    A[3] = -iz * K.fx;
    A[4] = 0.0;
    A[5] = x * iz2 * K.fx;
    A[6] = (1.0 + y * y * iz2) * K.fy;
    A[7] = -xy * iz2 * K.fy;
    A[8] = -x * iz * K.fy;
    A[9] = 0.0;
    A[10] = -iz * K.fy;
    A[11] = y * iz2 * K.fy;
}

// ------------------------------------------------------------------ Eigen::LDLT<MatrixXd, Lower> (3.2.0), n = 6
// ldlt_inplace<Lower>::unblocked with diagonal pivoting on the lower triangle of M (row-major, full storage), the sign taken
// at the first pivot as that version does; then LDLT::solve.  Returns isPositive() and, when positive, x.
// std::max of the tolerance is the ternary (a < b) ? b : a, so a NaN behaves as it does there.
inline bool ldltSolve6(double M[36], const double b[6], double x[6])
{
    const int n = 6;
    int tr[6];
    double temp[6];
    double cutoff = 0.0;
    int sign = 0;
    for (int k = 0; k < n; k++) {
        // mat.diagonal().tail(n - k).cwiseAbs().maxCoeff(&idx): the first of the largest; a NaN never wins a `>`
        int big = k;
        double biggest = std::fabs(M[k * n + k]);
        for (int i = k + 1; i < n; i++) { const double a = std::fabs(M[i * n + i]); if (a > biggest) { biggest = a; big = i; } }
        if (k == 0) {
            cutoff = std::fabs(DBL_EPSILON * biggest);
            sign = M[big * n + big] > 0 ? 1 : -1;
        }
        if (biggest < cutoff) {
            for (int i = k; i < n; i++) tr[i] = i;
            break;
        }
        tr[k] = big;
        if (k != big) {
            const int s = n - big - 1;
            for (int c = 0; c < k; c++) { const double t = M[k * n + c]; M[k * n + c] = M[big * n + c]; M[big * n + c] = t; }
            for (int r = 0; r < s; r++) {
                const int row = n - s + r;
                const double t = M[row * n + k]; M[row * n + k] = M[row * n + big]; M[row * n + big] = t;
            }
            { const double t = M[k * n + k]; M[k * n + k] = M[big * n + big]; M[big * n + big] = t; }
            for (int i = k + 1; i < big; i++) { const double t = M[i * n + k]; M[i * n + k] = M[big * n + i]; M[big * n + i] = t; }
        }
        const int rs = n - k - 1;
        if (k > 0) {
            for (int c = 0; c < k; c++) temp[c] = M[c * n + c] * M[k * n + c];
            double dot = M[k * n + 0] * temp[0];
            for (int c = 1; c < k; c++) dot = dot + M[k * n + c] * temp[c];
            M[k * n + k] = M[k * n + k] - dot;
            for (int r = 0; r < rs; r++) {
                const int row = k + 1 + r;
                double d2 = M[row * n + 0] * temp[0];
                for (int c = 1; c < k; c++) d2 = d2 + M[row * n + c] * temp[c];
                M[row * n + k] = M[row * n + k] - d2;
            }
        }
        if (rs > 0 && std::fabs(M[k * n + k]) > cutoff)
            for (int r = 0; r < rs; r++) M[(k + 1 + r) * n + k] = M[(k + 1 + r) * n + k] / M[k * n + k];
    }
    if (sign != 1) return false;   // isPositive()
    double d[6];
    for (int i = 0; i < n; i++) d[i] = b[i];
    for (int k = 0; k < n; k++) { const double t = d[k]; d[k] = d[tr[k]]; d[tr[k]] = t; }   // P b
    for (int i = 0; i < n; i++)                                                             // L^-1, unit diagonal, column sweeps
        for (int r = i + 1; r < n; r++) d[r] = d[r] - d[i] * M[r * n + i];
    double maxAbs = std::fabs(M[0]);
    for (int i = 1; i < n; i++) { const double a = std::fabs(M[i * n + i]); if (a > maxAbs) maxAbs = a; }
    const double ta = maxAbs * DBL_EPSILON, tb = 1.0 / DBL_MAX;
    const double tol = (ta < tb) ? tb : ta;
    for (int i = 0; i < n; i++) {
        if (std::fabs(M[i * n + i]) > tol) d[i] = d[i] / M[i * n + i];
        else d[i] = 0.0;
    }
    for (int i = n - 2; i >= 0; i--) {                                                      // L^-T: a dot per row, then one subtraction
        double dot = M[(i + 1) * n + i] * d[i + 1];
        for (int c = i + 2; c < n; c++) dot = dot + M[c * n + i] * d[c];
        d[i] = d[i] - dot;
    }
    for (int k = n - 1; k >= 0; k--) { const double t = d[k]; d[k] = d[tr[k]]; d[tr[k]] = t; }   // P^T
    for (int i = 0; i < n; i++) x[i] = d[i];
    return true;
}

// ------------------------------------------------------------------ the function
struct Frame { float Tcw[16]; float K[4]; };   // mTcw; fx fy cx cy
struct Result {
    float Tcw[16];
    int32_t nInitial, nGood, rounds;
    int32_t iterations[4], trials[4];
    double lambda[4], chi2[4];
};
struct Diag {
    int32_t lastTrialRejected[4];   // the round's last Levenberg trial was rejected: its level-0 edges are classified stale
    double* classChi2;              // when given: 4 * n doubles, the chi2 every edge was classified with in every round
};

// A NaN leaves in ONE pattern, x86's default NaN (sign set, quiet bit, no payload): which of two NaN operands an operation hands on,
// and the sign a NaN is born with, are the machine's and not part of the definition.
inline double nanCanonical(double v)
{
    if (v == v) return v;
    const uint64_t bits = 0xFFF8000000000000ull;
    std::memcpy(&v, &bits, 8);
    return v;
}
inline float nanCanonical(float v)
{
    if (v == v) return v;
    const uint32_t bits = 0xFFC00000u;
    std::memcpy(&v, &bits, 4);
    return v;
}

// the index of entry (i, j), i >= j, among the 21 of the lower triangle
inline int lowerIndex(int i, int j) { return i * (i + 1) / 2 + j; }

template <class Mode> struct PoseOptimizer {
    Cam K;
    std::vector<EdgeD> edges;
    std::vector<uint8_t> level;     // setLevel: 1 leaves the edge out of the next round
    bool robust;                    // the Huber kernel is still on the edges
    double delta, dsqr;
    // OptimizationAlgorithmLevenberg's and the block solver's members that live across optimize() calls
    double lambda, growth, x[6];
    int flatSteps;
    SE3 est, errPose;               // the estimate; the pose the active edges' _error was last computed at

    // computeActiveErrors + activeRobustChi2 (g2o:core/sparse_optimizer.cpp:61-76, 100-114) at pose p
    double activeRobustChi2(const SE3& p)
    {
        EdgeSums<Mode, 1> sum;
        for (size_t e = 0; e < edges.size(); e++) {
            if (level[e]) continue;
            double err[2], rho[3];
            computeError(p, K, edges[e], err);
            const double c = chi2Of(err, edges[e].Om);
            if (robust) { huber(c, delta, dsqr, rho); sum.add((int)e, 0, rho[0]); }
            else sum.add((int)e, 0, c);
        }
        errPose = p;
        double out[1];
        sum.total(out);
        return out[0];
    }

    // buildSystem (g2o:core/block_solver.hpp:506-565): linearizeOplus + constructQuadraticForm (g2o:core/base_unary_edge.hpp:43-72)
    // of every active edge, _error being what computeActiveErrors left (the estimate's)
    void buildSystem(double H[21], double b[6])
    {
        EdgeSums<Mode, 21> sh;
        EdgeSums<Mode, 6> sb;
        for (size_t e = 0; e < edges.size(); e++) {
            if (level[e]) continue;
            const EdgeD& E = edges[e];
            double err[2], A[12], T[12];
            computeError(est, K, E, err);
            linearizeOplus(est, K, E, A);
            double W[4] = {E.Om[0], E.Om[1], E.Om[2], E.Om[3]};
            if (robust) {
                double rho[3];
                huber(chi2Of(err, E.Om), delta, dsqr, rho);
                // robustInformation = rho[1] * Omega, no second-order term
                for (int k = 0; k < 4; k++) W[k] = rho[1] * E.Om[k];
                // b -= rho[1] * A^T * omega * _error, left to right
                for (int i = 0; i < 6; i++) {
                    const double t0 = (rho[1] * A[i]) * E.Om[0] + (rho[1] * A[6 + i]) * E.Om[2];
                    const double t1 = (rho[1] * A[i]) * E.Om[1] + (rho[1] * A[6 + i]) * E.Om[3];
                    sb.sub((int)e, i, t0 * err[0] + t1 * err[1]);
                }
            } else {
                for (int i = 0; i < 6; i++) {
                    const double t0 = A[i] * E.Om[0] + A[6 + i] * E.Om[2];
                    const double t1 = A[i] * E.Om[1] + A[6 + i] * E.Om[3];
                    sb.sub((int)e, i, t0 * err[0] + t1 * err[1]);
                }
            }
            for (int i = 0; i < 6; i++) { T[i * 2] = A[i] * W[0] + A[6 + i] * W[2]; T[i * 2 + 1] = A[i] * W[1] + A[6 + i] * W[3]; }
            for (int i = 0; i < 6; i++)
                for (int j = 0; j <= i; j++) sh.add((int)e, lowerIndex(i, j), T[i * 2] * A[j] + T[i * 2 + 1] * A[6 + j]);
        }
        sh.total(H);
        sb.total(b);
    }

    // OptimizationAlgorithmLevenberg::solve (g2o:core/optimization_algorithm_levenberg.cpp:61-164); false: Terminate
    bool solve(int iteration, int& trials, double& chiOut, bool& lastRejected)
    {
        double chiNow = activeRobustChi2(est);
        double chiTrial = chiNow;
        const double chiStart = chiNow;
        double H[21], b[6];
        buildSystem(H, b);
        if (iteration == 0) {
            // computeLambdaInit (:166-180), tau 1e-5; std::max(a, b) is (a < b) ? b : a
            double diagMax = 0.;
            for (int j = 0; j < 6; j++) { const double a = std::fabs(H[lowerIndex(j, j)]); diagMax = (a < diagMax) ? diagMax : a; }
            lambda = 1e-5 * diagMax;
            growth = 2;
            flatSteps = 0;
        }
        double gain = 0;
        int nTried = 0;
        do {
            const SE3 backup = est;   // push()
            double M[36];
            for (int i = 0; i < 6; i++) for (int j = 0; j <= i; j++) { M[i * 6 + j] = H[lowerIndex(i, j)]; M[j * 6 + i] = H[lowerIndex(i, j)]; }
            for (int i = 0; i < 6; i++) M[i * 6 + i] = M[i * 6 + i] + lambda;   // setLambda(_currentLambda, true)
            // LinearSolverDense::solve (g2o:solvers/linear_solver_dense.h:65-113): x is written only when isPositive(); otherwise
            // it keeps what the last solve left.  Before any solve it is ZERO here: a chosen reading -- g2o zeroes _x only in a
            // debug build (g2o:core/solver.cpp:56 sits under #ifndef NDEBUG), a release build leaves it uninitialised.  It matters
            // only when the very first factorisation of a call is not positive.
            const bool solved = ldltSolve6(M, b, x);
            est = se3Mul(se3Exp<Mode>(x), est);   // oplusImpl: exp(dx) * estimate (g2o:types/types_six_dof_expmap.h:73-76)
            chiTrial = activeRobustChi2(est);
            if (!solved) chiTrial = DBL_MAX;
            gain = (chiNow - chiTrial);
            double scale = 0.;   // computeScale (:182-189)
            for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            gain /= scale;
            if (gain > 0 && (chiTrial >= -DBL_MAX && chiTrial <= DBL_MAX)) {
                const double t = 2 * gain - 1;
                double keep = 1. - Arith<Mode>::cube(t);
                // std::min(keep, 2/3) then std::max(1/3, keep), as their ternaries
                keep = ((2. / 3.) < keep) ? (2. / 3.) : keep;
                const double shrink = ((1. / 3.) < keep) ? keep : (1. / 3.);
                lambda *= shrink;
                growth = 2;
                chiNow = chiTrial;
                lastRejected = false;
            } else {
                lambda *= growth;
                growth *= 2;
                // STALE ERRORS: pop() restores the estimate, not the edges' _error -- errPose stays the rejected pose
                est = backup;
                lastRejected = true;
            }
            nTried++;
        } while (gain < 0 && nTried < 10);
        trials += nTried;
        chiOut = chiNow;
        if (nTried == 10 || gain == 0) return false;
        if ((chiStart - chiNow) * 1e3 < chiStart) flatSteps++;
        else flatSteps = 0;
        if (flatSteps >= 3) return false;
        return true;
    }
};

// ref:261-473.  edges in vpEdgesMono's order; outlier gets one byte per edge (mvbOutlier at the edge's feature)
template <class Mode> inline void poseOptimization(const Frame& F, const Edge* edges, int n, Result& res, uint8_t* outlier, Diag* diag)
{
    std::memset(&res, 0, sizeof res);
    std::memcpy(res.Tcw, F.Tcw, sizeof res.Tcw);
    res.nInitial = n;
    for (int e = 0; e < n; e++) outlier[e] = 0;   // ref:311
    if (diag) for (int r = 0; r < 4; r++) diag->lastTrialRejected[r] = 0;
    if (n < 3) return;   // ref:386: returns 0, the pose as it was
    PoseOptimizer<Mode> o;
    o.K.fx = (double)F.K[0]; o.K.fy = (double)F.K[1]; o.K.cx = (double)F.K[2]; o.K.cy = (double)F.K[3];
    o.edges.resize((size_t)n);
    for (int e = 0; e < n; e++) o.edges[(size_t)e] = widen(edges[e]);
    o.level.assign((size_t)n, 0);
    o.robust = true;
    const float deltaMono = std::sqrt(5.991);   // ref:295: a float
    o.delta = (double)deltaMono;
    o.dsqr = o.delta * o.delta;
    o.lambda = -1.; o.growth = 2.; o.flatSteps = 0;
    for (int j = 0; j < 6; j++) o.x[j] = 0.0;
    int nBad = 0;
    for (int it = 0; it < 4; it++) {
        // POSE WRITTEN BACK ONLY AT THE END: mTcw is read again here (ref:399) and SetPose comes at ref:470, so every round
        // starts from the caller's pose
        o.est = toSE3Quat(F.Tcw);
        o.errPose = o.est;
        int nActive = 0;
        for (int e = 0; e < n; e++) nActive += o.level[(size_t)e] == 0;
        bool lastRejected = false;
        if (nActive > 0) {   // (no edge at level 0: initializeOptimization finds no vertex and optimize() returns at once)
            for (int i = 0; i < 10; i++) {
                res.iterations[it]++;
                if (!o.solve(i, res.trials[it], res.chi2[it], lastRejected)) break;
            }
            res.lambda[it] = o.lambda;
        }
        if (diag) diag->lastTrialRejected[it] = lastRejected;
        nBad = 0;
        for (int e = 0; e < n; e++) {
            // STALE ERRORS: a level-0 edge keeps the _error of the last computeActiveErrors, which is the last TRIAL's pose even
            // when that trial was rejected; only an edge already marked an outlier gets a fresh computeError() (ref:410-413)
            double err[2];
            computeError(outlier[e] ? o.est : o.errPose, o.K, o.edges[(size_t)e], err);
            const float chi2 = (float)chi2Of(err, o.edges[(size_t)e].Om);
            if (diag && diag->classChi2) diag->classChi2[(size_t)it * n + e] = chi2Of(err, o.edges[(size_t)e].Om);
            if (chi2 > 5.991f) { outlier[e] = 1; o.level[(size_t)e] = 1; nBad++; }
            else { outlier[e] = 0; o.level[(size_t)e] = 0; }
        }
        if (it == 2) o.robust = false;   // ref:429-430
        res.rounds = it + 1;
        if (n < 10) break;   // ref:462: the edge count never changes
    }
    toCvMat(o.est, res.Tcw);
    for (int k = 0; k < 16; k++) res.Tcw[k] = nanCanonical(res.Tcw[k]);
    for (int r = 0; r < 4; r++) { res.lambda[r] = nanCanonical(res.lambda[r]); res.chi2[r] = nanCanonical(res.chi2[r]); }
    res.nGood = n - nBad;
}

}  // namespace poseopt_ref
