// sim3opt_ref.hpp -- an independent restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1348-1543; `ref:LINE` cites it),
// monocular, for the tests and for tools/sim3opt_bench.py: the 7-dof Levenberg that LoopClosing::ComputeSim3 and
// MultiMapper::Run run on every loop / merge candidate, on the host, in plain C++11 with the standard library alone.  It shares
// no header with the library; from poseopt_ref.hpp it takes the pieces that are the same (definedSinCos, quatFromMatrix, quatMul,
// quatRotate, huber, chi2Of, EdgeSums, lowerIndex, nanCanonical).  The g2o pieces are restated here (`g2o:FILE:LINE` cites
// Thirdparty/g2o/g2o/FILE); Eigen is cited by function, as of Eigen 3.2.0: no Eigen is installed, so parity against g2o itself
// is UNPINNED, as poseopt_ref.hpp says of itself.  Build with -ffp-contract=off.
//
// Two arithmetic modes, as there:
//   Serial   sums the edges' H, b and chi2 in edge order and calls libm's sin, cos and exp.
//   Defined  what the device is held to bit for bit.  To §8o's definition it adds only:
//     THE EDGE INDEX.  Correspondence c (its position in the list the caller passes) owns edge 2c (e12) and edge 2c + 1 (e21), the
//       order of addEdge (ref:1458, 1476); a removed pair keeps its indices and is skipped.  Edge e goes to partial e % 64 of the
//       same tree, over the 28 entries of H's lower triangle, the 7 of b and the robust chi2.  b is built as p = p + term.
//     exp is definedExp below: + - * /, comparisons, integer conversion and 2^k built from its exponent bits.
//
// Readings chosen: every inner product is sequential in index order; the quaternion product is the generic one; the solver's x
// is zero before any solve and lives across the two optimize() calls (poseopt_ref.hpp says why this is a reading).
#pragma once

#include "poseopt_ref.hpp"

namespace sim3opt_ref {

using poseopt_ref::Defined;
using poseopt_ref::Serial;

// ------------------------------------------------------------------ the Defined exp
// 2^k for k in [-1022, 1023], from its exponent bits
inline double pow2Bits(int k)
{
    const uint64_t bits = (uint64_t)(k + 1023) << 52;
    double v;
    std::memcpy(&v, &bits, 8);
    return v;
}

// k = (int64)(x / ln2 +- 0.5), r = (x - k L1) - k L2 with ln 2 in two parts (L1: 21 significant bits, so k L1 is exact for
// |k| < 2^11), e^r = 1 + (r + r^2 q(r)) with q the Taylor polynomial to r^11 (e^r's to r^13: the next term is below 2^-57 on
// |r| <= ln2 / 2) in Horner form, then times 2^k (in two steps where 2^k itself is no normal number).  NaN -> NaN, above
// 709.782712893384 -> +inf, below -745.1332191019412 -> 0.
inline double definedExp(double x)
{
    if (!(x == x)) return x + x;
    if (x > 709.782712893384) return pow2Bits(1023) * 2.0;
    if (x < -745.1332191019412) return 0.0;
    const double kLn2 = 0.6931471805599453, L1 = 6.93147180369123816490e-01, L2 = 1.90821492927058770002e-10;
    const int64_t k = (int64_t)(x / kLn2 + (x < 0 ? -0.5 : 0.5));
    const double kd = (double)k;
    const double r = (x - kd * L1) - kd * L2;
    double q = 1.0 / 6227020800.0;       // 1/13!
    q = q * r + 1.0 / 479001600.0;       // 1/12!
    q = q * r + 1.0 / 39916800.0;        // 1/11!
    q = q * r + 1.0 / 3628800.0;         // 1/10!
    q = q * r + 1.0 / 362880.0;          // 1/9!
    q = q * r + 1.0 / 40320.0;           // 1/8!
    q = q * r + 1.0 / 5040.0;            // 1/7!
    q = q * r + 1.0 / 720.0;             // 1/6!
    q = q * r + 1.0 / 120.0;             // 1/5!
    q = q * r + 1.0 / 24.0;              // 1/4!
    q = q * r + 1.0 / 6.0;               // 1/3!
    q = q * r + 0.5;                     // 1/2!
    const double e = 1.0 + (r + (r * r) * q);
    if (k > 1023) return (e * pow2Bits(1023)) * 2.0;
    if (k < -1022) return (e * pow2Bits((int)k + 1000)) * pow2Bits(-1000);
    return e * pow2Bits((int)k);
}

template <class Mode> struct Exp;
template <> struct Exp<Serial> { static double exp(double x) { return std::exp(x); } };
template <> struct Exp<Defined> { static double exp(double x) { return definedExp(x); } };

// ------------------------------------------------------------------ g2o::Sim3 (g2o:types/sim3.h)
struct Sim3 { double q[4]; double t[3]; double s; };   // q: x y z w, Eigen's coefficient order

// Sim3(const Vector7d& update) (g2o:types/sim3.h:70-142): update = (omega, upsilon, sigma), all four branches
template <class Mode> inline Sim3 sim3Exp(const double u[7])
{
    const double sigma = u[6];
    const double theta = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double Om[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    Sim3 o;
    o.s = Exp<Mode>::exp(sigma);
    double Om2[9], R[9];
    poseopt_ref::mat3Mul(Om, Om, Om2);
    const double eps = 0.00001;
    double A, B, C;
    const bool smallTheta = theta < eps;
    double sn = 0.0, cs = 0.0;
    if (!smallTheta) poseopt_ref::Arith<Mode>::sincos(theta, sn, cs);
    if (smallTheta) {
        for (int k = 0; k < 9; k++) R[k] = (I[k] + Om[k]) + Om2[k];   // un-normalised: Quaterniond(R) of it below
    } else {
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int k = 0; k < 9; k++) R[k] = (I[k] + a * Om[k]) + b * Om2[k];
    }
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (smallTheta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cs) / (theta2);
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (o.s - 1) / sigma;
        if (smallTheta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * o.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * o.s) / (sigma2 * sigma);
        } else {
            const double a = o.s * sn, b = o.s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    poseopt_ref::quatFromMatrix(R, o.q);
    double W[9];
    for (int k = 0; k < 9; k++) W[k] = (A * Om[k] + B * Om2[k]) + C * I[k];
    for (int i = 0; i < 3; i++) o.t[i] = (W[i * 3] * u[3] + W[i * 3 + 1] * u[4]) + W[i * 3 + 2] * u[5];
    return o;
}

// Sim3::map (:144-146): s * (r * xyz) + t
inline void sim3Map(const Sim3& S, const double p[3], double o[3])
{
    double r[3];
    poseopt_ref::quatRotate(S.q, p, r);
    for (int i = 0; i < 3; i++) o[i] = S.s * r[i] + S.t[i];
}

// Sim3::operator* (:266-272): NO normalisation of the quaternion, unlike SE3Quat
inline Sim3 sim3Mul(const Sim3& a, const Sim3& b)
{
    Sim3 o;
    poseopt_ref::quatMul(a.q, b.q, o.q);
    double r[3];
    poseopt_ref::quatRotate(a.q, b.t, r);
    for (int i = 0; i < 3; i++) o.t[i] = a.s * r[i] + a.t[i];
    o.s = a.s * b.s;
    return o;
}

// Sim3::inverse (:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
inline Sim3 sim3Inverse(const Sim3& S)
{
    Sim3 o;
    o.q[0] = -S.q[0]; o.q[1] = -S.q[1]; o.q[2] = -S.q[2]; o.q[3] = S.q[3];
    const double f = -1. / S.s;
    const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    poseopt_ref::quatRotate(o.q, v, o.t);
    o.s = 1. / S.s;
    return o;
}

// VertexSim3Expmap::oplusImpl (g2o:types/types_seven_dof_expmap.h:60-69): update[6] = 0 under _fix_scale -- WRITTEN INTO THE
// CALLER'S ARRAY, which for a Levenberg step is the solver's x -- then Sim3(update) * estimate
template <class Mode> inline Sim3 oplus(const Sim3& est, double u[7], bool fixScale)
{
    if (fixScale) u[6] = 0;
    return sim3Mul(sim3Exp<Mode>(u), est);
}

// ------------------------------------------------------------------ the inputs, after the pointer chasing of ref:1401-1440
struct Problem {
    double q[4], t[3], s;                 // g2oS12
    float R1w[9], t1w[3], K1[4];          // pKF1: GetRotation, GetTranslation, fx fy cx cy
    float R2w[9], t2w[3], K2[4];          // pKF2
    float th2;
    int32_t fixScale;
};
struct Corr {
    float obs1[2]; float invSigma2_1;     // mvKeysUn[i].pt of pKF1, mvInvLevelSigma2[octave]
    float obs2[2]; float invSigma2_2;     // mvKeysUn[i2].pt of pKF2
    float X1w[3], X2w[3];                 // GetWorldPos() of pMP1, pMP2
};
struct Result {
    double q[4], t[3], s;
    int32_t written, nCorr, nBad, nIn;
    int32_t iterations[2], trials[2];
    double lambda[2], chi2[2];
};
struct Diag {
    int32_t lastTrialRejected[2];   // the pass's last Levenberg trial was rejected: the check that follows reads stale errors
    double* classChi2;              // when given: 2 passes x 2n doubles, the chi2 every edge was checked with (NaN where none)
};

// cv::Mat R * X + t in CV_32F (ref:1421, 1429): gemm's small branch with a C -- the float dot product left to right, then
// (float)((double)dot + (double)t)
inline void cameraPoint(const float R[9], const float t[3], const float X[3], double o[3])
{
    for (int r = 0; r < 3; r++) {
        const float d = R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2];
        o[r] = (double)(float)((double)d * 1.0 + (double)t[r] * 1.0);
    }
}

struct EdgeD { double obs[2], Om[4], P[3]; int inverse; };   // inverse: EdgeInverseSim3ProjectXYZ, camera 2

// ------------------------------------------------------------------ Eigen::LDLT<MatrixXd, Lower> (3.2.0) at size N: poseopt_ref's
// ldltSolve6 with the size a template parameter (same steps, same order)
template <int N> inline bool ldltSolveN(double* M, const double* b, double* x)
{
    const int n = N;
    int tr[N];
    double temp[N];
    double cutoff = 0.0;
    int sign = 0;
    for (int k = 0; k < n; k++) {
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
            for (int c = 0; c < k; c++) { const double t = M[k * n + c]; M[k * n + c] = M[big * n + c]; M[big * n + c] = t; }
            for (int row = big + 1; row < n; row++) { const double t = M[row * n + k]; M[row * n + k] = M[row * n + big]; M[row * n + big] = t; }
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
    if (sign != 1) return false;
    double d[N];
    for (int i = 0; i < n; i++) d[i] = b[i];
    for (int k = 0; k < n; k++) { const double t = d[k]; d[k] = d[tr[k]]; d[tr[k]] = t; }
    for (int i = 0; i < n; i++)
        for (int r = i + 1; r < n; r++) d[r] = d[r] - d[i] * M[r * n + i];
    double maxAbs = std::fabs(M[0]);
    for (int i = 1; i < n; i++) { const double a = std::fabs(M[i * n + i]); if (a > maxAbs) maxAbs = a; }
    const double ta = maxAbs * DBL_EPSILON, tb = 1.0 / DBL_MAX;
    const double tol = (ta < tb) ? tb : ta;
    for (int i = 0; i < n; i++) {
        if (std::fabs(M[i * n + i]) > tol) d[i] = d[i] / M[i * n + i];
        else d[i] = 0.0;
    }
    for (int i = n - 2; i >= 0; i--) {
        double dot = M[(i + 1) * n + i] * d[i + 1];
        for (int c = i + 2; c < n; c++) dot = dot + M[c * n + i] * d[c];
        d[i] = d[i] - dot;
    }
    for (int k = n - 1; k >= 0; k--) { const double t = d[k]; d[k] = d[tr[k]]; d[tr[k]] = t; }
    for (int i = 0; i < n; i++) x[i] = d[i];
    return true;
}

// ------------------------------------------------------------------ the optimiser
template <class Mode> struct Sim3Optimizer {
    poseopt_ref::Cam K[2];            // cam_map1, cam_map2 (g2o:types/types_seven_dof_expmap.h:74-88)
    std::vector<EdgeD> edges;         // 2c: e12 of correspondence c, 2c + 1: e21
    std::vector<uint8_t> removed;     // per correspondence: removeEdge of both (ref:1500-1501)
    bool fixScale, cached;
    double delta, dsqr;
    double lambda, growth, x[7];
    int flatSteps;
    Sim3 est, errS;                   // the estimate; the estimate the active edges' _error was last computed at

    // computeError of either edge type at estimate S (g2o:types/types_seven_dof_expmap.h:138-145, 160-167); Sinv: S.inverse()
    // when the caller has it, else it is taken here, per edge, as g2o takes it
    void edgeError(const EdgeD& E, const Sim3& S, const Sim3* Sinv, double err[2]) const
    {
        double p[3];
        if (E.inverse) {
            if (Sinv) sim3Map(*Sinv, E.P, p);
            else { const Sim3 inv = sim3Inverse(S); sim3Map(inv, E.P, p); }
        } else sim3Map(S, E.P, p);
        const poseopt_ref::Cam& C = K[E.inverse];
        const double px = p[0] / p[2], py = p[1] / p[2];   // project (g2o:types/se3_ops.hpp)
        err[0] = E.obs[0] - (px * C.fx + C.cx);
        err[1] = E.obs[1] - (py * C.fy + C.cy);
    }

    // computeActiveErrors + activeRobustChi2 at S
    double activeRobustChi2(const Sim3& S)
    {
        poseopt_ref::EdgeSums<Mode, 1> sum;
        for (size_t e = 0; e < edges.size(); e++) {
            if (removed[e / 2]) continue;
            double err[2], rho[3];
            edgeError(edges[e], S, nullptr, err);
            poseopt_ref::huber(poseopt_ref::chi2Of(err, edges[e].Om), delta, dsqr, rho);
            sum.add((int)e, 0, rho[0]);
        }
        errS = S;
        double out[1];
        sum.total(out);
        return out[0];
    }

    // buildSystem: BaseBinaryEdge::linearizeOplus, numeric (g2o:core/base_binary_edge.hpp:131-205; only the Sim3 vertex is free), and
    // constructQuadraticForm's robust branch for the `to` vertex (:91-113) of every active edge.  _error is the estimate's: the
    // numeric pass restores it (:150, :200)
    void buildSystem(double H[28], double b[7])
    {
        poseopt_ref::EdgeSums<Mode, 28> sh;
        poseopt_ref::EdgeSums<Mode, 7> sb;
        const double dlt = 1e-9;
        const double scalar = 1.0 / (2 * dlt);
        // the cached evaluation: oplus is a pure function of the estimate and d, so the 14 perturbed estimates and their inverses
        // are the same for every edge
        Sim3 pert[7][2], pinv[7][2], estInv = sim3Inverse(est);
        if (cached)
            for (int d = 0; d < 7; d++)
                for (int sgn = 0; sgn < 2; sgn++) {
                    double add[7] = {0, 0, 0, 0, 0, 0, 0};
                    add[d] = sgn ? -dlt : dlt;
                    pert[d][sgn] = oplus<Mode>(est, add, fixScale);
                    pinv[d][sgn] = sim3Inverse(pert[d][sgn]);
                }
        for (size_t e = 0; e < edges.size(); e++) {
            if (removed[e / 2]) continue;
            const EdgeD& E = edges[e];
            double err[2], B[2][7];
            edgeError(E, est, cached ? &estInv : nullptr, err);
            double add[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int d = 0; d < 7; d++) {
                double ep[2], em[2];
                if (cached) {
                    edgeError(E, pert[d][0], &pinv[d][0], ep);
                    edgeError(E, pert[d][1], &pinv[d][1], em);
                } else {
                    add[d] = dlt;                                    // push, oplus, computeError, pop
                    const Sim3 sp = oplus<Mode>(est, add, fixScale);
                    edgeError(E, sp, nullptr, ep);
                    add[d] = -dlt;                                   // push, oplus, computeError, pop
                    const Sim3 sm = oplus<Mode>(est, add, fixScale);
                    edgeError(E, sm, nullptr, em);
                    add[d] = 0.0;
                }
                B[0][d] = scalar * (ep[0] - em[0]);
                B[1][d] = scalar * (ep[1] - em[1]);
            }
            double rho[3];
            poseopt_ref::huber(poseopt_ref::chi2Of(err, E.Om), delta, dsqr, rho);
            double r0 = -(E.Om[0] * err[0] + E.Om[1] * err[1]), r1 = -(E.Om[2] * err[0] + E.Om[3] * err[1]);   // omega_r = -omega * _error
            r0 = r0 * rho[1]; r1 = r1 * rho[1];
            const double W[4] = {rho[1] * E.Om[0], rho[1] * E.Om[1], rho[1] * E.Om[2], rho[1] * E.Om[3]};          // robustInformation
            for (int i = 0; i < 7; i++) sb.add((int)e, i, B[0][i] * r0 + B[1][i] * r1);                            // b += B^T omega_r
            for (int i = 0; i < 7; i++) {                                                                          // H += (B^T W) B
                const double t0 = B[0][i] * W[0] + B[1][i] * W[2], t1 = B[0][i] * W[1] + B[1][i] * W[3];
                for (int j = 0; j <= i; j++) sh.add((int)e, poseopt_ref::lowerIndex(i, j), t0 * B[0][j] + t1 * B[1][j]);
            }
        }
        sh.total(H);
        sb.total(b);
    }

    // OptimizationAlgorithmLevenberg::solve (g2o:core/optimization_algorithm_levenberg.cpp:61-164) on the one 7 x 7 block
    bool solve(int iteration, int& trials, double& chiOut, bool& lastRejected)
    {
        double chiNow = activeRobustChi2(est);
        double chiTrial = chiNow;
        const double chiStart = chiNow;
        double H[28], b[7];
        buildSystem(H, b);
        if (iteration == 0) {
            double diagMax = 0.;
            for (int j = 0; j < 7; j++) { const double a = std::fabs(H[poseopt_ref::lowerIndex(j, j)]); diagMax = (a < diagMax) ? diagMax : a; }
            lambda = 1e-5 * diagMax;
            growth = 2;
            flatSteps = 0;
        }
        double gain = 0;
        int nTried = 0;
        do {
            const Sim3 backup = est;
            double M[49];
            for (int i = 0; i < 7; i++) for (int j = 0; j <= i; j++) { M[i * 7 + j] = H[poseopt_ref::lowerIndex(i, j)]; M[j * 7 + i] = M[i * 7 + j]; }
            for (int i = 0; i < 7; i++) M[i * 7 + i] = M[i * 7 + i] + lambda;
            const bool solved = ldltSolveN<7>(M, b, x);
            est = oplus<Mode>(est, x, fixScale);   // (x[6] becomes 0 under fixScale, for computeScale below as well)
            chiTrial = activeRobustChi2(est);
            if (!solved) chiTrial = DBL_MAX;
            gain = (chiNow - chiTrial);
            double scale = 0.;
            for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            gain /= scale;
            if (gain > 0 && (chiTrial >= -DBL_MAX && chiTrial <= DBL_MAX)) {
                const double t = 2 * gain - 1;
                double keep = 1. - poseopt_ref::Arith<Mode>::cube(t);
                keep = ((2. / 3.) < keep) ? (2. / 3.) : keep;
                const double shrink = ((1. / 3.) < keep) ? keep : (1. / 3.);
                lambda *= shrink;
                growth = 2;
                chiNow = chiTrial;
                lastRejected = false;
            } else {
                lambda *= growth;
                growth *= 2;
                est = backup;   // STALE ERRORS: pop() restores the estimate, not the edges' _error
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

// ref:1348-1543.  corrs in ascending i (vnIndexEdge's order).  removed: one byte per correspondence, 0 kept, 1 nulled by the
// first check, 2 by the second.  cached: the 14 perturbed estimates once per linearisation instead of per edge
template <class Mode> inline void optimizeSim3(const Problem& P, const Corr* corrs, int n, Result& res, uint8_t* removed, Diag* diag, bool cached = false)
{
    std::memset(&res, 0, sizeof res);
    for (int k = 0; k < 4; k++) res.q[k] = P.q[k];
    for (int k = 0; k < 3; k++) res.t[k] = P.t[k];
    res.s = P.s;
    res.nCorr = n;
    for (int c = 0; c < n; c++) removed[c] = 0;
    if (diag) { diag->lastTrialRejected[0] = diag->lastTrialRejected[1] = 0; }
    Sim3Optimizer<Mode> o;
    const float* Kf[2] = {P.K1, P.K2};
    for (int k = 0; k < 2; k++) { o.K[k].fx = (double)Kf[k][0]; o.K[k].fy = (double)Kf[k][1]; o.K[k].cx = (double)Kf[k][2]; o.K[k].cy = (double)Kf[k][3]; }
    o.edges.resize((size_t)2 * n);
    for (int c = 0; c < n; c++) {
        double P1c[3], P2c[3];
        cameraPoint(P.R1w, P.t1w, corrs[c].X1w, P1c);
        cameraPoint(P.R2w, P.t2w, corrs[c].X2w, P2c);
        EdgeD& a = o.edges[(size_t)2 * c];
        EdgeD& b = o.edges[(size_t)2 * c + 1];
        const double w1 = (double)corrs[c].invSigma2_1, w2 = (double)corrs[c].invSigma2_2;   // Identity * invSigma2 (ref:1453, 1471)
        a.obs[0] = (double)corrs[c].obs1[0]; a.obs[1] = (double)corrs[c].obs1[1];
        a.Om[0] = 1.0 * w1; a.Om[1] = 0.0 * w1; a.Om[2] = 0.0 * w1; a.Om[3] = 1.0 * w1;
        for (int k = 0; k < 3; k++) a.P[k] = P2c[k];     // x1 = S12 * X2
        a.inverse = 0;
        b.obs[0] = (double)corrs[c].obs2[0]; b.obs[1] = (double)corrs[c].obs2[1];
        b.Om[0] = 1.0 * w2; b.Om[1] = 0.0 * w2; b.Om[2] = 0.0 * w2; b.Om[3] = 1.0 * w2;
        for (int k = 0; k < 3; k++) b.P[k] = P1c[k];     // x2 = S21 * X1
        b.inverse = 1;
    }
    o.removed.assign((size_t)n, 0);
    o.fixScale = P.fixScale != 0;
    o.cached = cached;
    const float deltaHuber = std::sqrt(P.th2);   // ref:1398: the float square root of the float
    o.delta = (double)deltaHuber;
    o.dsqr = o.delta * o.delta;
    o.lambda = -1.; o.growth = 2.; o.flatSteps = 0;
    for (int j = 0; j < 7; j++) o.x[j] = 0.0;
    for (int k = 0; k < 4; k++) o.est.q[k] = P.q[k];
    for (int k = 0; k < 3; k++) o.est.t[k] = P.t[k];
    o.est.s = P.s;
    o.errS = o.est;
    const double th2 = (double)P.th2;
    int nBad = 0, nIn = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int maxIt = pass == 0 ? 5 : (nBad > 0 ? 10 : 5);   // ref:1485, 1508-1512
        bool lastRejected = false;
        if (n - nBad > 0) {   // (no edge: initializeOptimization finds no vertex and optimize() returns at once)
            for (int i = 0; i < maxIt; i++) {
                res.iterations[pass]++;
                if (!o.solve(i, res.trials[pass], res.chi2[pass], lastRejected)) break;
            }
            res.lambda[pass] = o.lambda;
        }
        if (diag) diag->lastTrialRejected[pass] = lastRejected;
        // the check (ref:1489-1506, 1523-1537): chi2() reads _error, which is the last TRIAL's, accepted or not
        for (int c = 0; c < n; c++) {
            if (diag && diag->classChi2) {
                const double nan = std::nan("");
                diag->classChi2[(size_t)pass * 2 * n + 2 * c] = nan;
                diag->classChi2[(size_t)pass * 2 * n + 2 * c + 1] = nan;
            }
            if (o.removed[(size_t)c]) continue;
            double e12[2], e21[2];
            o.edgeError(o.edges[(size_t)2 * c], o.errS, nullptr, e12);
            o.edgeError(o.edges[(size_t)2 * c + 1], o.errS, nullptr, e21);
            const double c12 = poseopt_ref::chi2Of(e12, o.edges[(size_t)2 * c].Om), c21 = poseopt_ref::chi2Of(e21, o.edges[(size_t)2 * c + 1].Om);
            if (diag && diag->classChi2) {
                diag->classChi2[(size_t)pass * 2 * n + 2 * c] = c12;
                diag->classChi2[(size_t)pass * 2 * n + 2 * c + 1] = c21;
            }
            if (c12 > th2 || c21 > th2) {
                removed[c] = (uint8_t)(pass + 1);
                if (pass == 0) { o.removed[(size_t)c] = 1; nBad++; }
            } else if (pass == 1) nIn++;
        }
        res.lambda[pass] = poseopt_ref::nanCanonical(res.lambda[pass]);
        res.chi2[pass] = poseopt_ref::nanCanonical(res.chi2[pass]);
        res.nBad = nBad;
        if (pass == 0 && n - nBad < 10) return;   // ref:1514: before g2oS12 is written, the nulled matches stay nulled
    }
    for (int k = 0; k < 4; k++) res.q[k] = poseopt_ref::nanCanonical(o.est.q[k]);
    for (int k = 0; k < 3; k++) res.t[k] = poseopt_ref::nanCanonical(o.est.t[k]);
    res.s = poseopt_ref::nanCanonical(o.est.s);
    res.written = 1;
    res.nIn = nIn;
}

}  // namespace sim3opt_ref
