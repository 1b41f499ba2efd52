// orbg_kernels.hip -- the g2o / Eigen pieces under the device optimizers (part of orbslamm_hip.hip): what PoseOptimization
// (orbo_kernels.hip) and OptimizeSim3 (orbz_kernels.hip, §8p) both run, stated once -- the defined sin / cos and
// exp, the NaN canonicalisers, Eigen's quaternion pieces and the so(3) exponential, the reprojection edge's record, Eigen's
// pivoted LDLT at size N, and ONE run of OptimizationAlgorithmLevenberg over a problem object that the calling kernel defines.
// Every line is held bit for bit to the restatements under tools/ (which share nothing with this file) through the kernels that
// use it: one IEEE operation per source operation (-ffp-contract=off), and an expression rewritten here is a changed result.
// The scalar pieces are __host__ __device__, so a program with no device can hold them to the restatements as well
// (tests/cpp/g2o_core_check.hip).  Needs nothing of the library: no orbm::, no orbx::, no ABI header.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace orbg {

constexpr int kLanes = 64;
constexpr int kIterations = 10, kTrials = 10;   // the most one optimize() call runs; the most trials one iteration takes

// ---- the sin / cos of §8o: + - * /, comparisons and integer conversion only
__host__ __device__ __forceinline__ double trunc_defined(double q)
{
    const double a = q < 0 ? -q : q;
    if (!(a < 4503599627370496.0)) return q;
    return (double)(long long)q;
}

__host__ __device__ inline __noinline__ void sincos_defined(double x, double& sOut, double& cOut)
{
    if (!(x - x == 0.0)) { sOut = x - x; cOut = x - x; return; }
    const bool neg = x < 0;
    double a = neg ? -x : x;
    for (int i = 0; i < 24; i++) {
        if (a < 1048576.0) break;
        a = a - trunc_defined(a / 6.283185307179586) * 6.283185307179586;
        if (a < 0) a = -a;
    }
    if (!(a < 1048576.0)) a = 0.0;
    const long long k = (long long)(a * 0.6366197723675814 + 0.5);
    const double kd = (double)k;
    const double r = ((a - kd * 1.5707963267341256) - kd * 6.077100506303966e-11) - kd * 2.0222662487959506e-21;
    const double z = r * r;
    double ps = 1.0 / 355687428096000.0;
    ps = ps * z - 1.0 / 1307674368000.0;
    ps = ps * z + 1.0 / 6227020800.0;
    ps = ps * z - 1.0 / 39916800.0;
    ps = ps * z + 1.0 / 362880.0;
    ps = ps * z - 1.0 / 5040.0;
    ps = ps * z + 1.0 / 120.0;
    ps = ps * z - 1.0 / 6.0;
    const double sr = r + r * (z * ps);
    double pc = 1.0 / 20922789888000.0;
    pc = pc * z - 1.0 / 87178291200.0;
    pc = pc * z + 1.0 / 479001600.0;
    pc = pc * z - 1.0 / 3628800.0;
    pc = pc * z + 1.0 / 40320.0;
    pc = pc * z - 1.0 / 720.0;
    pc = pc * z + 1.0 / 24.0;
    pc = pc * z - 0.5;
    const double cr = 1.0 + z * pc;
    const int quad = (int)(k & 3);
    const double ss = quad == 0 ? sr : quad == 1 ? cr : quad == 2 ? -sr : -cr;
    const double cc = quad == 0 ? cr : quad == 1 ? -sr : quad == 2 ? -cr : sr;
    sOut = neg ? -ss : ss;
    cOut = cc;
}

// ---- the exp of §8p: + - * /, comparisons, integer conversion, 2^k from its exponent bits
__host__ __device__ __forceinline__ double pow2_bits(int k) { return __builtin_bit_cast(double, (long long)(k + 1023) << 52); }

__host__ __device__ __forceinline__ double exp_defined(double x)
{
    if (!(x == x)) return x + x;
    if (x > 709.782712893384) return pow2_bits(1023) * 2.0;
    if (x < -745.1332191019412) return 0.0;
    const long long k = (long long)(x / 0.6931471805599453 + (x < 0 ? -0.5 : 0.5));
    const double kd = (double)k;
    const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    double q = 1.0 / 6227020800.0;
    q = q * r + 1.0 / 479001600.0;
    q = q * r + 1.0 / 39916800.0;
    q = q * r + 1.0 / 3628800.0;
    q = q * r + 1.0 / 362880.0;
    q = q * r + 1.0 / 40320.0;
    q = q * r + 1.0 / 5040.0;
    q = q * r + 1.0 / 720.0;
    q = q * r + 1.0 / 120.0;
    q = q * r + 1.0 / 24.0;
    q = q * r + 1.0 / 6.0;
    q = q * r + 0.5;
    const double e = 1.0 + (r + (r * r) * q);
    if (k > 1023) return (e * pow2_bits(1023)) * 2.0;
    if (k < -1022) return (e * pow2_bits((int)k + 1000)) * pow2_bits(-1000);
    return e * pow2_bits((int)k);
}

// a NaN among the outputs leaves as ONE pattern, x86's default NaN: a NaN born on the device is 0x7FF8..., on x86 0xFFF8..., and
// which operand's NaN an operation hands on is the machine's (the PnP kernels do the same)
__host__ __device__ __forceinline__ double nan_canon(double v) { return v != v ? __builtin_bit_cast(double, 0xFFF8000000000000ull) : v; }
__host__ __device__ __forceinline__ float nan_canon_f(double v) { const float f = (float)v; return f != f ? __builtin_bit_cast(float, 0xFFC00000u) : f; }

// ---- Eigen's quaternion pieces
struct Quat { double x, y, z, w; };

__host__ __device__ __forceinline__ void normalize_rotation(Quat& q)
{
    if (q.w < 0) { q.x = q.x * -1.0; q.y = q.y * -1.0; q.z = q.z * -1.0; q.w = q.w * -1.0; }
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    q.x = q.x / n; q.y = q.y / n; q.z = q.z / n; q.w = q.w / n;
}

// Quaterniond(R), R row-major; the largest-diagonal branch written out for i = 0, 1, 2
__host__ __device__ __forceinline__ Quat quat_of_matrix(const double (&R)[9])
{
    Quat q;
    double t = R[0] + R[4] + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (R[7] - R[5]) * t;
        q.y = (R[2] - R[6]) * t;
        q.z = (R[3] - R[1]) * t;
        return q;
    }
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i == 0 ? R[0] : R[4])) i = 2;
    if (i == 0) {          // j = 1, k = 2
        t = sqrt(R[0] - R[4] - R[8] + 1.0);
        q.x = 0.5 * t;
        t = 0.5 / t;
        q.w = (R[7] - R[5]) * t;
        q.y = (R[3] + R[1]) * t;
        q.z = (R[6] + R[2]) * t;
    } else if (i == 1) {   // j = 2, k = 0
        t = sqrt(R[4] - R[8] - R[0] + 1.0);
        q.y = 0.5 * t;
        t = 0.5 / t;
        q.w = (R[2] - R[6]) * t;
        q.z = (R[7] + R[5]) * t;
        q.x = (R[1] + R[3]) * t;
    } else {               // j = 0, k = 1
        t = sqrt(R[8] - R[0] - R[4] + 1.0);
        q.z = 0.5 * t;
        t = 0.5 / t;
        q.w = (R[3] - R[1]) * t;
        q.x = (R[2] + R[6]) * t;
        q.y = (R[5] + R[7]) * t;
    }
    return q;
}

// q * v (_transformVector), for a quaternion that need not be a unit one
__host__ __device__ __forceinline__ void rotate(const Quat& q, double vx, double vy, double vz, double& ox, double& oy, double& oz)
{
    double ux = q.y * vz - q.z * vy, uy = q.z * vx - q.x * vz, uz = q.x * vy - q.y * vx;
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    const double cx = q.y * uz - q.z * uy, cy = q.z * ux - q.x * uz, cz = q.x * uy - q.y * ux;
    ox = (vx + q.w * ux) + cx;
    oy = (vy + q.w * uy) + cy;
    oz = (vz + q.w * uz) + cz;
}

// a * b: Eigen's generic quat_product, no normalisation
__host__ __device__ __forceinline__ Quat quat_mul(const Quat& a, const Quat& b)
{
    Quat o;
    o.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    o.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    o.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    o.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return o;
}

// ---- the so(3) exponential both SE3Quat::exp and Sim3(update) open with: Omega = skew(omega) and Omega * Omega as full 3 x 3
// products (the zeros multiply: an infinity stays a NaN as it does there), R = I + a Omega + b Omega^2, and below the threshold
// R = I + Omega + Omega^2 with no factor (sn, cs and b are not taken then and stay zero)
struct So3Exp {
    double theta, sn, cs, b;
    bool small;
    double Om[9], Om2[9], R[9];
};

__host__ __device__ __forceinline__ So3Exp so3_exp(double w0, double w1, double w2)
{
    So3Exp e;
    e.theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double Om[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double Id[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int k = 0; k < 9; k++) e.Om[k] = Om[k];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) e.Om2[i * 3 + j] = (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
    e.small = e.theta < 0.00001;
    double sn = 0.0, cs = 0.0;   // (locals: a field handed to the call by reference would keep the whole record in memory)
    double a = 0.0;
    e.b = 0.0;
    if (!e.small) {
        sincos_defined(e.theta, sn, cs);
        a = sn / e.theta;
        e.b = (1.0 - cs) / (e.theta * e.theta);
    }
    e.sn = sn; e.cs = cs;
#pragma unroll
    for (int k = 0; k < 9; k++) e.R[k] = e.small ? ((Id[k] + Om[k]) + e.Om2[k]) : ((Id[k] + a * Om[k]) + e.b * e.Om2[k]);
    return e;
}

// ---- the reprojection edge: observation, information (Identity * invSigma2, its zeros kept), the point it projects
struct EdgeReg { double u, v, w00, w01, w10, w11, X, Y, Z; };
struct Cam { double fx, fy, cx, cy; };

// p: the point and invSigma2, o: the observation, as the gathers leave them per edge
__host__ __device__ __forceinline__ EdgeReg load_edge(const float4 p, const float2 o)
{
    EdgeReg E;
    E.u = (double)o.x; E.v = (double)o.y;
    const double w = (double)p.w;
    E.w00 = 1.0 * w; E.w01 = 0.0 * w; E.w10 = 0.0 * w; E.w11 = 1.0 * w;
    E.X = (double)p.x; E.Y = (double)p.y; E.Z = (double)p.z;
    return E;
}

// obs - cam_project(x, y, z)
__host__ __device__ __forceinline__ void pinhole_error(const Cam& K, const EdgeReg& E, double x, double y, double z, double& e0, double& e1)
{
    const double px = x / z, py = y / z;
    e0 = E.u - (px * K.fx + K.cx);
    e1 = E.v - (py * K.fy + K.cy);
}

__host__ __device__ __forceinline__ double edge_chi2(const EdgeReg& E, double e0, double e1)
{
    const double t0 = E.w00 * e0 + E.w01 * e1, t1 = E.w10 * e0 + E.w11 * e1;
    return e0 * t0 + e1 * t1;
}

// the Huber kernel on a chi2: the robust cost and the weight (its first derivative)
__host__ __device__ __forceinline__ void huber(double c, double delta, double delta2, double& cost, double& weight)
{
    if (c <= delta2) { cost = c; weight = 1.; }
    else {
        const double sq = sqrt(c);
        cost = 2 * sq * delta - delta2;
        weight = delta / sq;
    }
}

// THE SUMMATION TREE's close (§8o): the xor butterfly 32, 16, ..., 1 over the 64 lanes' partials; every lane holds the sum
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, kLanes);
    return v;
}

// ---- Eigen's unblocked LDLT with diagonal pivoting on the lower triangle of M (N x N, row-major), isPositive(), solve.
// Returns isPositive(); x is written only then.  tr and tmp: N words each of working space.
template <int N> __host__ __device__ __noinline__ bool ldlt_solve(double* M, const double* rhs, double* x, int* tr, double* tmp)
{
    constexpr int n = N;
    double cutoff = 0.0;
    int sign = 0;
    for (int k = 0; k < n; k++) {
        int big = k;
        double biggest = fabs(M[k * n + k]);
        for (int i = k + 1; i < n; i++) { const double v = fabs(M[i * n + i]); if (v > biggest) { biggest = v; big = i; } }
        if (k == 0) {
            cutoff = fabs(2.220446049250313e-16 * biggest);
            sign = M[big * n + big] > 0 ? 1 : -1;
        }
        if (biggest < cutoff) {
            for (int i = k; i < n; i++) tr[i] = i;
            break;
        }
        tr[k] = big;
        if (k != big) {
            for (int c = 0; c < k; c++) { const double t = M[k * n + c]; M[k * n + c] = M[big * n + c]; M[big * n + c] = t; }
            for (int r = big + 1; r < n; r++) { const double t = M[r * n + k]; M[r * n + k] = M[r * n + big]; M[r * n + big] = t; }
            const double t = M[k * n + k]; M[k * n + k] = M[big * n + big]; M[big * n + big] = t;
            for (int i = k + 1; i < big; i++) { const double s = M[i * n + k]; M[i * n + k] = M[big * n + i]; M[big * n + i] = s; }
        }
        if (k > 0) {
            for (int c = 0; c < k; c++) tmp[c] = M[c * n + c] * M[k * n + c];
            double dot = M[k * n] * tmp[0];
            for (int c = 1; c < k; c++) dot = dot + M[k * n + c] * tmp[c];
            M[k * n + k] = M[k * n + k] - dot;
            for (int r = k + 1; r < n; r++) {
                double d2 = M[r * n] * tmp[0];
                for (int c = 1; c < k; c++) d2 = d2 + M[r * n + c] * tmp[c];
                M[r * n + k] = M[r * n + k] - d2;
            }
        }
        if (k + 1 < n && fabs(M[k * n + k]) > cutoff)
            for (int r = k + 1; r < n; r++) M[r * n + k] = M[r * n + k] / M[k * n + k];
    }
    if (sign != 1) return false;
    for (int i = 0; i < n; i++) tmp[i] = rhs[i];
    for (int k = 0; k < n; k++) { const double t = tmp[k]; tmp[k] = tmp[tr[k]]; tmp[tr[k]] = t; }
    for (int i = 0; i < n; i++)
        for (int r = i + 1; r < n; r++) tmp[r] = tmp[r] - tmp[i] * M[r * n + i];
    double maxAbs = fabs(M[0]);
    for (int i = 1; i < n; i++) { const double v = fabs(M[i * n + i]); if (v > maxAbs) maxAbs = v; }
    const double ta = maxAbs * 2.220446049250313e-16, tb = 1.0 / 1.7976931348623157e308;
    const double tol = (ta < tb) ? tb : ta;
    for (int i = 0; i < n; i++) {
        if (fabs(M[i * n + i]) > tol) tmp[i] = tmp[i] / M[i * n + i];
        else tmp[i] = 0.0;
    }
    for (int i = n - 2; i >= 0; i--) {
        double dot = M[(i + 1) * n + i] * tmp[i + 1];
        for (int c = i + 2; c < n; c++) dot = dot + M[c * n + i] * tmp[c];
        tmp[i] = tmp[i] - dot;
    }
    for (int k = n - 1; k >= 0; k--) { const double t = tmp[k]; tmp[k] = tmp[tr[k]]; tmp[tr[k]] = t; }
    for (int i = 0; i < n; i++) x[i] = tmp[i];
    return true;
}

// ---- OptimizationAlgorithmLevenberg over one N-dof vertex, one wave a problem.  The estimate, lambda and the rest of the state
// are wave-uniform and computed redundantly by every lane; the pivoted LDLT and its solve run on lane 0 in LDS (the pivoting
// indexes at run time) and the step is read back by all.
// The LDS the solve works in: the kernel declares one __shared__
template <int N> struct LmShared { double M[N * N], B[N], X[N], Tmp[N]; int Tr[N], ok; };

// What lives across optimize() calls (a kernel's rounds or passes).  lambda, growth and flatSteps are reset at iteration 0 of
// every call.  x is the solver's: written only by a solve whose factorisation is positive, ZERO before any solve -- a chosen
// reading: g2o zeroes it in a debug build only and a release build leaves it uninitialised, which matters when a call's very
// first factorisation fails
template <int N> struct LmState {
    double lambda = -1., growth = 2.;
    int flatSteps = 0;
    double x[N] = {};
};

struct LmRun { int iterations, trials; double chi2; };

// One optimize(maxIt) call, maxIt <= kIterations.  The calling kernel's Problem supplies what differs:
//   est, err           the estimate, and the estimate the active edges' _error was last computed at
//   build(H, b, chi)   linearise at est: H's lower triangle row by row, b, the robust chi2, each sum closed by wave_sum
//   step(x)            what oplusImpl writes into the solver's x before it is applied
//   oplus(x)           the candidate: est moved by x
//   chi2(cand)         computeActiveErrors + activeRobustChi2 at the candidate
// All 64 lanes call it together: it holds __syncthreads().
template <int N, class Problem>
__device__ __forceinline__ LmRun levenberg(Problem& p, LmShared<N>& sh, LmState<N>& st, int maxIt, int lane)
{
    LmRun run = {0, 0, 0.0};
    for (int i = 0; i < kIterations; i++) {
        if (i >= maxIt) break;
        run.iterations++;
        double H[N * (N + 1) / 2], b[N], chiNow;
        p.build(H, b, chiNow);
        p.err = p.est;
        const double chiStart = chiNow;
        if (i == 0) {
            double diagMax = 0.;
            int q = 0;
#pragma unroll
            for (int j = 0; j < N; j++) {
                q += j;
                const double dj = fabs(H[q + j]);   // entry (j, j) of the lower triangle
                diagMax = (dj < diagMax) ? diagMax : dj;
            }
            st.lambda = 1e-5 * diagMax;
            st.growth = 2;
            st.flatSteps = 0;
        }
        double gain = 0;
        int nTried = 0;
        for (int t = 0; t < kTrials; t++) {
            __syncthreads();   // (the last trial's reads of sh.X / sh.ok are done)
            if (lane == 0) {
                int q = 0;
#pragma unroll
                for (int r = 0; r < N; r++)
#pragma unroll
                    for (int c = 0; c <= r; c++, q++) { sh.M[r * N + c] = H[q]; sh.M[c * N + r] = H[q]; }
#pragma unroll
                for (int r = 0; r < N; r++) { sh.M[r * N + r] = sh.M[r * N + r] + st.lambda; sh.B[r] = b[r]; }
                sh.ok = ldlt_solve<N>(sh.M, sh.B, sh.X, sh.Tr, sh.Tmp) ? 1 : 0;
            }
            __syncthreads();
            const bool solved = sh.ok != 0;
            if (solved) {
#pragma unroll
                for (int r = 0; r < N; r++) st.x[r] = sh.X[r];   // (else x keeps the last solve's)
            }
            p.step(st.x);
            const auto cand = p.oplus(st.x);
            double chiTrial = p.chi2(cand);
            p.err = cand;   // STALE ERRORS: a rejected trial leaves the edges' _error at the rejected estimate
            if (!solved) chiTrial = 1.7976931348623157e308;
            gain = (chiNow - chiTrial);
            double scale = 0.;
#pragma unroll
            for (int r = 0; r < N; r++) scale += st.x[r] * (st.lambda * st.x[r] + b[r]);
            scale += 1e-3;
            gain /= scale;
            if (gain > 0 && (chiTrial >= -1.7976931348623157e308 && chiTrial <= 1.7976931348623157e308)) {
                const double c = 2 * gain - 1;
                double keep = 1. - c * c * c;
                keep = ((2. / 3.) < keep) ? (2. / 3.) : keep;
                const double shrink = ((1. / 3.) < keep) ? keep : (1. / 3.);
                st.lambda *= shrink;
                st.growth = 2;
                chiNow = chiTrial;
                p.est = cand;
            } else {
                st.lambda *= st.growth;
                st.growth *= 2;
            }
            nTried++;
            if (!(gain < 0)) break;
        }
        run.trials += nTried;
        run.chi2 = chiNow;
        if (nTried == kTrials || gain == 0) break;
        if ((chiStart - chiNow) * 1e3 < chiStart) st.flatSteps++;
        else st.flatSteps = 0;
        if (st.flatSteps >= 3) break;
    }
    return run;
}

}  // namespace orbg
