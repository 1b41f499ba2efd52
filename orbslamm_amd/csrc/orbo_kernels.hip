// orbo_kernels.hip -- device PoseOptimization (part of orbslamm_hip.hip; host side: orbo_host.inc, ABI:
// include/orbslamm_poseopt.h): Optimizer::PoseOptimization (src/Optimizer.cc:261-473), monocular, for a
// batch of frames in ONE launch.  One wave owns a frame from its first round to its last: the frame's edges are strided over
// the 64 lanes (edge e is lane e % 64's, always), every lane keeps its partial H (21), b (6) and chi2 in registers, and the
// sums are closed by the xor butterfly 32, 16, ..., 1 -- THE SUMMATION TREE of §8o, a function of the edge count alone.  The
// pose, lambda and the Levenberg state are wave-uniform and computed redundantly by every lane; the 6 x 6 pivoted LDLT and
// its solve run on lane 0 in LDS (the pivoting indexes at run time) and the step is read back by all.
// Binary64 throughout, built with -ffp-contract=off, no atomics; every loop is bounded at compile time (4 rounds, 10
// iterations, 10 trials, kMaxEdgesPerLane edges), so no input can make the kernel spin.
// A lane reads back only per-edge words that the same lane wrote (the gathered edges, the outlier bytes): no fence is needed.
#pragma once

namespace orbo {

constexpr int kLanes = 64;
constexpr int kMaxEdges = 65535;                 // ORBO_MAX_EDGES
constexpr int kMaxFrames = 4096;                 // ORBO_MAX_FRAMES
constexpr int kMaxEdgesPerLane = (kMaxEdges + kLanes - 1) / kLanes;
constexpr int kRounds = 4, kIterations = 10, kTrials = 10;

struct FrameIn {
    float Tcw[16];
    float K[4];
    const orbm::KeyDev* keys;   // a device-resident frame's mvKeysUn, or null: the edge's observation is in Args::obs
    int32_t nKeys, e0, n, pad;
};
struct Obs { float u, v; int32_t octave; };
struct Args {
    const FrameIn* frames;
    const OrboEdge* edges;
    const Obs* obs;
    float4* pw;          // per edge: Xw, invSigma2 (written and read by the edge's lane)
    float2* uv;          // per edge: the observation
    OrboResult* out;
    uint8_t* outlier;
    float invSigma2[ORBX_MAX_LEVELS];
    int32_t nlevels;
};

struct Pose { double qx, qy, qz, qw, tx, ty, tz; };
struct Cam { double fx, fy, cx, cy; };

// ---- the sin / cos of §8o: + - * /, comparisons and integer conversion only
__device__ __forceinline__ double trunc_defined(double q)
{
    const double a = q < 0 ? -q : q;
    if (!(a < 4503599627370496.0)) return q;
    return (double)(long long)q;
}

__device__ __noinline__ void sincos_defined(double x, double& sOut, double& cOut)
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

// ---- Eigen's quaternion pieces on named scalars
__device__ __forceinline__ void normalize_rotation(double& x, double& y, double& z, double& w)
{
    if (w < 0) { x = x * -1.0; y = y * -1.0; z = z * -1.0; w = w * -1.0; }
    const double n = sqrt(x * x + y * y + z * z + w * w);
    x = x / n; y = y / n; z = z / n; w = w / n;
}

// Quaterniond(R), R given by its nine entries; the largest-diagonal branch written out for i = 0, 1, 2
__device__ __forceinline__ void quat_of_matrix(double r00, double r01, double r02, double r10, double r11, double r12, double r20, double r21,
                                               double r22, double& x, double& y, double& z, double& w)
{
    double t = r00 + r11 + r22;
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        x = (r21 - r12) * t;
        y = (r02 - r20) * t;
        z = (r10 - r01) * t;
        return;
    }
    int i = 0;
    if (r11 > r00) i = 1;
    if (r22 > (i == 0 ? r00 : r11)) i = 2;
    if (i == 0) {          // j = 1, k = 2
        t = sqrt(r00 - r11 - r22 + 1.0);
        x = 0.5 * t;
        t = 0.5 / t;
        w = (r21 - r12) * t;
        y = (r10 + r01) * t;
        z = (r20 + r02) * t;
    } else if (i == 1) {   // j = 2, k = 0
        t = sqrt(r11 - r22 - r00 + 1.0);
        y = 0.5 * t;
        t = 0.5 / t;
        w = (r02 - r20) * t;
        z = (r21 + r12) * t;
        x = (r01 + r10) * t;
    } else {               // j = 0, k = 1
        t = sqrt(r22 - r00 - r11 + 1.0);
        z = 0.5 * t;
        t = 0.5 / t;
        w = (r10 - r01) * t;
        x = (r02 + r20) * t;
        y = (r12 + r21) * t;
    }
}

// q * v (_transformVector)
__device__ __forceinline__ void rotate(const Pose& P, double vx, double vy, double vz, double& ox, double& oy, double& oz)
{
    double ux = P.qy * vz - P.qz * vy, uy = P.qz * vx - P.qx * vz, uz = P.qx * vy - P.qy * vx;
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    const double cx = P.qy * uz - P.qz * uy, cy = P.qz * ux - P.qx * uz, cz = P.qx * uy - P.qy * ux;
    ox = (vx + P.qw * ux) + cx;
    oy = (vy + P.qw * uy) + cy;
    oz = (vz + P.qw * uz) + cz;
}

// Converter::toSE3Quat
__device__ __forceinline__ Pose pose_of_tcw(const float* T)
{
    Pose P;
    quat_of_matrix((double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10],
                   P.qx, P.qy, P.qz, P.qw);
    P.tx = (double)T[3]; P.ty = (double)T[7]; P.tz = (double)T[11];
    normalize_rotation(P.qx, P.qy, P.qz, P.qw);
    return P;
}

// exp(dx) * P: SE3Quat::exp, then SE3Quat::operator*
__device__ __noinline__ Pose oplus(const Pose& P, double w0, double w1, double w2, double u0, double u1, double u2)
{
    const double theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    // Omega = skew(omega) and Omega * Omega, full 3 x 3 products (the zeros multiply: an infinity stays a NaN as it does there)
    const double o00 = 0.0, o01 = -w2, o02 = w1, o10 = w2, o11 = 0.0, o12 = -w0, o20 = -w1, o21 = w0, o22 = 0.0;
#define ORBO_MM(i, j) ((o##i##0 * o0##j + o##i##1 * o1##j) + o##i##2 * o2##j)
    const double s00 = ORBO_MM(0, 0), s01 = ORBO_MM(0, 1), s02 = ORBO_MM(0, 2), s10 = ORBO_MM(1, 0), s11 = ORBO_MM(1, 1), s12 = ORBO_MM(1, 2),
                 s20 = ORBO_MM(2, 0), s21 = ORBO_MM(2, 1), s22 = ORBO_MM(2, 2);
#undef ORBO_MM
    double a = 1.0, b = 1.0, d = 1.0;
    const bool small = theta < 0.00001;
    if (!small) {
        double s, c;
        sincos_defined(theta, s, c);
        a = s / theta;
        b = (1.0 - c) / (theta * theta);
        d = (theta - s) / (theta * theta * theta);
    }
    // R = I + a Omega + b Omega^2, V = I + b Omega + d Omega^2; below the threshold R = V = I + Omega + Omega^2 with no factor
#define ORBO_R(i, j, id) (small ? ((id + o##i##j) + s##i##j) : ((id + a * o##i##j) + b * s##i##j))
#define ORBO_V(i, j, id) (small ? ((id + o##i##j) + s##i##j) : ((id + b * o##i##j) + d * s##i##j))
    Pose E;
    quat_of_matrix(ORBO_R(0, 0, 1.0), ORBO_R(0, 1, 0.0), ORBO_R(0, 2, 0.0), ORBO_R(1, 0, 0.0), ORBO_R(1, 1, 1.0), ORBO_R(1, 2, 0.0), ORBO_R(2, 0, 0.0),
                   ORBO_R(2, 1, 0.0), ORBO_R(2, 2, 1.0), E.qx, E.qy, E.qz, E.qw);
    E.tx = (ORBO_V(0, 0, 1.0) * u0 + ORBO_V(0, 1, 0.0) * u1) + ORBO_V(0, 2, 0.0) * u2;
    E.ty = (ORBO_V(1, 0, 0.0) * u0 + ORBO_V(1, 1, 1.0) * u1) + ORBO_V(1, 2, 0.0) * u2;
    E.tz = (ORBO_V(2, 0, 0.0) * u0 + ORBO_V(2, 1, 0.0) * u1) + ORBO_V(2, 2, 1.0) * u2;
#undef ORBO_R
#undef ORBO_V
    normalize_rotation(E.qx, E.qy, E.qz, E.qw);
    Pose O;
    double rx, ry, rz;
    rotate(E, P.tx, P.ty, P.tz, rx, ry, rz);
    O.tx = E.tx + rx; O.ty = E.ty + ry; O.tz = E.tz + rz;
    O.qw = E.qw * P.qw - E.qx * P.qx - E.qy * P.qy - E.qz * P.qz;
    O.qx = E.qw * P.qx + E.qx * P.qw + E.qy * P.qz - E.qz * P.qy;
    O.qy = E.qw * P.qy + E.qy * P.qw + E.qz * P.qx - E.qx * P.qz;
    O.qz = E.qw * P.qz + E.qz * P.qw + E.qx * P.qy - E.qy * P.qx;
    normalize_rotation(O.qx, O.qy, O.qz, O.qw);
    return O;
}

// ---- the edge
struct EdgeReg { double u, v, w00, w01, w10, w11, X, Y, Z; };

__device__ __forceinline__ EdgeReg load_edge(const Args& a, int e)
{
    const float4 p = a.pw[e];
    const float2 o = a.uv[e];
    EdgeReg E;
    E.u = (double)o.x; E.v = (double)o.y;
    const double w = (double)p.w;
    E.w00 = 1.0 * w; E.w01 = 0.0 * w; E.w10 = 0.0 * w; E.w11 = 1.0 * w;
    E.X = (double)p.x; E.Y = (double)p.y; E.Z = (double)p.z;
    return E;
}

__device__ __forceinline__ void camera_point(const Pose& P, const EdgeReg& E, double& x, double& y, double& z)
{
    double rx, ry, rz;
    rotate(P, E.X, E.Y, E.Z, rx, ry, rz);
    x = rx + P.tx; y = ry + P.ty; z = rz + P.tz;
}

__device__ __forceinline__ void edge_error(const Cam& K, const EdgeReg& E, double x, double y, double z, double& e0, double& e1)
{
    const double px = x / z, py = y / z;
    e0 = E.u - (px * K.fx + K.cx);
    e1 = E.v - (py * K.fy + K.cy);
}

__device__ __forceinline__ double edge_chi2(const EdgeReg& E, double e0, double e1)
{
    const double t0 = E.w00 * e0 + E.w01 * e1, t1 = E.w10 * e0 + E.w11 * e1;
    return e0 * t0 + e1 * t1;
}

// the Huber kernel on a chi2: the robust cost and the weight (its first derivative)
__device__ __forceinline__ void huber(double c, double delta, double delta2, double& cost, double& weight)
{
    if (c <= delta2) { cost = c; weight = 1.; }
    else {
        const double sq = sqrt(c);
        cost = 2 * sq * delta - delta2;
        weight = delta / sq;
    }
}

// a NaN among the outputs leaves as ONE pattern, x86's default NaN: a NaN born on the device is 0x7FF8..., on x86 0xFFF8..., and
// which operand's NaN an operation hands on is the machine's (the PnP kernels do the same)
__device__ __forceinline__ double nan_canon(double v) { return v != v ? __longlong_as_double((long long)0xFFF8000000000000ull) : v; }
__device__ __forceinline__ float nan_canon_f(double v) { const float f = (float)v; return f != f ? __uint_as_float(0xFFC00000u) : f; }

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, kLanes);
    return v;
}

// computeActiveErrors + activeRobustChi2 at pose P
__device__ __noinline__ double pass_chi2(const Args& a, int e0, int n, int lane, const Pose& P, const Cam& K, bool robust, double delta, double delta2)
{
    double part = 0.0;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= n) break;
        if (a.outlier[e0 + e]) continue;
        const EdgeReg E = load_edge(a, e0 + e);
        double x, y, z, r0, r1;
        camera_point(P, E, x, y, z);
        edge_error(K, E, x, y, z, r0, r1);
        const double c = edge_chi2(E, r0, r1);
        if (robust) {
            double cost, weight;
            huber(c, delta, delta2, cost, weight);
            part = part + cost;
        } else part = part + c;
    }
    return wave_sum(part);
}

// the same chi2 sum fused with buildSystem at the estimate: H's lower triangle (row by row), b, chi2
__device__ __noinline__ void pass_build(const Args& a, int e0, int n, int lane, const Pose& P, const Cam& K, bool robust, double delta, double delta2,
                                        double (&H)[21], double (&b)[6], double& chiOut)
{
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 21; i++) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) b[i] = 0.0;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= n) break;
        if (a.outlier[e0 + e]) continue;
        const EdgeReg E = load_edge(a, e0 + e);
        double x, y, z, r0, r1;
        camera_point(P, E, x, y, z);
        edge_error(K, E, x, y, z, r0, r1);
        const double c = edge_chi2(E, r0, r1);
        double cost = c, weight = 1.0;
        if (robust) huber(c, delta, delta2, cost, weight);
        chi = chi + cost;
        // the projection's derivative by the pose increment (rotation part first), row u then row v; the order of the operations
        // is the edge type's
        const double iz = 1.0 / z, iz2 = iz * iz, xy = x * y;
        double J0[6], J1[6];
        J0[0] = xy * iz2 * K.fx;
        J0[1] = -(1.0 + x * x * iz2) * K.fx;
        J0[2] = y * iz * K.fx;
        J0[3] = -iz * K.fx;
        J0[4] = 0.0;
        J0[5] = x * iz2 * K.fx;
        J1[0] = (1.0 + y * y * iz2) * K.fy;
        J1[1] = -xy * iz2 * K.fy;
        J1[2] = -x * iz * K.fy;
        J1[3] = 0.0;
        J1[4] = -iz * K.fy;
        J1[5] = y * iz2 * K.fy;
        // constructQuadraticForm: with a kernel b -= ((weight A^T) Omega) e and H += (A^T (weight Omega)) A, without b -= (A^T Omega) e
        // and H += (A^T Omega) A
        const double W00 = robust ? weight * E.w00 : E.w00, W01 = robust ? weight * E.w01 : E.w01, W10 = robust ? weight * E.w10 : E.w10,
                     W11 = robust ? weight * E.w11 : E.w11;
        double T0[6], T1[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double l0 = robust ? weight * J0[i] : J0[i], l1 = robust ? weight * J1[i] : J1[i];
            const double g0 = l0 * E.w00 + l1 * E.w10, g1 = l0 * E.w01 + l1 * E.w11;
            b[i] = b[i] - (g0 * r0 + g1 * r1);
            T0[i] = J0[i] * W00 + J1[i] * W10;
            T1[i] = J0[i] * W01 + J1[i] * W11;
        }
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++, q++) H[q] = H[q] + (T0[i] * J0[j] + T1[i] * J1[j]);
    }
#pragma unroll
    for (int i = 0; i < 21; i++) H[i] = wave_sum(H[i]);
#pragma unroll
    for (int i = 0; i < 6; i++) b[i] = wave_sum(b[i]);
    chiOut = wave_sum(chi);
}

// Eigen's unblocked LDLT with diagonal pivoting on the lower triangle of M (6 x 6 in LDS, row-major), isPositive(), solve:
// one lane.  Returns isPositive(); x is written only then.
__device__ __noinline__ bool ldlt_solve6(double* M, const double* rhs, double* x, int* tr, double* tmp)
{
    constexpr int n = 6;
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

__global__ __launch_bounds__(kLanes) void k_pose_optimize(Args a, int nFrames)
{
    __shared__ double sM[36], sB[6], sX[6], sTmp[6];
    __shared__ int sTr[6], sOk;
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= nFrames) return;
    const FrameIn& F = a.frames[f];
    const int e0 = F.e0, n = F.n;
    OrboResult* out = a.out + f;
    // the gather (Optimizer.cc:302-341): observation, information, world position of the lane's edges; mvbOutlier = false
    bool bad = false;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= n) break;
        const OrboEdge ed = a.edges[e0 + e];
        float u, v;
        int oct;
        if (F.keys) { const orbm::KeyDev kp = F.keys[ed.feature]; u = kp.x; v = kp.y; oct = kp.octave; }
        else { const Obs o = a.obs[e0 + e]; u = o.u; v = o.v; oct = o.octave; }
        const bool okOct = oct >= 0 && oct < a.nlevels;
        bad |= !okOct;
        a.pw[e0 + e] = make_float4(ed.Xw[0], ed.Xw[1], ed.Xw[2], okOct ? a.invSigma2[oct] : 0.f);
        a.uv[e0 + e] = make_float2(u, v);
        a.outlier[e0 + e] = 0;
    }
    const bool anyBad = __any(bad);
    if (lane == 0) {
        for (int i = 0; i < 16; i++) out->Tcw[i] = F.Tcw[i];
        out->n_initial = n; out->n_good = 0; out->rounds = anyBad ? -1 : 0;   // (-1: an octave outside nlevels; the host refuses)
        for (int r = 0; r < kRounds; r++) { out->iterations[r] = 0; out->trials[r] = 0; out->lambda[r] = 0.0; out->chi2[r] = 0.0; }
    }
    if (anyBad || n < 3) return;   // :386

    const Cam K = {(double)F.K[0], (double)F.K[1], (double)F.K[2], (double)F.K[3]};
    const double delta = (double)2.44765191f;   // (float)sqrt(5.991), widened (:295)
    const double delta2 = delta * delta;
    bool robust = true;
    double lambda = -1., growth = 2.;
    int flatSteps = 0;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, x4 = 0.0, x5 = 0.0;   // the solver's x: lives across the rounds
    Pose est = pose_of_tcw(F.Tcw);
    int nBad = 0, rounds = 0;
    for (int it = 0; it < kRounds; it++) {
        // every round starts from the caller's pose: mTcw is written only at the end (:399, :470)
        est = pose_of_tcw(F.Tcw);
        Pose errPose = est;   // where the active edges' _error was last computed
        int nActive = 0;
        for (int k = 0; k < kMaxEdgesPerLane; k++) {
            const int e = lane + k * kLanes;
            if (e >= n) break;
            nActive += a.outlier[e0 + e] == 0;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nActive += __shfl_xor(nActive, m, kLanes);
        int iterations = 0, trials = 0;
        double chiRound = 0.0;
        if (nActive > 0) {
            for (int i = 0; i < kIterations; i++) {
                iterations++;
                double H[21], b[6], chiNow;
                pass_build(a, e0, n, lane, est, K, robust, delta, delta2, H, b, chiNow);
                errPose = est;
                const double chiStart = chiNow;
                if (i == 0) {
                    double diagMax = 0.;
                    {
                        const double d0 = fabs(H[0]), d1 = fabs(H[2]), d2 = fabs(H[5]), d3 = fabs(H[9]), d4 = fabs(H[14]), d5 = fabs(H[20]);
                        diagMax = (d0 < diagMax) ? diagMax : d0;
                        diagMax = (d1 < diagMax) ? diagMax : d1;
                        diagMax = (d2 < diagMax) ? diagMax : d2;
                        diagMax = (d3 < diagMax) ? diagMax : d3;
                        diagMax = (d4 < diagMax) ? diagMax : d4;
                        diagMax = (d5 < diagMax) ? diagMax : d5;
                    }
                    lambda = 1e-5 * diagMax;
                    growth = 2;
                    flatSteps = 0;
                }
                double gain = 0;
                int nTried = 0;
                for (int t = 0; t < kTrials; t++) {
                    __syncthreads();   // (the last trial's reads of sX / sOk are done)
                    if (lane == 0) {
                        int q = 0;
#pragma unroll
                        for (int r = 0; r < 6; r++)
#pragma unroll
                            for (int c = 0; c <= r; c++, q++) { sM[r * 6 + c] = H[q]; sM[c * 6 + r] = H[q]; }
#pragma unroll
                        for (int r = 0; r < 6; r++) { sM[r * 6 + r] = sM[r * 6 + r] + lambda; sB[r] = b[r]; }
                        sOk = ldlt_solve6(sM, sB, sX, sTr, sTmp) ? 1 : 0;
                    }
                    __syncthreads();
                    const bool solved = sOk != 0;
                    if (solved) { x0 = sX[0]; x1 = sX[1]; x2 = sX[2]; x3 = sX[3]; x4 = sX[4]; x5 = sX[5]; }   // (else x keeps the last solve's)
                    const Pose cand = oplus(est, x0, x1, x2, x3, x4, x5);
                    double chiTrial = pass_chi2(a, e0, n, lane, cand, K, robust, delta, delta2);
                    errPose = cand;   // STALE ERRORS: a rejected trial leaves the edges' _error at the rejected pose
                    if (!solved) chiTrial = 1.7976931348623157e308;
                    gain = (chiNow - chiTrial);
                    double scale = 0.;
                    scale += x0 * (lambda * x0 + b[0]);
                    scale += x1 * (lambda * x1 + b[1]);
                    scale += x2 * (lambda * x2 + b[2]);
                    scale += x3 * (lambda * x3 + b[3]);
                    scale += x4 * (lambda * x4 + b[4]);
                    scale += x5 * (lambda * x5 + b[5]);
                    scale += 1e-3;
                    gain /= scale;
                    if (gain > 0 && (chiTrial >= -1.7976931348623157e308 && chiTrial <= 1.7976931348623157e308)) {
                        const double c = 2 * gain - 1;
                        double keep = 1. - c * c * c;
                        keep = ((2. / 3.) < keep) ? (2. / 3.) : keep;
                        const double shrink = ((1. / 3.) < keep) ? keep : (1. / 3.);
                        lambda *= shrink;
                        growth = 2;
                        chiNow = chiTrial;
                        est = cand;
                    } else {
                        lambda *= growth;
                        growth *= 2;
                    }
                    nTried++;
                    if (!(gain < 0)) break;
                }
                trials += nTried;
                chiRound = chiNow;
                if (nTried == kTrials || gain == 0) break;
                if ((chiStart - chiNow) * 1e3 < chiStart) flatSteps++;
                else flatSteps = 0;
                if (flatSteps >= 3) break;
            }
        }
        // the classification (:404-431): level-0 edges with the error of the last trial's pose, outliers with a fresh one
        nBad = 0;
        for (int k = 0; k < kMaxEdgesPerLane; k++) {
            const int e = lane + k * kLanes;
            if (e >= n) break;
            const EdgeReg E = load_edge(a, e0 + e);
            const bool was = a.outlier[e0 + e] != 0;
            double x, y, z, r0, r1;
            camera_point(was ? est : errPose, E, x, y, z);
            edge_error(K, E, x, y, z, r0, r1);
            const float chi2 = (float)edge_chi2(E, r0, r1);
            const bool isOut = chi2 > 5.991f;
            a.outlier[e0 + e] = isOut ? 1 : 0;
            nBad += isOut;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nBad += __shfl_xor(nBad, m, kLanes);
        if (lane == 0) {
            out->iterations[it] = iterations; out->trials[it] = trials;
            out->lambda[it] = nActive > 0 ? nan_canon(lambda) : 0.0; out->chi2[it] = nan_canon(chiRound);
        }
        if (it == 2) robust = false;   // :429-430
        rounds = it + 1;
        if (n < 10) break;   // :462
    }
    if (lane == 0) {
        // Converter::toCvMat(SE3Quat): toRotationMatrix, narrowed
        const double tx = 2.0 * est.qx, ty = 2.0 * est.qy, tz = 2.0 * est.qz;
        const double twx = tx * est.qw, twy = ty * est.qw, twz = tz * est.qw;
        const double txx = tx * est.qx, txy = ty * est.qx, txz = tz * est.qx;
        const double tyy = ty * est.qy, tyz = tz * est.qy, tzz = tz * est.qz;
        float* T = out->Tcw;
        T[0] = nan_canon_f(1.0 - (tyy + tzz)); T[1] = nan_canon_f(txy - twz); T[2] = nan_canon_f(txz + twy); T[3] = nan_canon_f(est.tx);
        T[4] = nan_canon_f(txy + twz); T[5] = nan_canon_f(1.0 - (txx + tzz)); T[6] = nan_canon_f(tyz - twx); T[7] = nan_canon_f(est.ty);
        T[8] = nan_canon_f(txz - twy); T[9] = nan_canon_f(tyz + twx); T[10] = nan_canon_f(1.0 - (txx + tyy)); T[11] = nan_canon_f(est.tz);
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
        out->n_good = n - nBad;
        out->rounds = rounds;
    }
}

}  // namespace orbo
