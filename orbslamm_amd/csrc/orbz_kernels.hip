// orbz_kernels.hip -- device OptimizeSim3 (part of orbslamm_hip.hip; host side: orbz_host.inc, ABI: include/orbslamm_sim3opt.h,
// DESIGN.md §8p): Optimizer::OptimizeSim3 (src/Optimizer.cc:1348-1543), monocular, for a batch of loop / merge candidates in ONE
// launch.  One wave owns a problem from its first pass to its last.  Correspondence c owns edge 2c (e12: S12 maps pKF2's point into
// camera 1) and edge 2c + 1 (e21: the inverse maps pKF1's point into camera 2); edge e is lane e % 64's, always, so even lanes hold
// e12 edges and odd lanes e21 edges and the difference between them is DATA (which record set, which K, which point), not control
// flow.  Every lane keeps its partial H (28), b (7) and chi2 in registers and the sums are closed by the xor butterfly 32 .. 1 --
// THE SUMMATION TREE of §8o over the edge index.
// g2o differentiates these edges NUMERICALLY (linearizeOplus is commented out in types_seven_dof_expmap.h): 14 perturbed
// estimates Sim3(+-1e-9 e_d) * S per linearisation.  They and their inverses depend on the problem, not on the edge: lanes 0 .. 13
// compute them once into LDS (with the base estimate 30 records of 8 doubles) and every edge evaluates its 15 errors from there.
// The estimate, lambda and the Levenberg state are wave-uniform and computed redundantly by every lane; the 7 x 7 pivoted LDLT runs
// on lane 0 in LDS.  Binary64 throughout, -ffp-contract=off, no atomics; every loop is bounded at compile time (2 passes, 5 / 10
// iterations, 10 trials, kMaxEdgesPerLane edges).  A lane reads back only per-edge words that the same lane wrote.
#pragma once

namespace orbz {

constexpr int kLanes = 64;
constexpr int kMaxCorr = 32767;                  // ORBZ_MAX_CORR
constexpr int kMaxProblems = 4096;               // ORBZ_MAX_PROBLEMS
constexpr int kMaxEdgesPerLane = (2 * kMaxCorr + kLanes - 1) / kLanes;
constexpr int kPasses = 2, kIterations = 10, kTrials = 10;
constexpr int kRecords = 30;                     // (base + 14 perturbed) x (itself, its inverse)

struct ProblemIn {
    OrbzProblem p;
    double delta;        // (double)sqrtf(th2): the Huber width (:1398), taken on the host
    int32_t c0, n;
};
struct Args {
    const ProblemIn* problems;
    const OrbzCorr* corrs;
    float4* pw;          // per edge: the camera-frame point, invSigma2 (written and read by the edge's lane)
    float2* uv;          // per edge: the observation
    uint8_t* off;        // per edge: its pair was removed by the first check (written and read by the edge's lane)
    OrbzResult* out;
    uint8_t* removed;    // per correspondence: the output (written by the even lane, never read here)
    const float* invSigma2;   // the two keyframes' level tables, ORBX_MAX_LEVELS floats each
    int32_t nlevels;
};

struct S3 { double qx, qy, qz, qw, tx, ty, tz, s; };
struct Cam { double fx, fy, cx, cy; };

// ---- the exp of §8p: + - * /, comparisons, integer conversion, 2^k from its exponent bits
__device__ __forceinline__ double pow2_bits(int k) { return __longlong_as_double((long long)(k + 1023) << 52); }

__device__ __forceinline__ double exp_defined(double x)
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

// q * v (_transformVector), for a quaternion that need not be a unit one
__device__ __forceinline__ void rotate(const S3& P, double vx, double vy, double vz, double& ox, double& oy, double& oz)
{
    double ux = P.qy * vz - P.qz * vy, uy = P.qz * vx - P.qx * vz, uz = P.qx * vy - P.qy * vx;
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    const double cx = P.qy * uz - P.qz * uy, cy = P.qz * ux - P.qx * uz, cz = P.qx * uy - P.qy * ux;
    ox = (vx + P.qw * ux) + cx;
    oy = (vy + P.qw * uy) + cy;
    oz = (vz + P.qw * uz) + cz;
}

// Sim3::inverse: Sim3(conj, conj * ((-1. / s) * t), 1. / s)
__device__ __forceinline__ S3 inverse(const S3& S)
{
    S3 o;
    o.qx = -S.qx; o.qy = -S.qy; o.qz = -S.qz; o.qw = S.qw;
    const double f = -1. / S.s;
    rotate(o, f * S.tx, f * S.ty, f * S.tz, o.tx, o.ty, o.tz);
    o.s = 1. / S.s;
    return o;
}

// Sim3(update) * P: the constructor's four branches (types/sim3.h:70-142), then operator* with NO normalisation
__device__ __noinline__ S3 oplus(const S3 P, double w0, double w1, double w2, double u0, double u1, double u2, double sigma)
{
    const double theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double Om[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double Id[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    S3 E;
    E.s = exp_defined(sigma);
    double Om2[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Om2[i * 3 + j] = (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
    const bool smallTheta = theta < 0.00001;
    double sn = 0.0, cs = 0.0;
    if (!smallTheta) orbo::sincos_defined(theta, sn, cs);
    {
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = smallTheta ? ((Id[k] + Om[k]) + Om2[k]) : ((Id[k] + a * Om[k]) + b * Om2[k]);
    }
    double A, B, C;
    if (fabs(sigma) < 0.00001) {
        C = 1;
        if (smallTheta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cs) / (theta2);
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (E.s - 1) / sigma;
        if (smallTheta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * E.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * E.s) / (sigma2 * sigma);
        } else {
            const double a = E.s * sn, b = E.s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    orbo::quat_of_matrix(R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], E.qx, E.qy, E.qz, E.qw);
    double W[9];
#pragma unroll
    for (int k = 0; k < 9; k++) W[k] = (A * Om[k] + B * Om2[k]) + C * Id[k];
    E.tx = (W[0] * u0 + W[1] * u1) + W[2] * u2;
    E.ty = (W[3] * u0 + W[4] * u1) + W[5] * u2;
    E.tz = (W[6] * u0 + W[7] * u1) + W[8] * u2;
    S3 O;
    O.qw = E.qw * P.qw - E.qx * P.qx - E.qy * P.qy - E.qz * P.qz;
    O.qx = E.qw * P.qx + E.qx * P.qw + E.qy * P.qz - E.qz * P.qy;
    O.qy = E.qw * P.qy + E.qy * P.qw + E.qz * P.qx - E.qx * P.qz;
    O.qz = E.qw * P.qz + E.qz * P.qw + E.qx * P.qy - E.qy * P.qx;
    double rx, ry, rz;
    rotate(E, P.tx, P.ty, P.tz, rx, ry, rz);
    O.tx = E.s * rx + E.tx; O.ty = E.s * ry + E.ty; O.tz = E.s * rz + E.tz;
    O.s = E.s * P.s;
    return O;
}

__device__ __forceinline__ void store_record(double* rec, const S3& S)
{
    rec[0] = S.qx; rec[1] = S.qy; rec[2] = S.qz; rec[3] = S.qw; rec[4] = S.tx; rec[5] = S.ty; rec[6] = S.tz; rec[7] = S.s;
}
__device__ __forceinline__ S3 load_record(const double* rec)
{
    S3 S;
    S.qx = rec[0]; S.qy = rec[1]; S.qz = rec[2]; S.qw = rec[3]; S.tx = rec[4]; S.ty = rec[5]; S.tz = rec[6]; S.s = rec[7];
    return S;
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

// computeError of either edge type: obs - cam_map(project(S.map(P))), S being the estimate or its inverse by the edge's side
__device__ __forceinline__ void edge_error(const S3& S, const Cam& K, const EdgeReg& E, double& e0, double& e1)
{
    double rx, ry, rz;
    rotate(S, E.X, E.Y, E.Z, rx, ry, rz);
    const double x = S.s * rx + S.tx, y = S.s * ry + S.ty, z = S.s * rz + S.tz;
    const double px = x / z, py = y / z;
    e0 = E.u - (px * K.fx + K.cx);
    e1 = E.v - (py * K.fy + K.cy);
}

__device__ __forceinline__ double edge_chi2(const EdgeReg& E, double e0, double e1)
{
    const double t0 = E.w00 * e0 + E.w01 * e1, t1 = E.w10 * e0 + E.w11 * e1;
    return e0 * t0 + e1 * t1;
}

// computeActiveErrors + activeRobustChi2 at estimate S (Sinv its inverse; the lane's side picks)
__device__ __forceinline__ double pass_chi2(const Args& a, int e0, int nE, int lane, const S3& mine, const Cam& K, double delta, double delta2)
{
    double part = 0.0;
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= nE) break;
        if (a.off[e0 + e]) continue;
        const EdgeReg E = load_edge(a, e0 + e);
        double r0, r1, cost, weight;
        edge_error(mine, K, E, r0, r1);
        orbo::huber(edge_chi2(E, r0, r1), delta, delta2, cost, weight);
        part = part + cost;
    }
    return orbo::wave_sum(part);
}

// the same chi2 sum fused with buildSystem at the estimate: the numeric Jacobian from the records in LDS, H's lower triangle
// (row by row), b, chi2.  rec: the lane's side's record set, 15 records at a stride of 16 doubles
__device__ __forceinline__ void pass_build(const Args& a, int e0, int nE, int lane, const double* rec, const Cam& K, double delta, double delta2,
                                           double (&H)[28], double (&b)[7], double& chiOut)
{
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 28; i++) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) b[i] = 0.0;
    const double scalar = 1.0 / (2 * 1e-9);
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= nE) break;
        if (a.off[e0 + e]) continue;
        const EdgeReg E = load_edge(a, e0 + e);
        double r0, r1;
        edge_error(load_record(rec), K, E, r0, r1);
        double B0[7], B1[7];
#pragma unroll
        for (int d = 0; d < 7; d++) {
            double p0, p1, m0, m1;
            edge_error(load_record(rec + (1 + 2 * d) * 16), K, E, p0, p1);
            edge_error(load_record(rec + (2 + 2 * d) * 16), K, E, m0, m1);
            B0[d] = scalar * (p0 - m0);
            B1[d] = scalar * (p1 - m1);
        }
        double cost, weight;
        orbo::huber(edge_chi2(E, r0, r1), delta, delta2, cost, weight);
        chi = chi + cost;
        // constructQuadraticForm, robust, the `to` vertex: omega_r = -(Omega e), *= weight; b += B^T omega_r; H += (B^T (weight Omega)) B
        double g0 = -(E.w00 * r0 + E.w01 * r1), g1 = -(E.w10 * r0 + E.w11 * r1);
        g0 = g0 * weight; g1 = g1 * weight;
        const double W00 = weight * E.w00, W01 = weight * E.w01, W10 = weight * E.w10, W11 = weight * E.w11;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 7; i++) {
            b[i] = b[i] + (B0[i] * g0 + B1[i] * g1);
            const double t0 = B0[i] * W00 + B1[i] * W10, t1 = B0[i] * W01 + B1[i] * W11;
#pragma unroll
            for (int j = 0; j <= i; j++, q++) H[q] = H[q] + (t0 * B0[j] + t1 * B1[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 28; i++) H[i] = orbo::wave_sum(H[i]);
#pragma unroll
    for (int i = 0; i < 7; i++) b[i] = orbo::wave_sum(b[i]);
    chiOut = orbo::wave_sum(chi);
}

// orbo::ldlt_solve6 at size n: Eigen's unblocked LDLT with diagonal pivoting on the lower triangle of M (n x n in LDS, row-major),
// isPositive(), solve: one lane.  Returns isPositive(); x is written only then.
template <int n> __device__ __noinline__ bool ldlt_solve(double* M, const double* rhs, double* x, int* tr, double* tmp)
{
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

__global__ __launch_bounds__(kLanes) void k_sim3_optimize(Args a, int nProblems)
{
    // the records: [j][side] at (2 j + side) * 8, j = 0 the estimate, 1 + 2 d the +delta step of dimension d, 2 + 2 d the -delta
    // step; side 0 the Sim3 itself (e12 edges), side 1 its inverse (e21 edges)
    __shared__ double sRec[kRecords * 8];
    __shared__ double sM[49], sB[7], sX[7], sTmp[7];
    __shared__ int sTr[7], sOk;
    const int pIdx = blockIdx.x, lane = threadIdx.x, side = lane & 1;
    if (pIdx >= nProblems) return;
    const ProblemIn& P = a.problems[pIdx];
    const int c0 = P.c0, n = P.n, e0 = 2 * c0, nE = 2 * n;
    OrbzResult* out = a.out + pIdx;
    // the gather (Optimizer.cc:1401-1481): the observation, its level's information and the OTHER keyframe's point in ITS camera
    // frame (R * Xw + t through gemm's small branch, as orbs_create takes it); nothing removed yet
    for (int k = 0; k < kMaxEdgesPerLane; k++) {
        const int e = lane + k * kLanes;
        if (e >= nE) break;
        const OrbzCorr c = a.corrs[c0 + (e >> 1)];
        const float* R = side ? P.p.R1w : P.p.R2w;
        const float* t = side ? P.p.t1w : P.p.t2w;
        const float* Xw = side ? c.X1w : c.X2w;
        const int oct = side ? c.oct2 : c.oct1;
        float X[3];
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = cvm::gemm3_elem(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], Xw[0], Xw[1], Xw[2], 1.0, t[r], 1.0);
        const bool okOct = oct >= 0 && oct < a.nlevels;   // (the host has refused anything else)
        a.pw[e0 + e] = make_float4(X[0], X[1], X[2], okOct ? a.invSigma2[side * ORBX_MAX_LEVELS + oct] : 0.f);
        a.uv[e0 + e] = side ? make_float2(c.obs2[0], c.obs2[1]) : make_float2(c.obs1[0], c.obs1[1]);
        a.off[e0 + e] = 0;
        if (!side) a.removed[c0 + (e >> 1)] = 0;
    }
    S3 est;
    est.qx = P.p.q[0]; est.qy = P.p.q[1]; est.qz = P.p.q[2]; est.qw = P.p.q[3];
    est.tx = P.p.t[0]; est.ty = P.p.t[1]; est.tz = P.p.t[2]; est.s = P.p.s;
    if (lane == 0) {
        out->q[0] = est.qx; out->q[1] = est.qy; out->q[2] = est.qz; out->q[3] = est.qw;
        out->t[0] = est.tx; out->t[1] = est.ty; out->t[2] = est.tz; out->s = est.s;
        out->written = 0; out->n_corr = n; out->n_bad = 0; out->n_in = 0;
        for (int r = 0; r < kPasses; r++) { out->iterations[r] = 0; out->trials[r] = 0; out->lambda[r] = 0.0; out->chi2[r] = 0.0; }
    }
    if (n == 0) return;   // no edge: no vertex is found, no iteration runs, and 0 - 0 < 10 (:1514)

    const float* Kf = side ? P.p.K2 : P.p.K1;   // cam_map1 for e12, cam_map2 for e21
    const Cam K = {(double)Kf[0], (double)Kf[1], (double)Kf[2], (double)Kf[3]};
    const bool fixScale = P.p.fix_scale != 0;
    const double delta = P.delta, delta2 = delta * delta;
    const double th2 = (double)P.p.th2;
    const double* myRec = sRec + side * 8;
    double lambda = -1., growth = 2.;
    int flatSteps = 0;
    double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // the solver's x: lives across the passes
    int nBad = 0, nIn = 0;
    const int kEdgeRounds = (nE + kLanes - 1) / kLanes;
    for (int pass = 0; pass < kPasses; pass++) {
        const int maxIt = pass == 0 ? 5 : (nBad > 0 ? 10 : 5);   // :1485, :1508-1512
        S3 errS = est;   // where the active edges' _error was last computed
        int iterations = 0, trials = 0;
        double chiPass = 0.0;
        for (int i = 0; i < kIterations; i++) {
            if (i >= maxIt) break;
            iterations++;
            __syncthreads();   // (the last linearisation's reads of sRec are done)
            if (lane < 15) {
                // lane 14: the estimate; lanes 0 .. 13: the step +-delta along dimension lane / 2 (with its scale entry zeroed
                // under fix_scale, as oplusImpl zeroes it)
                const int d = lane >> 1;
                const double step = lane == 14 ? 0.0 : ((lane & 1) ? -1e-9 : 1e-9);
                const S3 Sp = lane == 14 ? est
                                         : oplus(est, d == 0 ? step : 0.0, d == 1 ? step : 0.0, d == 2 ? step : 0.0, d == 3 ? step : 0.0,
                                                 d == 4 ? step : 0.0, d == 5 ? step : 0.0, (d == 6 && !fixScale) ? step : 0.0);
                const int j = lane == 14 ? 0 : 1 + lane;
                store_record(sRec + (2 * j) * 8, Sp);
                store_record(sRec + (2 * j + 1) * 8, inverse(Sp));
            }
            __syncthreads();
            double H[28], b[7], chiNow;
            pass_build(a, e0, nE, lane, myRec, K, delta, delta2, H, b, chiNow);
            errS = est;
            const double chiStart = chiNow;
            if (i == 0) {
                double diagMax = 0.;
                int q = 0;
#pragma unroll
                for (int j = 0; j < 7; j++) {
                    q += j;
                    const double dj = fabs(H[q + j]);   // entry (j, j) of the lower triangle
                    diagMax = (dj < diagMax) ? diagMax : dj;
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
                    for (int r = 0; r < 7; r++)
#pragma unroll
                        for (int c = 0; c <= r; c++, q++) { sM[r * 7 + c] = H[q]; sM[c * 7 + r] = H[q]; }
#pragma unroll
                    for (int r = 0; r < 7; r++) { sM[r * 7 + r] = sM[r * 7 + r] + lambda; sB[r] = b[r]; }
                    sOk = ldlt_solve<7>(sM, sB, sX, sTr, sTmp) ? 1 : 0;
                }
                __syncthreads();
                const bool solved = sOk != 0;
                if (solved) {
#pragma unroll
                    for (int r = 0; r < 7; r++) x[r] = sX[r];   // (else x keeps the last solve's)
                }
                if (fixScale) x[6] = 0;   // oplusImpl writes the zero into the solver's x
                const S3 cand = oplus(est, x[0], x[1], x[2], x[3], x[4], x[5], x[6]);
                const S3 candInv = inverse(cand);
                double chiTrial = pass_chi2(a, e0, nE, lane, side ? candInv : cand, K, delta, delta2);
                errS = cand;   // STALE ERRORS: a rejected trial leaves the edges' _error at the rejected estimate
                if (!solved) chiTrial = 1.7976931348623157e308;
                gain = (chiNow - chiTrial);
                double scale = 0.;
#pragma unroll
                for (int r = 0; r < 7; r++) scale += x[r] * (lambda * x[r] + b[r]);
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
            chiPass = chiNow;
            if (nTried == kTrials || gain == 0) break;
            if ((chiStart - chiNow) * 1e3 < chiStart) flatSteps++;
            else flatSteps = 0;
            if (flatSteps >= 3) break;
        }
        // the check (:1489-1506, :1523-1537): both edges of a pair with the error of the last trial's estimate; the pair's two lanes
        // exchange their chi2.  The loop bound is wave-uniform so that both lanes of every pair reach the exchange
        const S3 errInv = inverse(errS);
        const S3 mine = side ? errInv : errS;
        int bad = 0, in = 0;
        for (int k = 0; k < kMaxEdgesPerLane; k++) {
            if (k >= kEdgeRounds) break;
            const int e = lane + k * kLanes;
            const bool live = e < nE && a.off[e0 + (e < nE ? e : 0)] == 0;
            double c = 0.0;
            if (live) {
                const EdgeReg E = load_edge(a, e0 + e);
                double r0, r1;
                edge_error(mine, K, E, r0, r1);
                c = edge_chi2(E, r0, r1);
            }
            const double other = __shfl_xor(c, 1, kLanes);
            if (live) {
                const bool fails = c > th2 || other > th2;
                if (fails) {
                    if (pass == 0) a.off[e0 + e] = 1;
                    if (!side) a.removed[c0 + (e >> 1)] = (uint8_t)(pass + 1);
                }
                if (!side) { bad += fails; in += !fails; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { bad += __shfl_xor(bad, m, kLanes); in += __shfl_xor(in, m, kLanes); }
        if (pass == 0) nBad = bad;
        else nIn = in;
        if (lane == 0) {
            out->iterations[pass] = iterations; out->trials[pass] = trials;
            out->lambda[pass] = orbo::nan_canon(lambda); out->chi2[pass] = orbo::nan_canon(chiPass);
            out->n_bad = nBad;
        }
        if (pass == 0 && n - nBad < 10) return;   // :1514: before g2oS12 is written; the nulled matches stay nulled
    }
    if (lane == 0) {
        out->q[0] = orbo::nan_canon(est.qx); out->q[1] = orbo::nan_canon(est.qy); out->q[2] = orbo::nan_canon(est.qz); out->q[3] = orbo::nan_canon(est.qw);
        out->t[0] = orbo::nan_canon(est.tx); out->t[1] = orbo::nan_canon(est.ty); out->t[2] = orbo::nan_canon(est.tz); out->s = orbo::nan_canon(est.s);
        out->written = 1;
        out->n_in = nIn;
    }
}

}  // namespace orbz
