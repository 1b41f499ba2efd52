// orbg_schur.hip -- the g2o / Eigen pieces of a bundle adjustment with marginalised points (part of orbslamm_hip.hip), beside
// orbg_kernels.hip whose sin / cos, quaternion pieces, edge record, Huber kernel, wave_sum and NaN canonicalisers it uses: the
// two-vertex edge EdgeSE3ProjectXYZ with both Jacobians and BaseBinaryEdge's quadratic form, Eigen's 3 x 3 inverse, one
// landmark's share of BlockSolver::solve's Schur complement, the unpivoted LDLt of the reduced system at size N, the landmark
// back-substitution, and ONE run of OptimizationAlgorithmLevenberg over the FULL system (poses and points) on a problem object
// that the calling kernel defines.  The first kernel on it is orbb_kernels.hip; a local bundle adjustment would
// stand on the same pieces.  Every line is held bit for bit to tools/initmap_ref.hpp (which shares nothing with this file):
// one IEEE operation per source operation (-ffp-contract=off).  The scalar pieces are __host__ __device__, so a program with no
// device holds them to the restatement as well (tests/cpp/schur_core_check.hip).  Needs nothing of the library.
#pragma once

#include "orbg_kernels.hip"

namespace orbg {

constexpr int kBaIterations = 20;   // the most one optimize() call of the full system runs

struct SE3Pose { Quat q; double tx, ty, tz; };

// std::max(a, b)
__host__ __device__ __forceinline__ double max_of(double a, double b) { return (a < b) ? b : a; }

// the index of entry (i, j), i <= j, among the 21 of a 6 x 6 upper triangle, row by row
__host__ __device__ constexpr int upper_index(int i, int j) { return i * (13 - i) / 2 + (j - i); }

// Eigen's QuaternionBase::toRotationMatrix, row-major
__host__ __device__ __forceinline__ void quat_to_matrix(const Quat& q, double (&R)[9])
{
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// SE3Quat::map of the edge's point
__host__ __device__ __forceinline__ void se3_map(const SE3Pose& P, double X, double Y, double Z, double& x, double& y, double& z)
{
    double rx, ry, rz;
    rotate(P.q, X, Y, Z, rx, ry, rz);
    x = rx + P.tx; y = ry + P.ty; z = rz + P.tz;
}

// ---- the two-vertex edge (types_six_dof_expmap.cpp:103-138): E carries the observation, the information and the POINT's estimate.
// computeError, and linearizeOplus: A = _jacobianOplusXi (2 x 3, by the point: -1./z * tmp * R, the scaled tmp formed first),
// B = _jacobianOplusXj (2 x 6, by the pose), both row-major, in the edge type's operation order
struct EdgeLin { double e0, e1, A[6], B[12]; };

__host__ __device__ inline void linearize_xyz(const SE3Pose& P, const double (&R)[9], const Cam& K, const EdgeReg& E, EdgeLin& L)
{
    double x, y, z;
    se3_map(P, E.X, E.Y, E.Z, x, y, z);
    pinhole_error(K, E, x, y, z, L.e0, L.e1);
    const double z_2 = z * z;
    const double tmp[6] = {K.fx, 0.0, -x / z * K.fx, 0.0, K.fy, -y / z * K.fy};
    const double c = -1. / z;
    double S[6];
#pragma unroll
    for (int k = 0; k < 6; k++) S[k] = c * tmp[k];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) L.A[i * 3 + j] = (S[i * 3] * R[j] + S[i * 3 + 1] * R[3 + j]) + S[i * 3 + 2] * R[6 + j];
    L.B[0] = x * y / z_2 * K.fx;
    L.B[1] = -(1 + (x * x / z_2)) * K.fx;
    L.B[2] = y / z * K.fx;
    L.B[3] = -1. / z * K.fx;
    L.B[4] = 0;
    L.B[5] = x / z_2 * K.fx;
    L.B[6] = (1 + y * y / z_2) * K.fy;
    L.B[7] = -x * y / z_2 * K.fy;
    L.B[8] = -x / z * K.fy;
    L.B[9] = 0;
    L.B[10] = -1. / z * K.fy;
    L.B[11] = y / z_2 * K.fy;
}

// BaseBinaryEdge::constructQuadraticForm (base_binary_edge.hpp:55-120) of one linearised edge: `from` is the point (never fixed),
// `to` the pose.  The point's D (3 x 3 row-major) and b3 take the edge's terms; with a free pose Bp (its 6 x 3 block of Hpl,
// row-major: _hessianRowMajor is true, the point being vertex 0) takes B^T W A (robust) or B^T (A^T Omega)^T, and the pose's own
// terms are handed back: Hterm (the 21 upper entries of (B^T W) B) and bterm.  The robust weight enters as rho[1] only
__host__ __device__ inline void quadratic_form(const EdgeReg& E, const EdgeLin& L, bool robust, double delta, double delta2, bool poseFixed,
                                               double (&D)[9], double (&b3)[3], double (&Bp)[18], double (&Hterm)[21], double (&bterm)[6])
{
    // omega_r = - omega * _error: the unary minus binds to omega
    double r0 = (-E.w00) * L.e0 + (-E.w01) * L.e1, r1 = (-E.w10) * L.e0 + (-E.w11) * L.e1;
    double W00 = E.w00, W01 = E.w01, W10 = E.w10, W11 = E.w11;
    if (robust) {
        double cost, weight;
        huber(edge_chi2(E, L.e0, L.e1), delta, delta2, cost, weight);
        W00 = weight * E.w00; W01 = weight * E.w01; W10 = weight * E.w10; W11 = weight * E.w11;
        r0 = r0 * weight; r1 = r1 * weight;
    }
    double AtW[6];
#pragma unroll
    for (int i = 0; i < 3; i++) { AtW[i * 2] = L.A[i] * W00 + L.A[3 + i] * W10; AtW[i * 2 + 1] = L.A[i] * W01 + L.A[3 + i] * W11; }
#pragma unroll
    for (int i = 0; i < 3; i++) b3[i] = b3[i] + (L.A[i] * r0 + L.A[3 + i] * r1);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D[i * 3 + j] = D[i * 3 + j] + (AtW[i * 2] * L.A[j] + AtW[i * 2 + 1] * L.A[3 + j]);
    if (poseFixed) return;
    double BtW[12];
#pragma unroll
    for (int i = 0; i < 6; i++) { BtW[i * 2] = L.B[i] * W00 + L.B[6 + i] * W10; BtW[i * 2 + 1] = L.B[i] * W01 + L.B[6 + i] * W11; }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            Bp[i * 3 + j] = Bp[i * 3 + j] + (robust ? (BtW[i * 2] * L.A[j] + BtW[i * 2 + 1] * L.A[3 + j]) : (L.B[i] * AtW[j * 2] + L.B[6 + i] * AtW[j * 2 + 1]));
#pragma unroll
    for (int i = 0; i < 6; i++) bterm[i] = L.B[i] * r0 + L.B[6 + i] * r1;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) Hterm[upper_index(i, j)] = BtW[i * 2] * L.B[j] + BtW[i * 2 + 1] * L.B[6 + j];
}

// ---- Eigen's 3 x 3 inverse (compute_inverse_size3_helper): the cofactors, the determinant from the first column, one reciprocal
__host__ __device__ __forceinline__ void inverse3(const double (&M)[9], double (&out)[9])
{
    const double c00 = M[4] * M[8] - M[5] * M[7], c10 = M[7] * M[2] - M[8] * M[1], c20 = M[1] * M[5] - M[2] * M[4];
    const double det = (c00 * M[0] + c10 * M[3]) + c20 * M[6];
    const double invdet = 1.0 / det;
    out[0] = c00 * invdet; out[1] = c10 * invdet; out[2] = c20 * invdet;
    out[3] = (M[5] * M[6] - M[3] * M[8]) * invdet;   // cofactor (0, 1)
    out[4] = (M[8] * M[0] - M[6] * M[2]) * invdet;   // cofactor (1, 1)
    out[5] = (M[2] * M[3] - M[0] * M[5]) * invdet;   // cofactor (2, 1)
    out[6] = (M[3] * M[7] - M[4] * M[6]) * invdet;   // cofactor (0, 2)
    out[7] = (M[6] * M[1] - M[7] * M[0]) * invdet;   // cofactor (1, 2)
    out[8] = (M[0] * M[4] - M[1] * M[3]) * invdet;   // cofactor (2, 2)
}

// ---- one landmark of BlockSolver::solve's marginalisation (block_solver.hpp:385-436) behind setLambda (:586-591): Dinv of the
// damped block, db = Dinv * db, and per free pose BDinv = Bi * Dinv, the term of Bb += Bi * db (Cterm, pose * 6 + i) and the terms
// of Hschur(i1, i2) -= BDinv * Bj^T for i2 >= i1 (Sterm: [0, 21) block (0, 0) upper, [21, 57) block (0, 1) full row-major,
// [57, 78) block (1, 1) upper).  Bp0 / Bp1: the point's 6 x 3 blocks.  Entries of a fixed pose are left untouched
constexpr int kS01 = 21, kS11 = 57, kSchurTerms = 78;

__host__ __device__ inline void schur_point(const double (&D)[9], const double (&b3)[3], const double (&Bp0)[18], const double (&Bp1)[18], bool fixed0,
                                            bool fixed1, double lambda, double (&Dinv)[9], double (&Cterm)[12], double (&Sterm)[kSchurTerms])
{
    double Dl[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Dl[i] = D[i];
    Dl[0] = Dl[0] + lambda; Dl[4] = Dl[4] + lambda; Dl[8] = Dl[8] + lambda;
    inverse3(Dl, Dinv);
    double db[3];
#pragma unroll
    for (int i = 0; i < 3; i++) db[i] = (Dinv[i * 3] * b3[0] + Dinv[i * 3 + 1] * b3[1]) + Dinv[i * 3 + 2] * b3[2];
    double BD0[18], BD1[18];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            BD0[i * 3 + j] = (Bp0[i * 3] * Dinv[j] + Bp0[i * 3 + 1] * Dinv[3 + j]) + Bp0[i * 3 + 2] * Dinv[6 + j];
            BD1[i * 3 + j] = (Bp1[i * 3] * Dinv[j] + Bp1[i * 3 + 1] * Dinv[3 + j]) + Bp1[i * 3 + 2] * Dinv[6 + j];
        }
    if (!fixed0) {
#pragma unroll
        for (int i = 0; i < 6; i++) Cterm[i] = (Bp0[i * 3] * db[0] + Bp0[i * 3 + 1] * db[1]) + Bp0[i * 3 + 2] * db[2];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) Sterm[upper_index(i, j)] = (BD0[i * 3] * Bp0[j * 3] + BD0[i * 3 + 1] * Bp0[j * 3 + 1]) + BD0[i * 3 + 2] * Bp0[j * 3 + 2];
        if (!fixed1) {
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) Sterm[kS01 + i * 6 + j] = (BD0[i * 3] * Bp1[j * 3] + BD0[i * 3 + 1] * Bp1[j * 3 + 1]) + BD0[i * 3 + 2] * Bp1[j * 3 + 2];
        }
    }
    if (!fixed1) {
#pragma unroll
        for (int i = 0; i < 6; i++) Cterm[6 + i] = (Bp1[i * 3] * db[0] + Bp1[i * 3 + 1] * db[1]) + Bp1[i * 3 + 2] * db[2];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) Sterm[kS11 + upper_index(i, j)] = (BD1[i * 3] * Bp1[j * 3] + BD1[i * 3 + 1] * Bp1[j * 3 + 1]) + BD1[i * 3 + 2] * Bp1[j * 3 + 2];
    }
}

// ---- one landmark of the back-substitution (:463-486): cl = bl - Bt * xp (rightMultiply with cp = -xp, pose by pose), xl = Dinv *
// cl into zeroed memory.  xp0 / xp1: the steps of pose 0 and pose 1 (a fixed pose's is not read)
__host__ __device__ inline void back_substitute(const double (&b3)[3], const double (&Bp0)[18], const double (&Bp1)[18], bool fixed0, bool fixed1,
                                                const double* xp0, const double* xp1, const double (&Dinv)[9], double (&xl)[3])
{
    double cl[3] = {b3[0], b3[1], b3[2]};
    if (!fixed0) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double dot = Bp0[j] * -xp0[0];
#pragma unroll
            for (int i = 1; i < 6; i++) dot = dot + Bp0[i * 3 + j] * -xp0[i];
            cl[j] = cl[j] + dot;
        }
    }
    if (!fixed1) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double dot = Bp1[j] * -xp1[0];
#pragma unroll
            for (int i = 1; i < 6; i++) dot = dot + Bp1[i * 3 + j] * -xp1[i];
            cl[j] = cl[j] + dot;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) xl[j] = 0.0 + ((Dinv[j * 3] * cl[0] + Dinv[j * 3 + 1] * cl[1]) + Dinv[j * 3 + 2] * cl[2]);
}

// ---- THE REDUCED SOLVE (a DEFINED CHOICE where g2o runs SimplicialLDLT behind an ordering): an unpivoted LDLt in the
// poses' natural order.  M: n x n row-major (n <= 12), its LOWER triangle holds the matrix -- entry (r, c), c <= r, is Hschur's
// (c, r) -- and is overwritten by L (unit diagonal implied) with D on the diagonal.  Row by row, every dot product left to right
// from its first product.  Fails (false, x unwritten) on a pivot that is zero or not finite.  w, y: 12 words each
__host__ __device__ __noinline__ bool ldlt_plain(int n, double* M, const double* rhs, double* x, double* w, double* y)
{
    for (int r = 0; r < n; r++) {
        for (int c = 0; c < r; c++) {
            double t = M[r * n + c];
            if (c > 0) {
                double dot = w[0] * M[c * n];
                for (int k = 1; k < c; k++) dot = dot + w[k] * M[c * n + k];
                t = t - dot;
            }
            w[c] = t;
        }
        for (int c = 0; c < r; c++) M[r * n + c] = w[c] / M[c * n + c];
        double d = M[r * n + r];
        if (r > 0) {
            double dot = w[0] * M[r * n];
            for (int c = 1; c < r; c++) dot = dot + w[c] * M[r * n + c];
            d = d - dot;
        }
        if (!(d - d == 0.0) || d == 0.0) return false;
        M[r * n + r] = d;
    }
    for (int r = 0; r < n; r++) {
        double t = rhs[r];
        if (r > 0) {
            double dot = M[r * n] * y[0];
            for (int k = 1; k < r; k++) dot = dot + M[r * n + k] * y[k];
            t = t - dot;
        }
        y[r] = t;
    }
    for (int r = 0; r < n; r++) y[r] = y[r] / M[r * n + r];
    for (int r = n - 2; r >= 0; r--) {
        double dot = M[(r + 1) * n + r] * y[r + 1];
        for (int k = r + 2; k < n; k++) dot = dot + M[k * n + r] * y[k];
        y[r] = y[r] - dot;
    }
    for (int r = 0; r < n; r++) x[r] = y[r];
    return true;
}

// the reduced system from the summed Schur blocks S (schur_point's layout) and bschur = bp - coeff, into M's lower triangle.
// nFree poses, the first free one being pose f0
__host__ __device__ inline void assemble_reduced(const double* S, const double* bp, const double* coeff, int nFree, int f0, double* M, double* bs)
{
    const int n = 6 * nFree;
    for (int i = 0; i < n * n; i++) M[i] = 0.0;
    for (int a = 0; a < nFree; a++) {
        const int s = a == 0 ? f0 : 1;
        for (int i = 0; i < 6; i++) {
            bs[6 * a + i] = bp[6 * s + i] - coeff[6 * s + i];
            for (int j = i; j < 6; j++) M[(6 * a + j) * n + (6 * a + i)] = S[(s ? kS11 : 0) + upper_index(i, j)];
        }
    }
    if (nFree == 2)
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) M[(6 + j) * n + i] = S[kS01 + i * 6 + j];
}

// ---- OptimizationAlgorithmLevenberg over the full system, one wave a problem (optimization_algorithm_levenberg.cpp:61-180 with
// computeLambdaInit's maximum over the poses' AND the points' diagonals, computeScale over all dimensions, setLambda on both block
// families, and a rejected trial restoring every vertex).  Lambda, the poses and the rest of the state are wave-uniform and
// computed redundantly by every lane; the reduced solve runs on lane 0 in LDS and the poses' step is read back by all.
struct BaShared { double Hpp[42], bp[12], S[kSchurTerms], coeff[12], M[144], B[12], X[12], W[12], Y[12]; int ok; };

// x: the poses' step (the free poses in their order), ZERO before any solve and kept when a solve fails -- the points' steps, which
// follow the same rule, live with the kernel
struct BaState {
    double lambda = 0., growth = 2.;
    int flatSteps = 0;
    double x[12] = {};
};

struct BaRun { int iterations, trials, stop; double chiFirst, chiLast; };
constexpr int kStopIterations = 0, kStopTrials = 1, kStopRhoZero = 2, kStopFlat = 3;

// One optimize(maxIt) call, maxIt <= kBaIterations.  The calling kernel's Problem supplies, every sum closed by THE SUMMATION TREE
// over its points:
//   fixed0, fixed1                  which pose is fixed (not both)
//   chi2(candidate)                 computeActiveErrors + activeRobustChi2 at the estimates (false) or at the trial's candidates (true:
//                                   the free poses moved by x, every point by its kept step)
//   build(Hpp, bp, diagMax)         buildSystem at the estimates: the points' blocks stored, the free poses' upper triangles
//                                   (pose * 21 + upper_index) and b (pose * 6 + i) summed, the maximum over the POINTS' diagonals
//   marginalise(lambda, S, coeff)   the Schur pass: every point's Dinv stored, the 78 Schur terms and `coefficients` summed as p - term
//                                   and p + term (S comes back WITHOUT its start)
//   back_substitute(x)              every point's step from the poses' (called only behind a successful solve)
//   move_poses(x)                   the candidates of the free poses
//   scale_points(lambda)            computeScale's landmark part at the kept steps
//   accept()                        the candidates become the estimates
// All 64 lanes call it together: it holds __syncthreads().
template <class Problem>
__device__ __forceinline__ BaRun levenberg_full(Problem& p, BaShared& sh, BaState& st, int maxIt, int lane)
{
    BaRun run = {0, 0, kStopIterations, 0.0, 0.0};
    const int nFree = (p.fixed0 ? 0 : 1) + (p.fixed1 ? 0 : 1), f0 = p.fixed0 ? 1 : 0, n = 6 * nFree;
    for (int it = 0; it < kBaIterations; it++) {
        if (it >= maxIt) break;
        run.iterations++;
        double chiNow = p.chi2(false);
        const double chiStart = chiNow;
        if (it == 0) run.chiFirst = chiNow;
        double pointMax;
        {
            // the poses' blocks go to LDS at once: lane 0 assembles every trial's reduced system from them, and a lane's registers
            // are the Schur pass's
            double Hpp[42], bp[12];
            p.build(Hpp, bp, pointMax);
            if (it == 0) {
                double poseMax = 0.;
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    if (s == 0 ? p.fixed0 : p.fixed1) continue;
#pragma unroll
                    for (int j = 0; j < 6; j++) poseMax = max_of(fabs(Hpp[21 * s + upper_index(j, j)]), poseMax);
                }
                st.lambda = 1e-5 * max_of(pointMax, poseMax);
                st.growth = 2;
                st.flatSteps = 0;
            }
            __syncthreads();   // (the last iteration's reads of sh.bp are done)
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 42; i++) sh.Hpp[i] = Hpp[i];
#pragma unroll
                for (int i = 0; i < 12; i++) sh.bp[i] = bp[i];
            }
            __syncthreads();
        }
        double gain = 0;
        int nTried = 0;
        for (int t = 0; t < kTrials; t++) {
            {
                double S[kSchurTerms], coeff[12];
                p.marginalise(st.lambda, S, coeff);
                __syncthreads();   // (the last trial's reads of sh.X / sh.ok are done)
                if (lane == 0) {
                    // _Hschur->clear(); _Hpp->add(_Hschur): zero plus the damped block, then the summed updates
#pragma unroll
                    for (int i = 0; i < 36; i++) sh.S[kS01 + i] = 0.0 + S[kS01 + i];
#pragma unroll
                    for (int s = 0; s < 2; s++)
#pragma unroll
                        for (int i = 0; i < 6; i++)
#pragma unroll
                            for (int j = i; j < 6; j++) {
                                const double h = sh.Hpp[21 * s + upper_index(i, j)];
                                sh.S[(s ? kS11 : 0) + upper_index(i, j)] = (0.0 + (i == j ? h + st.lambda : h)) + S[(s ? kS11 : 0) + upper_index(i, j)];
                            }
#pragma unroll
                    for (int i = 0; i < 12; i++) sh.coeff[i] = coeff[i];
                }
            }
            if (lane == 0) {
                assemble_reduced(sh.S, sh.bp, sh.coeff, nFree, f0, sh.M, sh.B);
                sh.ok = ldlt_plain(n, sh.M, sh.B, sh.X, sh.W, sh.Y) ? 1 : 0;
            }
            __syncthreads();
            const bool solved = sh.ok != 0;
            if (solved) {
#pragma unroll
                for (int r = 0; r < 12; r++) st.x[r] = r < n ? sh.X[r] : st.x[r];
                p.back_substitute(st.x);
            }
            p.move_poses(st.x);
            double chiTrial = p.chi2(true);
            if (!solved) chiTrial = 1.7976931348623157e308;
            gain = (chiNow - chiTrial);
            double poseScale = 0.;
#pragma unroll
            for (int s = 0; s < 2; s++) {
                if (s == 0 ? p.fixed0 : p.fixed1) continue;
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const double xj = (s == 0 || p.fixed0) ? st.x[j] : st.x[6 + j];
                    poseScale += xj * (st.lambda * xj + sh.bp[6 * s + j]);
                }
            }
            double scale = poseScale + p.scale_points(st.lambda);
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
                p.accept();
            } else {
                st.lambda = st.lambda * st.growth;   // (the full system's own run of the algorithm: orbg::levenberg's is over one N-dof vertex)
                st.growth *= 2;
            }
            nTried++;
            if (!(gain < 0)) break;
        }
        run.trials += nTried;
        run.chiLast = chiNow;
        if (nTried == kTrials) { run.stop = kStopTrials; break; }
        if (gain == 0) { run.stop = kStopRhoZero; break; }
        if ((chiStart - chiNow) * 1e3 < chiStart) st.flatSteps++;
        else st.flatSteps = 0;
        if (st.flatSteps >= 3) { run.stop = kStopFlat; break; }
    }
    return run;
}

}  // namespace orbg
