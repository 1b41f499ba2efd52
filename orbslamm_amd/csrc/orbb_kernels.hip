// orbb_kernels.hip -- the device initial map (part of orbslamm_hip.hip; host side: orbb_host.inc, ABI:
// include/orbslamm_initmap.h): Tracking::CreateInitialMapMonocular from its bundle adjustment on
// (src/Tracking.cc:728-758) -- Optimizer::BundleAdjustment (src/Optimizer.cc:68-260) over two keyframes and the points they
// share, ComputeSceneMedianDepth(2), the verdict and the rescaling -- for any number of maps in ONE launch.  One wave owns a
// problem from its compaction to its result: point k is lane k % 64's, always; a lane keeps its partial sums in registers (the Schur pass's in its LDS column) and
// every sum is closed by the xor butterfly 32, 16, ..., 1 -- THE SUMMATION TREE of §8o over points, a function of the point count
// alone.  This file keeps what is the initial map's own: the records, the compaction of mvIniMatches into the point list (ballot
// + prefix, in feature order), the four passes over the points (chi2, buildSystem, the Schur pass, the back-substitution), the
// recovery with UpdateNormalAndDepth, the median by a bit search, the verdict and the rescaling.  The edge, the 3 x 3 inverse, a
// landmark's Schur share, the reduced LDLt and the Levenberg run over the full system are orbg_schur.hip's; SE3Quat's oplus and
// Converter::toSE3Quat are orbo_kernels.hip's.
// Binary64 throughout, built with -ffp-contract=off, no atomics; every loop is bounded (20 iterations, 10 trials, a problem's
// points), so no input can make the kernel spin.
// THE ACCUMULATORS.  The Schur pass carries 78 + 12 binary64 partials a lane beside a point's working set (its 9 + 3 + 36 stored
// words, Dinv, the 18 + 18 of BDinv): in registers they spill.  They are LDS PARTIALS: partial i of lane l at sPart[i * 64 + l]
// (46 080 bytes a workgroup, which is one wave; a lane touches its own column alone, so nothing is synchronised and the 64 lanes
// of an access fall on consecutive words), read back once at the end for the butterfly.  buildSystem's 42 + 12 + 1 stay in
// registers.  The resource figures are in DESIGN.md §8aa; a blocked accumulation (pose 0's 63 sums, then pose 1's 27) is the
// alternative, and nobody has measured which is faster.
// A point's stored words (estimate, kept step, D, b, the two blocks of Hpl, Dinv) live in a per-call scratch block in global
// memory, field-major (word f of slot s at f * total + s: a wave's loads are contiguous), written and read by the point's own lane;
// the compaction's words, written by the lane that holds the feature, are read behind a workgroup barrier.
#pragma once

namespace orbb {

constexpr int kLanes = 64;
constexpr int kMaxFeatures = 65535;           // ORBB_MAX_FEATURES
constexpr int kMaxProblems = 256;             // ORBB_MAX_PROBLEMS
constexpr int kMaxCallFeatures = 1 << 18;     // ORBB_MAX_CALL_FEATURES
constexpr double kDelta = (double)2.44744754f, kDelta2 = kDelta * kDelta;   // the Huber width: (float)sqrt(5.99), widened (Optimizer.cc:106)
// a slot's words in the scratch block
constexpr int kPartials = orbg::kSchurTerms + 12;   // the Schur pass's sums a lane
constexpr int F_X = 0, F_XL = 3, F_D = 6, F_BL = 15, F_BP = 18, F_DINV = 54, kSlotWords = 63;

struct ProbIn {
    float Tcw[2][12];
    float K[4];
    int32_t fixed0, fixed1, iterations, robust, n1, n2;
    const orbm::KeyDev* keys1;   // mvKeysUn of the initial and of the current frame: a device-resident frame's, or the call's upload
    const orbm::KeyDev* keys2;
    int32_t off, pad;            // the problem's first feature among the call's: its matches, positions, point records and slots start there
};
struct Args {
    const ProbIn* probs;
    const int32_t* matches;      // per feature of the initial frames
    const float* p3d;            // 3 per feature
    OrbbResult* out;
    OrbbPoint* pts;              // per feature, zeroed before the launch
    double* scr;                 // kSlotWords * total, field-major
    float4* ob;                  // 2 * total: a point's observation in keyframe 0 (at slot) and 1 (at total + slot): u, v, invSigma2
    int32_t* feat;               // per slot: the point's feature in the initial frame
    int32_t* lvl;                // per slot: the octave of its feature in the current frame
    float* depth;                // per slot
    int32_t total, nlevels;
    float invSigma2[ORBX_MAX_LEVELS], sf[ORBX_MAX_LEVELS];
};

using orbg::Cam;
using orbg::EdgeReg;
using orbg::SE3Pose;
using orbg::nan_canon;
using orbg::wave_sum;

__device__ __forceinline__ float canon_f(float f) { return f != f ? __builtin_bit_cast(float, 0xFFC00000u) : f; }

// one problem at its estimates (est) and its trial's candidates (cand), with what the passes need to reach its points
struct Problem {
    const Args& a;
    int off, n, lane;
    const Cam& K;
    bool robust, fixed0, fixed1;
    SE3Pose (&est)[2];
    SE3Pose cand[2];
    double* part;   // the Schur pass's LDS partials: kPartials columns of 64

    __device__ __forceinline__ double* word(int f, int k) const { return a.scr + (size_t)f * a.total + (off + k); }
    __device__ __forceinline__ EdgeReg edge(int s, int k, const double (&X)[3]) const
    {
        EdgeReg E = orbg::load_edge(make_float4(0.f, 0.f, 0.f, a.ob[(size_t)s * a.total + off + k].z),
                                    make_float2(a.ob[(size_t)s * a.total + off + k].x, a.ob[(size_t)s * a.total + off + k].y));
        E.X = X[0]; E.Y = X[1]; E.Z = X[2];
        return E;
    }

    // computeActiveErrors + activeRobustChi2: point by point, pose 0's edge first
    __device__ __forceinline__ double chi2(bool candidate) const
    {
        const SE3Pose P0 = candidate ? cand[0] : est[0], P1 = candidate ? cand[1] : est[1];
        double part = 0.0;
        for (int k = lane; k < n; k += kLanes) {
            double X[3];
#pragma unroll
            for (int c = 0; c < 3; c++) X[c] = *word(F_X + c, k);
            if (candidate) {
#pragma unroll
                for (int c = 0; c < 3; c++) X[c] = X[c] + *word(F_XL + c, k);
            }
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const EdgeReg E = edge(s, k, X);
                double x, y, z, r0, r1;
                orbg::se3_map(s ? P1 : P0, E.X, E.Y, E.Z, x, y, z);
                orbg::pinhole_error(K, E, x, y, z, r0, r1);
                const double c = orbg::edge_chi2(E, r0, r1);
                if (robust) {
                    double cost, weight;
                    orbg::huber(c, kDelta, kDelta2, cost, weight);
                    part = part + cost;
                } else part = part + c;
            }
        }
        return wave_sum(part);
    }

    // buildSystem at the estimates
    __device__ __forceinline__ void build(double (&Hpp)[42], double (&bp)[12], double& pointMax) const
    {
        double R0[9], R1[9];
        orbg::quat_to_matrix(est[0].q, R0);
        orbg::quat_to_matrix(est[1].q, R1);
#pragma unroll
        for (int i = 0; i < 42; i++) Hpp[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 12; i++) bp[i] = 0.0;
        double pm = 0.0;
        for (int k = lane; k < n; k += kLanes) {
            double X[3], D[9], b3[3];
#pragma unroll
            for (int c = 0; c < 3; c++) X[c] = *word(F_X + c, k);
#pragma unroll
            for (int i = 0; i < 9; i++) D[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) b3[i] = 0.0;
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const bool fixed = s ? fixed1 : fixed0;
                const EdgeReg E = edge(s, k, X);
                orbg::EdgeLin L;
                orbg::linearize_xyz(s ? est[1] : est[0], s ? R1 : R0, K, E, L);
                double Bp[18], Hterm[21], bterm[6];
#pragma unroll
                for (int i = 0; i < 18; i++) Bp[i] = 0.0;
                orbg::quadratic_form(E, L, robust, kDelta, kDelta2, fixed, D, b3, Bp, Hterm, bterm);
#pragma unroll
                for (int i = 0; i < 18; i++) *word(F_BP + 18 * s + i, k) = Bp[i];
                if (!fixed) {
#pragma unroll
                    for (int i = 0; i < 6; i++) bp[6 * s + i] = bp[6 * s + i] + bterm[i];
#pragma unroll
                    for (int i = 0; i < 21; i++) Hpp[21 * s + i] = Hpp[21 * s + i] + Hterm[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 9; i++) *word(F_D + i, k) = D[i];
#pragma unroll
            for (int i = 0; i < 3; i++) *word(F_BL + i, k) = b3[i];
#pragma unroll
            for (int j = 0; j < 3; j++) pm = orbg::max_of(fabs(D[4 * j]), pm);
        }
#pragma unroll
        for (int i = 0; i < 42; i++) Hpp[i] = wave_sum(Hpp[i]);
#pragma unroll
        for (int i = 0; i < 12; i++) bp[i] = wave_sum(bp[i]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) pm = orbg::max_of(pm, __shfl_xor(pm, m, kLanes));
        pointMax = __shfl(pm, 0, kLanes);   // (partial 0's: max_of is not symmetric in a NaN)
    }

    // the Schur pass: S and coeff come back as the tree's sums of - term and + term; the partials live in LDS (the file's head)
    __device__ __forceinline__ void marginalise(double lambda, double (&S)[orbg::kSchurTerms], double (&coeff)[12]) const
    {
        double* my = part + lane;   // partial i at my[i * kLanes]: the Schur terms, then `coefficients`
#pragma unroll
        for (int i = 0; i < kPartials; i++) my[i * kLanes] = 0.0;
        for (int k = lane; k < n; k += kLanes) {
            double D[9], b3[3], Bp0[18], Bp1[18], Dinv[9], Cterm[12], Sterm[orbg::kSchurTerms];
#pragma unroll
            for (int i = 0; i < 9; i++) D[i] = *word(F_D + i, k);
#pragma unroll
            for (int i = 0; i < 3; i++) b3[i] = *word(F_BL + i, k);
#pragma unroll
            for (int i = 0; i < 18; i++) { Bp0[i] = *word(F_BP + i, k); Bp1[i] = *word(F_BP + 18 + i, k); }
            orbg::schur_point(D, b3, Bp0, Bp1, fixed0, fixed1, lambda, Dinv, Cterm, Sterm);
#pragma unroll
            for (int i = 0; i < 9; i++) *word(F_DINV + i, k) = Dinv[i];
            if (!fixed0) {
#pragma unroll
                for (int i = 0; i < 6; i++) my[(orbg::kSchurTerms + i) * kLanes] = my[(orbg::kSchurTerms + i) * kLanes] + Cterm[i];
#pragma unroll
                for (int i = 0; i < 21; i++) my[i * kLanes] = my[i * kLanes] - Sterm[i];
                if (!fixed1) {
#pragma unroll
                    for (int i = orbg::kS01; i < orbg::kS11; i++) my[i * kLanes] = my[i * kLanes] - Sterm[i];
                }
            }
            if (!fixed1) {
#pragma unroll
                for (int i = 6; i < 12; i++) my[(orbg::kSchurTerms + i) * kLanes] = my[(orbg::kSchurTerms + i) * kLanes] + Cterm[i];
#pragma unroll
                for (int i = orbg::kS11; i < orbg::kSchurTerms; i++) my[i * kLanes] = my[i * kLanes] - Sterm[i];
            }
        }
#pragma unroll
        for (int i = 0; i < orbg::kSchurTerms; i++) S[i] = wave_sum(my[i * kLanes]);
#pragma unroll
        for (int i = 0; i < 12; i++) coeff[i] = wave_sum(my[(orbg::kSchurTerms + i) * kLanes]);
    }

    __device__ __forceinline__ void back_substitute(const double (&x)[12]) const
    {
        double xp0[6], xp1[6];   // the steps of pose 0 and of pose 1 (the second six words when both are free)
#pragma unroll
        for (int i = 0; i < 6; i++) { xp0[i] = x[i]; xp1[i] = fixed0 ? x[i] : x[6 + i]; }
        for (int k = lane; k < n; k += kLanes) {
            double b3[3], Bp0[18], Bp1[18], Dinv[9], xl[3];
#pragma unroll
            for (int i = 0; i < 3; i++) b3[i] = *word(F_BL + i, k);
#pragma unroll
            for (int i = 0; i < 18; i++) { Bp0[i] = *word(F_BP + i, k); Bp1[i] = *word(F_BP + 18 + i, k); }
#pragma unroll
            for (int i = 0; i < 9; i++) Dinv[i] = *word(F_DINV + i, k);
            orbg::back_substitute(b3, Bp0, Bp1, fixed0, fixed1, xp0, xp1, Dinv, xl);
#pragma unroll
            for (int c = 0; c < 3; c++) *word(F_XL + c, k) = xl[c];
        }
    }

    // oplusImpl of the free poses: exp(dx) * estimate
    __device__ __forceinline__ void move_poses(const double (&x)[12])
    {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            cand[s] = est[s];
            if (s ? fixed1 : fixed0) continue;
            const int o = (s == 0 || fixed0) ? 0 : 6;
            const orbo::Pose P = {est[s].q, est[s].tx, est[s].ty, est[s].tz};
            const orbo::Pose Q = orbo::oplus(P, x[o], x[o + 1], x[o + 2], x[o + 3], x[o + 4], x[o + 5]);
            cand[s].q = Q.q; cand[s].tx = Q.tx; cand[s].ty = Q.ty; cand[s].tz = Q.tz;
        }
    }

    // computeScale's landmark part at the kept steps
    __device__ __forceinline__ double scale_points(double lambda) const
    {
        double part = 0.0;
        for (int k = lane; k < n; k += kLanes) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double xj = *word(F_XL + j, k);
                part = part + xj * (lambda * xj + *word(F_BL + j, k));
            }
        }
        return wave_sum(part);
    }

    __device__ __forceinline__ void accept()
    {
        est[0] = cand[0]; est[1] = cand[1];
        for (int k = lane; k < n; k += kLanes) {
#pragma unroll
            for (int c = 0; c < 3; c++) *word(F_X + c, k) = *word(F_X + c, k) + *word(F_XL + c, k);
        }
    }
};

// Converter::toCvMat(SE3Quat) narrowed, the rows above the last
__device__ __forceinline__ void pose_rows(const SE3Pose& P, float* T)
{
    double R[9];
    orbg::quat_to_matrix(P.q, R);
    T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2]; T[3] = (float)P.tx;
    T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5]; T[7] = (float)P.ty;
    T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8]; T[11] = (float)P.tz;
}

// a float's bits as an unsigned key that orders as the float does
__device__ __forceinline__ uint32_t depth_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kLanes) void k_initial_map(Args a, int nProblems)
{
    __shared__ orbg::BaShared sBa;
    __shared__ double sPart[kPartials * kLanes];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= nProblems) return;
    const ProbIn& in = a.probs[p];
    const int off = in.off, n1 = in.n1;
    // ---- the point list (Tracking.cc:694-708): the matched features of the initial frame in ascending index, by ballot + prefix
    int n = 0;
    bool bad = false;
    for (int base = 0; base < n1; base += kLanes) {
        const int i = base + lane;
        const int m = i < n1 ? a.matches[off + i] : -1;
        const bool has = m >= 0 && m < in.n2;   // (the host has refused what lies outside the current frame)
        const unsigned long long mask = __ballot(has);
        if (has) {
            const int slot = off + n + __popcll(mask & ((1ull << lane) - 1ull));
            const orbm::KeyDev k1 = in.keys1[i], k2 = in.keys2[m];
            const bool ok1 = k1.octave >= 0 && k1.octave < a.nlevels, ok2 = k2.octave >= 0 && k2.octave < a.nlevels;
            bad |= !ok1 || !ok2 || !(k1.x - k1.x == 0.f) || !(k1.y - k1.y == 0.f) || !(k2.x - k2.x == 0.f) || !(k2.y - k2.y == 0.f);
            a.ob[slot] = make_float4(k1.x, k1.y, ok1 ? a.invSigma2[k1.octave] : 0.f, 0.f);
            a.ob[(size_t)a.total + slot] = make_float4(k2.x, k2.y, ok2 ? a.invSigma2[k2.octave] : 0.f, 0.f);
            a.feat[slot] = i;
            a.lvl[slot] = ok2 ? k2.octave : 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                a.scr[(size_t)(F_X + c) * a.total + slot] = (double)a.p3d[3 * (size_t)(off + i) + c];   // Converter::toVector3d
                a.scr[(size_t)(F_XL + c) * a.total + slot] = 0.0;                                        // the solver's x: zero before any solve
            }
        }
        n += __popcll(mask);
    }
    __syncthreads();   // (a slot is read by lane slot % 64 from here on)
    OrbbResult* out = a.out + p;
    if (__any(bad)) {
        if (lane == 0) out->verdict = -1;   // a key on the device is out of range or not finite: the host refuses the call
        return;
    }

    const Cam K = {(double)in.K[0], (double)in.K[1], (double)in.K[2], (double)in.K[3]};
    SE3Pose est[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const orbo::Pose P = orbo::pose_of_tcw(in.Tcw[s]);   // (reads the twelve words of the rows above the last)
        est[s].q = P.q; est[s].tx = P.tx; est[s].ty = P.ty; est[s].tz = P.tz;
    }
    Problem pr = {a, off, n, lane, K, in.robust != 0, in.fixed0 != 0, in.fixed1 != 0, est, {est[0], est[1]}, sPart};
    orbg::BaState st;
    // optimize(nIterations): with no point there is no edge and no vertex to optimise
    const orbg::BaRun run = orbg::levenberg_full(pr, sBa, st, n > 0 ? in.iterations : 0, lane);

    // ---- the recovery (Optimizer.cc:214-258): the poses, their centres as KeyFrame::SetPose forms them, then every point
    float T1[12], T2[12], Ow1[3], Ow2[3];
    pose_rows(est[0], T1);
    pose_rows(est[1], T2);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        Ow1[i] = cvm::gemm3_elem(T1[i], T1[4 + i], T1[8 + i], T1[3], T1[7], T1[11], -1.0, 0.f, 0.0);
        Ow2[i] = cvm::gemm3_elem(T2[i], T2[4 + i], T2[8 + i], T2[3], T2[7], T2[11], -1.0, 0.f, 0.0);
    }
    bool finite = true;
    for (int k = lane; k < n; k += kLanes) {
        OrbbPoint& pt = a.pts[off + a.feat[off + k]];
        float P[3], normal[3], t0[3], t1[3], pc[3];
#pragma unroll
        for (int c = 0; c < 3; c++) P[c] = (float)*pr.word(F_X + c, k);
        // UpdateNormalAndDepth (MapPoint.cc:330-371) over the initial keyframe, then the current one; the reference keyframe is the current
#pragma unroll
        for (int c = 0; c < 3; c++) { t0[c] = P[c] - Ow1[c]; t1[c] = P[c] - Ow2[c]; pc[c] = t1[c]; }
        const float a0 = (float)(1. / cvm::norm3(t0)), a1 = (float)(1. / cvm::norm3(t1));
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float u0 = t0[c] * a0, u1 = t1[c] * a1;
            float s = u0 + 0.f;
            s = u1 + s;
            normal[c] = cvm::expr_scale(s, 1. / 2);
        }
        const float dist = (float)cvm::norm3(pc);
        const float maxD = dist * a.sf[a.lvl[off + k]];
        const float minD = maxD / a.sf[a.nlevels - 1];
        // KeyFrame.cc:695-705 with the adjusted pose of the initial keyframe: the dot in double, zcw widened, the sum narrowed
        double dot = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) dot += (double)T1[8 + c] * (double)P[c];
        const float z = (float)(dot + (double)T1[11]);
        if (!(z - z == 0.f)) finite = false;
        a.depth[off + k] = z;
#pragma unroll
        for (int c = 0; c < 3; c++) { pt.pos[c] = canon_f(P[c]); pt.normal[c] = canon_f(normal[c]); }
        pt.min_distance = canon_f(minD); pt.max_distance = canon_f(maxD);
        pt.status = 1;   // ORBR_ST_DONE
        pt.matched = 1;
    }
    finite = !__any(!finite);
    __syncthreads();   // (the depths are read by every lane)

    // ---- Tracking.cc:731-734: the element of rank (n - 1) / 2 of the sorted depths, found bit by bit over the ordered keys
    float median = __builtin_bit_cast(float, 0xFFC00000u), inv = median;
    int verdict = 3;   // ORBB_RESET_NONFINITE
    if (finite) {
        median = 0.f;   // DEFINED: no point
        if (n > 0) {
            const int rank = (n - 1) / 2;
            uint32_t prefix = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const uint32_t trial = prefix | (1u << bit);
                int below = 0;
                for (int k = lane; k < n; k += kLanes) below += depth_key(a.depth[off + k]) < trial ? 1 : 0;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) below += __shfl_xor(below, m, kLanes);
                if (below <= rank) prefix = trial;
            }
            median = __uint_as_float((prefix & 0x80000000u) ? (prefix & 0x7FFFFFFFu) : ~prefix) + 0.f;
        }
        inv = 1.0f / median;
        verdict = median < 0 ? 1 : n < 90 ? 2 : 0;
    }
    // ---- Tracking.cc:745-757: cv::Mat * float, alpha the float widened
    const bool rescale = verdict == 0;
    for (int k = lane; k < n; k += kLanes) {
        OrbbPoint& pt = a.pts[off + a.feat[off + k]];
#pragma unroll
        for (int c = 0; c < 3; c++) pt.pos_scaled[c] = rescale ? canon_f(cvm::expr_scale(pt.pos[c], (double)inv)) : pt.pos[c];
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            out->Tcw1[i] = canon_f(T1[i]); out->Tcw2[i] = canon_f(T2[i]);
            out->Tcw2_scaled[i] = canon_f((rescale && i % 4 == 3) ? cvm::expr_scale(T2[i], (double)inv) : T2[i]);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) { out->Ow1[i] = canon_f(Ow1[i]); out->Ow2[i] = canon_f(Ow2[i]); }
        out->median_depth = canon_f(median); out->inv_median_depth = canon_f(inv);
        out->n_points = n; out->verdict = verdict;
        out->iterations = run.iterations; out->trials = run.trials; out->stop = run.stop; out->pad = 0;
        out->chi2_first = nan_canon(run.chiFirst); out->chi2_last = nan_canon(run.chiLast); out->lambda = nan_canon(st.lambda);
    }
}

}  // namespace orbb
