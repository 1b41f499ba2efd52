// orbl_kernels.hip -- the device CreateNewMapPoints (LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:207-452 of both
// scenarios, monocular).  Part of the library's one translation unit (orbslamm_hip.hip); host side:
// orbl_host.inc.
//
// One call is one chain on the matcher handle's stream and one copy down:
//   k_newpoints_search    SearchForTriangulation (ORBmatcher.cc:659-825) of the current keyframe against EVERY neighbour:
//                         workgroups (x: a (neighbour, shared vocabulary node), y: a share of the node's queries), four
//                         waves each; the queries of a node are dealt out over gridDim.y * 4 waves, a wave scans the
//                         neighbour's features of the node for each of its queries (k_triangulation_pairs' arithmetic
//                         and tie-break: dist <= bestDist, the last one wins).  The scan is a chain of dependent gathers
//                         (index -> flag, descriptor, key): it is latency, hidden only by waves, so the host sizes
//                         gridDim.y to put a few thousand waves in flight whatever the vocabulary's node size.  No
//                         orientation histogram (the reference builds ORBmatcher(0.6, false)), so every (neighbour,
//                         query) is independent of every other.
//   k_newpoints_triangulate   one lane per (neighbour, query): the rays and their parallax, the 4x4 A and its
//                         JacobiSVDImpl_<float> on arrays in LDS (cvm::jacobi_svd), x3D, the five gates, and what
//                         MapPoint::UpdateNormalAndDepth leaves for a point with these two observations; a status byte and
//                         a record slot
//   k_newpoints_resolve   one lane per query: the serial loop's AddMapPoint(pMP, idx1) -- the first neighbour that
//                         accepted the query keeps it, every later neighbour reads "feature skipped"
//   k_newpoints_count / k_newpoints_compact   one workgroup per neighbour: the accepted records of its row counted, then
//                         written behind the earlier rows' in idx1 order (the reference's order).  Integers, no atomics.
// Arithmetic: one IEEE operation per source operation (the library is built with -ffp-contract=off); OpenCV's pieces are
// orbx_cvmath.hpp's.
// Below them: k_fuse_batch, the searches of LocalMapping::SearchInNeighbors' Fuse calls for all targets in one launch (§8l),
// on the shared Fuse pieces of orbf_kernels.hip (§8n).
#pragma once

namespace orbl {

constexpr int kMaxNeighbours = 32;
constexpr int kSearchWaves = 4;
constexpr int kSearchThreads = 64 * kSearchWaves;
constexpr int kSearchWavesWanted = 8192;   // waves in flight that hide the scan's gathers (8 a SIMD)
constexpr int kSearchMaxShares = 64;
constexpr int kTriThreads = 64;
constexpr int kRowThreads = 256;

// the status codes of include/orbslamm_hip.h (ORBL_ST_*)
enum : uint8_t { ST_NEIGHBOUR = 0, ST_FEATURE, ST_NO_MATCH, ST_PARALLAX, ST_X3D_ZERO, ST_Z1, ST_Z2, ST_REPROJ1, ST_REPROJ2, ST_DIST_ZERO, ST_SCALE, ST_ACCEPTED };

// one keyframe's side in HBM; F, ex, ey, gated: of a neighbour against the current keyframe
struct KfDev {
    const orbm::KeyDev* keys; const uint8_t* desc; const int32_t* fvStart; const int32_t* fvIdx; const uint8_t* skip;
    int32_t n, gated;
    float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, invfx, invfy;
    float F[9], ex, ey;
    int32_t pad;
};
struct Work { int32_t k, na, nb, pad; };   // neighbour, node position in the current keyframe's CSR, in the neighbour's
struct Rec { int32_t neighbour, idx1, idx2; float pos[3], normal[3], minDistance, maxDistance; };   // OrblNewPoint

struct Args {
    const KfDev* kf;          // [0] the current keyframe, [1 + k] neighbour k
    const Work* work;
    int32_t nNeigh, n1, nWork, nlevels;
    float sf[16], sigma2[16];
    float ratioFactor;
    int32_t* m12;             // nNeigh x n1, -1 where the search found nothing
    uint8_t* status;          // nNeigh x n1
    Rec* rec;                 // nNeigh x n1 slots
    int32_t* cnt;             // nNeigh
    int32_t* total;           // the call's count
    Rec* out;                 // n1 slots: a query yields at most one point
};

__global__ __launch_bounds__(kSearchThreads) void k_newpoints_search(Args a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Work w = a.work[blockIdx.x];
    const KfDev& A = a.kf[0];
    const KfDev& B = a.kf[1 + w.k];
    const int s1 = A.fvStart[w.na], e1 = A.fvStart[w.na + 1], s2 = B.fvStart[w.nb], e2 = B.fvStart[w.nb + 1];
    int32_t* m12 = a.m12 + (int64_t)w.k * a.n1;
    for (int i1 = s1 + (int)blockIdx.y * kSearchWaves + wave; i1 < e1; i1 += kSearchWaves * (int)gridDim.y) {
        const int q = A.fvIdx[i1];
        if (A.skip && A.skip[q]) continue;
        const orbm::KeyDev kp1 = A.keys[q];
        uint32_t qw[8];
        const uint32_t* qp = (const uint32_t*)(A.desc + (int64_t)q * 32);
#pragma unroll
        for (int i = 0; i < 8; i++) qw[i] = qp[i];
        // epipolar line in image 2: l = x1' F12 (ORBmatcher.cc:141-146)
        const float la = __fadd_rn(__fadd_rn(__fmul_rn(kp1.x, B.F[0]), __fmul_rn(kp1.y, B.F[3])), B.F[6]);
        const float lb = __fadd_rn(__fadd_rn(__fmul_rn(kp1.x, B.F[1]), __fmul_rn(kp1.y, B.F[4])), B.F[7]);
        const float lc = __fadd_rn(__fadd_rn(__fmul_rn(kp1.x, B.F[2]), __fmul_rn(kp1.y, B.F[5])), B.F[8]);
        const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
        uint32_t best = 0xFFFFFFFFu;
        for (int i2 = s2 + lane; i2 < e2; i2 += 64) {
            const int t = B.fvIdx[i2];
            if (B.skip && B.skip[t]) continue;
            const int d = orbm::hamming256(qw, (const uint32_t*)(B.desc + (int64_t)t * 32));
            if (d > 50) continue;  // TH_LOW
            const orbm::KeyDev& kp2 = B.keys[t];
            const float dx = __fsub_rn(B.ex, kp2.x), dy = __fsub_rn(B.ey, kp2.y);
            if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.f, a.sf[kp2.octave & 15])) continue;
            if (den == 0) continue;
            const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, kp2.x), __fmul_rn(lb, kp2.y)), lc);
            const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
            if (!((double)dsqr < 3.84 * (double)a.sigma2[kp2.octave & 15])) continue;
            const uint32_t key = ((uint32_t)d << 22) | (0x3FFFFFu - (uint32_t)(i2 - s2));
            best = min(best, key);
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) best = min(best, (uint32_t)__shfl_xor(best, dd));
        if (best != 0xFFFFFFFFu && lane == 0) m12[q] = B.fvIdx[s2 + (int)(0x3FFFFFu - (best & 0x3FFFFFu))];
    }
}

// Rcw.row(r).dot(x3Dt) + tcw(r): Mat::dot's double sum plus the float, rounded to float by the assignment
__device__ __forceinline__ float row_dot(const float* R, int r, const float* X, float t)
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)R[3 * r + k] * (double)X[k];
    return (float)(s + (double)t);
}

// (flatten: cvm::jacobi_svd is inlined here as it is in the Initializer's kernels -- no call left in the device code)
__global__ __launch_bounds__(kTriThreads) __attribute__((flatten)) void k_newpoints_triangulate(Args a)
{
    __shared__ float sA[16 * kTriThreads], sV[16 * kTriThreads];
    __shared__ double sW[4 * kTriThreads];
    const int64_t i = (int64_t)blockIdx.x * kTriThreads + threadIdx.x;
    if (i >= (int64_t)a.nNeigh * a.n1) return;   // (no barrier below)
    const int k = (int)(i / a.n1), q = (int)(i % a.n1);
    const KfDev& A = a.kf[0];
    const KfDev& B = a.kf[1 + k];
    if (B.gated) { a.status[i] = ST_NEIGHBOUR; return; }
    if (A.skip && A.skip[q]) { a.status[i] = ST_FEATURE; return; }
    const int t = a.m12[i];
    if (t < 0) { a.status[i] = ST_NO_MATCH; return; }
    const orbm::KeyDev kp1 = A.keys[q], kp2 = B.keys[t];
    // xn = ((u - cx)*invfx, (v - cy)*invfy, 1), ray = Rwc*xn (gemm's small-matrix branch on the transposed rotation)
    const float xn1[3] = {(kp1.x - A.cx) * A.invfx, (kp1.y - A.cy) * A.invfy, 1.f};
    const float xn2[3] = {(kp2.x - B.cx) * B.invfx, (kp2.y - B.cy) * B.invfy, 1.f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ray1[r] = cvm::gemm3_elem(A.Rcw[r], A.Rcw[3 + r], A.Rcw[6 + r], xn1[0], xn1[1], xn1[2], 1.0, 0.f, 0.0);
        ray2[r] = cvm::gemm3_elem(B.Rcw[r], B.Rcw[3 + r], B.Rcw[6 + r], xn2[0], xn2[1], xn2[2], 1.0, 0.f, 0.0);
    }
    double dt = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) dt += (double)ray1[r] * (double)ray2[r];
    const float cosParallaxRays = (float)(dt / (cvm::norm3(ray1) * cvm::norm3(ray2)));
    // monocular: cosParallaxStereo = cosParallaxRays + 1, so the test is cos > 0 && cos < 0.9998
    if (!(cosParallaxRays > 0 && (double)cosParallaxRays < 0.9998)) { a.status[i] = ST_PARALLAX; return; }
    // A.row(r) = x*Tcw.row(2) - Tcw.row(0|1): MatOp_AddEx(alpha = x, beta = -1) -> addWeighted in double; x == 1: subtract
    float* At = sA + threadIdx.x;
    float* Vt = sV + threadIdx.x;
    double* W = sW + threadIdx.x;
    const float xs[4] = {xn1[0], xn1[1], xn2[0], xn2[1]};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const KfDev& S = r < 2 ? A : B;
        const int pr = r & 1;
        const float x = xs[r];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float t2 = c < 3 ? S.Rcw[6 + c] : S.tcw[2], t0 = c < 3 ? S.Rcw[3 * pr + c] : S.tcw[pr];
            const float v = x == 1.f ? t2 - t0 : (float)((double)t2 * (double)x + (double)t0 * -1.0 + 0.0);
            At[(c * 4 + r) * kTriThreads] = v;   // !at: temp_a = A.t()
        }
    }
    cvm::jacobi_svd<float, kTriThreads>(At, W, Vt, 4, 4, 4, true, false);
    const float v3 = Vt[15 * kTriThreads];
    if (v3 == 0) { a.status[i] = ST_X3D_ZERO; return; }
    const double alpha = 1. / (double)v3;
    float X[3];
#pragma unroll
    for (int c = 0; c < 3; c++) X[c] = cvm::expr_scale(Vt[(12 + c) * kTriThreads], alpha);
    const float z1 = row_dot(A.Rcw, 2, X, A.tcw[2]);
    if (z1 <= 0) { a.status[i] = ST_Z1; return; }
    const float z2 = row_dot(B.Rcw, 2, X, B.tcw[2]);
    if (z2 <= 0) { a.status[i] = ST_Z2; return; }
    const int o1 = kp1.octave & 15, o2 = kp2.octave & 15;
    {
        const float x1 = row_dot(A.Rcw, 0, X, A.tcw[0]), y1 = row_dot(A.Rcw, 1, X, A.tcw[1]);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = A.fx * x1 * invz1 + A.cx, v1 = A.fy * y1 * invz1 + A.cy;
        const float ex = u1 - kp1.x, ey = v1 - kp1.y;
        if ((double)(ex * ex + ey * ey) > 5.991 * (double)a.sigma2[o1]) { a.status[i] = ST_REPROJ1; return; }
    }
    {
        const float x2 = row_dot(B.Rcw, 0, X, B.tcw[0]), y2 = row_dot(B.Rcw, 1, X, B.tcw[1]);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = B.fx * x2 * invz2 + B.cx, v2 = B.fy * y2 * invz2 + B.cy;
        const float ex = u2 - kp2.x, ey = v2 - kp2.y;
        if ((double)(ex * ex + ey * ey) > 5.991 * (double)a.sigma2[o2]) { a.status[i] = ST_REPROJ2; return; }
    }
    float n1[3], n2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { n1[c] = X[c] - A.Ow[c]; n2[c] = X[c] - B.Ow[c]; }
    const double nd1 = cvm::norm3(n1), nd2 = cvm::norm3(n2);
    const float dist1 = (float)nd1, dist2 = (float)nd2;
    if (dist1 == 0 || dist2 == 0) { a.status[i] = ST_DIST_ZERO; return; }
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = a.sf[o1] / a.sf[o2];
    if (ratioDist * a.ratioFactor < ratioOctave || ratioDist > ratioOctave * a.ratioFactor) { a.status[i] = ST_SCALE; return; }
    // MapPoint::UpdateNormalAndDepth (MapPoint.cc:330-371) with these two observations, mpRefKF the current keyframe
    Rec r;
    r.neighbour = k; r.idx1 = q; r.idx2 = t;
    // normal = normal + normali/cv::norm(normali): one MatOp_AddEx (alpha = 1/norm, beta = 1) -> cv::scaleAdd on CV_32F: the
    // scale converted to float, a float product, a float sum; normal starts as zeros
    const float a1 = (float)(1. / nd1), a2 = (float)(1. / nd2);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        r.pos[c] = X[c];
        const float s = n2[c] * a2 + (n1[c] * a1 + 0.f);
        r.normal[c] = cvm::expr_scale(s, 1. / 2);
    }
    r.maxDistance = dist1 * a.sf[o1];
    r.minDistance = r.maxDistance / a.sf[(a.nlevels - 1) & 15];
    a.rec[i] = r;
    a.status[i] = ST_ACCEPTED;
}

__global__ __launch_bounds__(kRowThreads) void k_newpoints_resolve(Args a)
{
    const int q = blockIdx.x * kRowThreads + threadIdx.x;
    if (q >= a.n1) return;
    bool taken = false;
    for (int k = 0; k < a.nNeigh; k++) {
        uint8_t* st = a.status + (int64_t)k * a.n1 + q;
        const uint8_t s = *st;
        if (taken) { if (s != ST_NEIGHBOUR) *st = ST_FEATURE; }
        else if (s == ST_ACCEPTED) taken = true;
    }
}

__global__ __launch_bounds__(kRowThreads) void k_newpoints_count(Args a)
{
    __shared__ int sWave[kRowThreads / 64];
    const int k = blockIdx.x;
    const uint8_t* st = a.status + (int64_t)k * a.n1;
    int total = 0;
    for (int base = 0; base < a.n1; base += kRowThreads) {
        const int q = base + threadIdx.x;
        int chunk;
        __syncthreads();   // (the previous chunk's reads of sWave are done)
        (void)orbf::block_rank<kRowThreads>(q < a.n1 && st[q] == ST_ACCEPTED, sWave, chunk);
        total += chunk;
    }
    if (threadIdx.x == 0) a.cnt[k] = total;
}

__global__ __launch_bounds__(kRowThreads) void k_newpoints_compact(Args a)
{
    __shared__ int sWave[kRowThreads / 64];
    const int k = blockIdx.x;
    int pos = 0;
    for (int j = 0; j < k; j++) pos += a.cnt[j];
    const uint8_t* st = a.status + (int64_t)k * a.n1;
    for (int base = 0; base < a.n1; base += kRowThreads) {
        const int q = base + threadIdx.x;
        const bool f = q < a.n1 && st[q] == ST_ACCEPTED;
        int chunk;
        __syncthreads();   // (the previous chunk's reads of sWave are done)
        const int r = orbf::block_rank<kRowThreads>(f, sWave, chunk);
        if (f && pos + r < a.n1) a.out[pos + r] = a.rec[(int64_t)k * a.n1 + q];
        pos += chunk;
    }
    if (k == a.nNeigh - 1 && threadIdx.x == 0) *a.total = pos;
}

// ------------------------------------------------------------------ SearchInNeighbors: the batched Fuse
// k_fuse_batch: the searches of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:854-951, monocular) for every
// (target, point) of a job list, one launch however many targets.  A workgroup takes one tile of kFuseTile consecutive job
// entries of ONE target (the host cuts the CSR into tiles: FuseWork), so the machine is filled from the job list and not
// from a target.  Two steps:
//   1. one lane per entry: the projection gates (orbf::project_gates), the result of a pair that a gate ended written at
//      once, the survivors compacted by ballot (orbf::block_rank) into LDS;
//   2. kFuseLpp lanes per survivor walk its window together in GetFeaturesInArea's order (for_each_in_area): each lane
//      holds 32 / kFuseLpp bytes of the point's descriptor and reads that share of a candidate's (one 32-byte line per
//      candidate and group instead of a 32-byte gather per lane), the partial popcounts are summed across the lanes, and
//      every lane keeps the same (bestDist, bestIdx) under the strict `<` of k_window_best.  This is orbf::window_best's
//      walk plus the chi-square test of :905-917, written out here: as a call of a shared template the kernel took two
//      more registers and its callers measured slower than the parent's (docs/experiments.md, "One Fuse core").
// No atomics: a job entry is written by exactly one lane.  kFuseLpp is a build-time choice (-DORBL_FUSE_LPP=1|2|4|8) so that
// tools/fuse_bench.py can A/B it; 8 measured best, and staging the target's cell-start table in LDS lost at every kFuseLpp
// (docs/experiments.md, "k_fuse_batch: lanes per point").
#ifndef ORBL_FUSE_LPP
#define ORBL_FUSE_LPP 8
#endif
constexpr int kFuseLpp = ORBL_FUSE_LPP;
constexpr int kFuseThreads = 256;
constexpr int kFuseTile = kFuseThreads / kFuseLpp;
static_assert(kFuseLpp == 1 || kFuseLpp == 2 || kFuseLpp == 4 || kFuseLpp == 8, "lanes per point");

struct FuseRes { int32_t bestIdx, bestDist; float u, v; int8_t level; uint8_t status, pad[2]; };  // OrblFuseResult
struct FuseWork { int32_t target, begin, count, pad; };
struct FuseArgs {
    const orbf::FuseTgt* tgt; const orbf::FusePt* pts; const int32_t* jobPoint; const FuseWork* work;
    FuseRes* out;
    float th; int32_t nlevels;
    float sf[16], invSigma2[16], breaks[17];
};

__global__ __launch_bounds__(kFuseThreads) void k_fuse_batch(FuseArgs a)
{
    __shared__ float sU[kFuseTile], sV[kFuseTile];
    __shared__ int32_t sEntry[kFuseTile], sPoint[kFuseTile], sLevel[kFuseTile];
    __shared__ int sWave[kFuseThreads / 64];
    const int tid = threadIdx.x;
    const FuseWork w = a.work[blockIdx.x];
    const orbf::FuseTgt& T = a.tgt[w.target];
    const orbm::GridDev grid = T.grid;
    // 1. the projection gates (:855-892), one lane per entry
    bool alive = false;
    float u = 0.f, v = 0.f;
    int level = -1, entry = 0, p = 0;
    if (tid < w.count) {   // (w.count <= kFuseTile)
        entry = w.begin + tid;
        p = a.jobPoint[entry];
        uint8_t st;
        alive = orbf::project_gates(T, a.pts[p], a.nlevels, a.breaks, u, v, level, st);
        if (!alive) {
            FuseRes r;
            r.bestIdx = -1; r.bestDist = 256; r.u = u; r.v = v; r.level = (int8_t)level; r.status = st; r.pad[0] = r.pad[1] = 0;
            a.out[entry] = r;
        }
    }
    // the survivors, in entry order
    int nSurv;
    const int s0 = orbf::block_rank<kFuseThreads>(alive, sWave, nSurv);
    if (alive) { sU[s0] = u; sV[s0] = v; sEntry[s0] = entry; sPoint[s0] = p; sLevel[s0] = level; }
    __syncthreads();
    // 2. kFuseLpp lanes per survivor: :894-951
    constexpr int W = 8 / kFuseLpp;
    const int sub = tid % kFuseLpp;
    for (int s = tid / kFuseLpp; s < nSurv; s += kFuseThreads / kFuseLpp) {
        const float su = sU[s], sv = sV[s];
        const int pred = sLevel[s];
        const float radius = a.th * a.sf[pred];
        uint32_t qw[W];
        const uint32_t* qp = a.pts[sPoint[s]].desc + sub * W;
#pragma unroll
        for (int i = 0; i < W; i++) qw[i] = qp[i];
        int bestDist = 256, bestIdx = -1;
        orbm::for_each_in_area(grid, T.keys, T.cellStart, T.cellIdx, su, sv, radius, -1, -1, [&](int idx) {
            const orbm::KeyDev& kp = T.keys[idx];
            const int kpLevel = kp.octave;
            if (kpLevel < pred - 1 || kpLevel > pred) return;
            const float ex = __fsub_rn(su, kp.x), ey = __fsub_rn(sv, kp.y);
            const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
            if ((double)__fmul_rn(e2, a.invSigma2[kpLevel]) > 5.99) return;
            const uint32_t* tp = (const uint32_t*)(T.desc + (int64_t)idx * 32) + sub * W;
            int d = 0;
#pragma unroll
            for (int i = 0; i < W; i++) d += __popc(qw[i] ^ tp[i]);
            // (the lanes of a point take the same path through the walk: their partners are active here)
#pragma unroll
            for (int k = kFuseLpp / 2; k >= 1; k >>= 1) d += __shfl_xor(d, k);
            if (d < bestDist) { bestDist = d; bestIdx = idx; }
        });
        if (sub == 0) {
            FuseRes o;
            o.bestIdx = bestIdx; o.bestDist = bestDist; o.u = su; o.v = sv; o.level = (int8_t)pred;
            o.status = bestIdx >= 0 ? orbf::FST_FOUND : orbf::FST_NO_CANDIDATE; o.pad[0] = o.pad[1] = 0;
            a.out[sEntry[s]] = o;
        }
    }
}

}  // namespace orbl
