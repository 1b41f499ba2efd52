// orbw_kernels.hip -- the device side of the map-point pool (part of orbslamm_hip.hip; ABI: include/orbslamm_mappool.h,
// DESIGN.md §8q; host side: orbw_host.inc).
//   k_pool_scatter   a setter's staged records (or flag bytes alone) into the pool's slots
//   k_view_project   Frame::isInFrustum + the head of SearchByProjection(F, vpMapPoints, th) (Frame.cc:269-325,
//                    ORBmatcher.cc:45-69), or the projection loop of SearchByProjection(CurrentFrame, LastFrame)
//                    (ORBmatcher.cc:1353-1392, monocular), one thread per query: it writes the query block k_proj_candidates
//                    and k_proj_resolve read (quvr, qlvl, qdesc, qvalid, qobs) and one status byte per query, and its last
//                    workgroups bring the call's staging head (pair record, occupancy) up
// A pool record is 68 bytes in four arrays, each read in one access: a = (pos, minDistance) and b = (normal, maxDistance) as
// float4, the flags as a word, the descriptor as two uint4.  A query's gather is element-granular by nature (a local map's
// points come in no order): 16-byte accesses, the lines come from L2 / Infinity Cache where the last frame left them.
// Arithmetic: one IEEE operation per source operation (-ffp-contract=off); OpenCV's pieces are orbx_cvmath.hpp's.
#pragma once

namespace orbw {

constexpr int kThreads = 256;
// the status codes of include/orbslamm_mappool.h (ORBW_ST_*)
enum : uint8_t { ST_BAD = 0, ST_DEPTH, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_VIEW_ANGLE, ST_LEVEL_RANGE, ST_IN_VIEW, ST_NO_POINT };

struct PoolDev { float4* a; float4* b; uint32_t* flags; uint4* desc; int32_t cap; };

// one staged record of orbw_pool_set: the record's arrays back to back, all 16-byte aligned (80 bytes)
struct StagedPoint { float4 a, b; uint4 d0, d1; uint32_t flags, id, pad[2]; };

// mode 0: n StagedPoint -> the four arrays.  mode 1: {id, flags} pairs -> the flags alone.  Ids are distinct within a call
// (the host keeps the last of a repeated id) and inside the pool (checked on the host).
__global__ __launch_bounds__(kThreads) void k_pool_scatter(PoolDev pool, const void* __restrict__ staged, int n, int mode)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) {
        const StagedPoint s = ((const StagedPoint*)staged)[i];
        if (s.id >= (uint32_t)pool.cap) return;
        pool.a[s.id] = s.a; pool.b[s.id] = s.b; pool.desc[2 * (size_t)s.id] = s.d0; pool.desc[2 * (size_t)s.id + 1] = s.d1; pool.flags[s.id] = s.flags;
    } else {
        const uint2 s = ((const uint2*)staged)[i];
        if (s.x >= (uint32_t)pool.cap) return;
        pool.flags[s.x] = s.y;
    }
}

// the view record (OrbwView), the call's th, and the two level tables; a kernel argument (scalar loads, no upload)
struct ViewArgs {
    float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, minX, maxX, minY, maxY, cosLimit;
    float th;
    int32_t nlevels;
    int32_t frame;                       // 0: local-map gate set, 1: frame/frame gate set
    float scale[16];                     // mvScaleFactors
    float breaks[17];                    // orbl_level_breaks' table (local-map gate set)
};
struct ProjectArgs {
    PoolDev pool;
    const int32_t* ids; int32_t nq;      // ids: pinned host memory (the searches) or device memory
    const orbm::KeyDev* lastKeys; const int32_t* lastN;   // frame/frame: the resident LastFrame
    float* quvr; int8_t* qlvl; uint4* qdesc; uint8_t* qvalid; uint8_t* qobs;   // qdesc null: frame/frame (LastFrame's own rows), or no search behind
    float* viewcos; uint8_t* status;     // viewcos optional; status: pinned host memory (the searches) or device memory
    const uint4* headSrc; uint4* headDst; int32_t head16;   // the staging head: head16 16-byte pieces, copied by the workgroups behind the queries'
};

__device__ __forceinline__ float radius_by_viewing_cos(float viewCos) { return (double)viewCos > 0.998 ? 2.5f : 4.0f; }   // ORBmatcher.cc:131-137

// the frame/frame gate set (ORBmatcher.cc:1362-1389, monocular) for one LastFrame point A of the given octave under the pose
// (Rcw, tcw): its status, and where it is in view the projection and the search radius.  k_view_project's and
// orbq::k_motion_project's one statement of it.
__device__ __forceinline__ uint8_t frame_gate(const float (&Rcw)[9], const float (&tcw)[3], float fx, float fy, float cx, float cy,
                                              float minX, float maxX, float minY, float maxY, float th, const float* scale,
                                              const float4 A, int octave, float& u, float& v, float& r)
{
    float pc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) pc[i] = cvm::gemm3_elem(Rcw[3 * i], Rcw[3 * i + 1], Rcw[3 * i + 2], A.x, A.y, A.z, 1.0, tcw[i], 1.0);
    const float invzc = (float)(1.0 / (double)pc[2]);   // :1367
    if (invzc < 0) return ST_DEPTH;
    u = fx * pc[0] * invzc + cx; v = fy * pc[1] * invzc + cy;
    if (!(u >= minX && u <= maxX && v >= minY && v <= maxY)) return ST_OUT_OF_IMAGE;
    r = th * scale[min(max(octave, 0), 15)];
    return ST_IN_VIEW;
}

__global__ __launch_bounds__(kThreads) void k_view_project(ProjectArgs p, ViewArgs V)
{
    const int qBlocks = (p.nq + kThreads - 1) / kThreads;
    if ((int)blockIdx.x >= qBlocks) {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const int i = ((int)blockIdx.x - qBlocks) * kThreads + threadIdx.x;
        if (i < p.head16) ((u32x4*)p.headDst)[i] = __builtin_nontemporal_load((const u32x4*)p.headSrc + i);
        return;
    }
    const int q = blockIdx.x * kThreads + threadIdx.x;
    const bool live = q < p.nq;
    const int id = live ? p.ids[q] : -1;
    float u = 0.f, v = 0.f, r = 0.f, viewCos = 0.f;
    int lo = 0, hi = 0;
    uint8_t st = 0, obs = 0;
    if (!live) {
    } else if (id < 0 || id >= p.pool.cap || (V.frame && q >= *p.lastN)) {
        st = ST_NO_POINT;   // (the host has checked the ids: a local-map list holds none, a frame/frame list -1 alone)
        if (p.qdesc) { p.qdesc[2 * (size_t)q] = make_uint4(0, 0, 0, 0); p.qdesc[2 * (size_t)q + 1] = make_uint4(0, 0, 0, 0); }
    } else if (V.frame) {
        // ORBmatcher.cc:1353-1392
        const float4 A = p.pool.a[id];
        obs = (p.pool.flags[id] >> 1) & 1;
        const int octave = p.lastKeys[q].octave;
        lo = octave - 1; hi = octave + 1;
        st = frame_gate(V.Rcw, V.tcw, V.fx, V.fy, V.cx, V.cy, V.minX, V.maxX, V.minY, V.maxY, V.th, V.scale, A, octave, u, v, r);
    } else {
        // Frame.cc:269-325, ORBmatcher.cc:57-69
        const float4 A = p.pool.a[id], B = p.pool.b[id];
        const uint32_t flags = p.pool.flags[id];
        if (p.qdesc) { p.qdesc[2 * (size_t)q] = p.pool.desc[2 * (size_t)id]; p.qdesc[2 * (size_t)q + 1] = p.pool.desc[2 * (size_t)id + 1]; }
        obs = (flags >> 1) & 1;
        int level = -1;
        st = ST_BAD;
        if (!(flags & 1)) {
            float pc[3];
#pragma unroll
            for (int i = 0; i < 3; i++) pc[i] = cvm::gemm3_elem(V.Rcw[3 * i], V.Rcw[3 * i + 1], V.Rcw[3 * i + 2], A.x, A.y, A.z, 1.0, V.tcw[i], 1.0);
            st = ST_DEPTH;
            if (!(pc[2] < 0.0f)) {
                const float invz = __fdiv_rn(1.0f, pc[2]);
                u = V.fx * pc[0] * invz + V.cx; v = V.fy * pc[1] * invz + V.cy;
                st = ST_OUT_OF_IMAGE;
                if (u >= V.minX && u <= V.maxX && v >= V.minY && v <= V.maxY) {
                    const float maxDistance = 1.2f * B.w, minDistance = 0.8f * A.w;
                    const float PO[3] = {A.x - V.Ow[0], A.y - V.Ow[1], A.z - V.Ow[2]};
                    const float dist = (float)cvm::norm3(PO);
                    st = ST_DISTANCE;
                    if (!(dist < minDistance || dist > maxDistance)) {
                        const double dt = 0. + (double)PO[0] * (double)B.x + (double)PO[1] * (double)B.y + (double)PO[2] * (double)B.z;
                        viewCos = (float)(dt / (double)dist);
                        st = ST_VIEW_ANGLE;
                        if (!(viewCos < V.cosLimit)) {
                            // PredictScale: the breaks below ratio (a NaN ratio is above none)
                            const float ratio = __fdiv_rn(B.w, dist);
                            int c = 0;
                            for (int j = 0; j <= V.nlevels; j++) c += ratio > V.breaks[j] ? 1 : 0;
                            level = c - 1;
                            st = ST_LEVEL_RANGE;
                            if (c >= 1 && c <= V.nlevels) {
                                st = ST_IN_VIEW;
                                r = radius_by_viewing_cos(viewCos);
                                if ((double)V.th != 1.0) r *= V.th;
                                r = r * V.scale[level];
                            }
                        }
                    }
                }
            }
        }
        lo = level - 1; hi = level;
    }
    if (live) {
        p.quvr[3 * (size_t)q] = u; p.quvr[3 * (size_t)q + 1] = v; p.quvr[3 * (size_t)q + 2] = r;
        p.qlvl[2 * (size_t)q] = (int8_t)lo; p.qlvl[2 * (size_t)q + 1] = (int8_t)hi;
        p.qvalid[q] = st == ST_IN_VIEW ? 1 : 0;
        p.qobs[q] = obs;
        if (p.viewcos) p.viewcos[q] = viewCos;
    }
    // the status bytes may cross the link to pinned host memory: four queries' bytes leave as one word (the array is
    // padded to 16 bytes; the bytes behind nq are 0)
    uint32_t w = st;
    w |= (uint32_t)__shfl_down((int)w, 1) << 8;
    w |= (uint32_t)__shfl_down((int)w, 2) << 16;
    if ((threadIdx.x & 3) == 0 && live) ((uint32_t*)p.status)[q >> 2] = w;
}

}  // namespace orbw
