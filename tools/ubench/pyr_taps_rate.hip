// micro-benchmark for k_pyramid's row loop: (a) the issue rate of v_dot2_u32_u16 beside v_perm_b32 and v_mul_i32_i24
// (pk_min3_rate.hip: 4.69 and 4.54 cycles per wave-instruction), 8 independent chains per lane, 8 waves per SIMD;
// (b) what one row iteration of a dword group costs -- the eight taps of two source rows and the two horizontal sums
// of four pixels -- at the kernel's access pattern (52 groups x 4 row lanes on 256 threads, a level-0 tile of 252-byte
// rows, scale 1.2: the lanes of a wave 4.8 bytes apart), in three forms:
//   0  sixteen ds_read_u8, mul + mad per sum (the form before the window)
//   1  two unaligned 8-byte reads at the first tap, perm + dot2 per sum
//   2  two aligned reads of three dwords at (first tap) & ~3 and two v_alignbyte_b32 each, perm + dot2 per sum
//   3  form 0 as hipcc compiles it when left alone: six unaligned ds_read_u16, four ds_read_u8
// All forms must print the same checksum.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/pyr_taps_rate.hip -o build_ub/pyr_taps_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>

template <int OP>
__global__ void k_rate(uint32_t* out, int iters)
{
    uint32_t a[8];
    for (int i = 0; i < 8; i++) a[i] = ((threadIdx.x * 37u + i * 11u) & 0xFF) | (((threadIdx.x * 13u + i * 7u) & 0xFF) << 16);
    uint32_t b = (threadIdx.x & 0xFF) | 0x00400000u, c = 0x00330021u;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (OP == 0) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
            if (OP == 1) asm volatile("v_mul_i32_i24 %0, %0, %1" : "+v"(a[i]) : "v"(b));
            if (OP == 2) asm volatile("v_mad_i32_i24 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
            if (OP == 3) asm volatile("v_dot2_u32_u16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
            if (OP == 4) asm volatile("v_dot2_u32_u16 %0, %0, %1, 0" : "+v"(a[i]) : "v"(b));
            if (OP == 5) asm volatile("v_alignbyte_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        }
    }
    uint32_t s = 0;
    for (int i = 0; i < 8; i++) s += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
constexpr int kCols = 52, kRowLanes = 4;          // dword groups per output row, row lanes: 208 of 256 threads work
constexpr int kSrcRows = 48, kSrcStride = 252;    // the source tile (bytes)
constexpr int kOutRows = (kSrcRows - 2) * 5 / 6;  // output rows at scale 1.2
constexpr int kTileWords = kSrcStride / 4 * kSrcRows + 4;

template <int FORM>
__global__ __launch_bounds__(256) void k_taps(uint32_t* out, int iters)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint8_t* const ldsb = (uint8_t*)lds;
    uint32_t* const syo = lds + kTileWords;   // per output row: the byte offset of its upper source row
    const int tid = threadIdx.x;
    for (int i = tid; i < kTileWords; i += 256) lds[i] = (uint32_t)i * 2654435761u ^ (uint32_t)(i >> 3);
    for (int i = tid; i < kOutRows; i += 256) syo[i] = (uint32_t)(((12 * i + 1) / 10) * kSrcStride);   // floor((i + .5) * 1.2 - .5)
    __syncthreads();
    const int yy0 = tid / kCols, gx = tid - yy0 * kCols;
    uint32_t acc = 0;
    if (yy0 < kRowLanes) {
        int sx[4], a0[4], a1[4];
        uint32_t sel[4], ac[4];
        for (int i = 0; i < 4; i++) {
            const int dx = 4 * gx + i, num = 12 * dx + 1;       // (dx + .5) * 1.2 - .5 = num / 10
            sx[i] = num / 10;
            a1[i] = (num - 10 * sx[i]) * 2048 / 10; a0[i] = 2048 - a1[i];
            const uint32_t d = (uint32_t)(sx[i] - sx[0]);
            sel[i] = d * 0x00010001u + 0x0c010c00u;
            ac[i] = (uint32_t)a0[i] | ((uint32_t)a1[i] << 16);
        }
        const int wo = sx[0], wsh = wo & 3, wo4 = (wo & ~3) >> 2;
        for (int it = 0; it < iters; it++) {
            for (int yy = yy0; yy < kOutRows; yy += kRowLanes) {
                const int o0 = (int)syo[yy], o1 = o0 + kSrcStride;
                if (FORM == 0) {
                    // through a volatile LDS pointer: sixteen ds_read_u8, as the kernel's loop had them
                    typedef const volatile __attribute__((address_space(3))) uint8_t lds_vbyte;
                    lds_vbyte* const vb = (lds_vbyte*)ldsb;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int s00 = vb[o0 + sx[i]], s01 = vb[o0 + sx[i] + 1], s10 = vb[o1 + sx[i]], s11 = vb[o1 + sx[i] + 1];
                        acc += (uint32_t)(s00 * a0[i] + s01 * a1[i]);
                        acc += (uint32_t)(s10 * a0[i] + s11 * a1[i]);
                    }
                } else if (FORM == 3) {
                    // left alone, hipcc merges a pixel's two adjacent bytes into one UNALIGNED ds_read_u16 here
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int s00 = ldsb[o0 + sx[i]], s10 = ldsb[o1 + sx[i]];
                        acc += (uint32_t)(s00 * a0[i] + ldsb[o0 + sx[i] + 1] * a1[i]);
                        acc += (uint32_t)(s10 * a0[i] + ldsb[o1 + sx[i] + 1] * a1[i]);
                    }
                } else {
                    uint2 w0, w1;
                    if (FORM == 1) {
                        __builtin_memcpy(&w0, ldsb + o0 + wo, 8);
                        __builtin_memcpy(&w1, ldsb + o1 + wo, 8);
                    } else {
                        const uint32_t* q0 = lds + (o0 >> 2) + wo4;
                        const uint32_t* q1 = lds + (o1 >> 2) + wo4;
                        const uint32_t u0 = q0[0], u1 = q0[1], u2 = q0[2], t0 = q1[0], t1 = q1[1], t2 = q1[2];
                        w0 = make_uint2(__builtin_amdgcn_alignbyte(u1, u0, wsh), __builtin_amdgcn_alignbyte(u2, u1, wsh));
                        w1 = make_uint2(__builtin_amdgcn_alignbyte(t1, t0, wsh), __builtin_amdgcn_alignbyte(t2, t1, wsh));
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const u16x2 a = __builtin_bit_cast(u16x2, ac[i]);
                        acc += __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, __builtin_amdgcn_perm(w0.y, w0.x, sel[i])), a, 0u, false);
                        acc += __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, __builtin_amdgcn_perm(w1.y, w1.x, sel[i])), a, 0u, false);
                    }
                }
            }
            acc = acc * 3u + (uint32_t)it;   // the iterations differ: nothing is hoisted out of the loop
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    out[blockIdx.x * 256 + tid] = acc;
}

int main()
{
    const int blocks = 2048;
    uint32_t* d; hipMalloc(&d, blocks * 256 * 4);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    {
        const int iters = 4096;
        const char* names[6] = {"v_perm_b32", "v_mul_i32_i24", "v_mad_i32_i24", "v_dot2_u32_u16", "v_dot2_u32_u16 (c = 0)", "v_alignbyte_b32"};
        for (int op = 0; op < 6; op++) {
            float ms = 0;
            for (int rep = 0; rep < 2; rep++) {
                hipEventRecord(e0);
                switch (op) {
                case 0: k_rate<0><<<blocks, 256>>>(d, iters); break;
                case 1: k_rate<1><<<blocks, 256>>>(d, iters); break;
                case 2: k_rate<2><<<blocks, 256>>>(d, iters); break;
                case 3: k_rate<3><<<blocks, 256>>>(d, iters); break;
                case 4: k_rate<4><<<blocks, 256>>>(d, iters); break;
                case 5: k_rate<5><<<blocks, 256>>>(d, iters); break;
                }
                hipEventRecord(e1); hipEventSynchronize(e1);
                hipEventElapsedTime(&ms, e0, e1);
            }
            const double waveinstr = (double)blocks * 4 * iters * 8;
            printf("%-28s %.3f ms, %.2f cycles per wave-instr per SIMD (at 2.4 GHz)\n", names[op], ms, ms * 1e-3 * 2.4e9 * 1024 / waveinstr);
        }
    }
    {
        // 32 KB per workgroup: five workgroups per CU, as beside the kernel's own tiles
        const int iters = 64, ldsBytes = 32 * 1024;
        static_assert((kTileWords + kOutRows) * 4 <= 32 * 1024, "tile larger than the LDS asked for");
        const char* names[4] = {"16 x ds_read_u8, mul + mad", "2 x unaligned 8 bytes, perm + dot2", "2 x 3 aligned dwords + alignbyte, perm + dot2",
                                "6 x unaligned ds_read_u16 + 4 x u8, mul + mad"};
        std::vector<uint32_t> host(blocks * 256);
        for (int form = 0; form < 4; form++) {
            float ms = 0;
            for (int rep = 0; rep < 2; rep++) {
                hipEventRecord(e0);
                switch (form) {
                case 0: k_taps<0><<<blocks, 256, ldsBytes>>>(d, iters); break;
                case 1: k_taps<1><<<blocks, 256, ldsBytes>>>(d, iters); break;
                case 2: k_taps<2><<<blocks, 256, ldsBytes>>>(d, iters); break;
                case 3: k_taps<3><<<blocks, 256, ldsBytes>>>(d, iters); break;
                }
                hipEventRecord(e1); hipEventSynchronize(e1);
                hipEventElapsedTime(&ms, e0, e1);
            }
            hipMemcpy(host.data(), d, host.size() * 4, hipMemcpyDeviceToHost);
            uint32_t sum = 0;
            for (uint32_t v : host) sum = sum * 31u + v;
            // a wave's row iterations: ceil(kOutRows / kRowLanes) per pass
            const double waveiters = (double)blocks * 4 * iters * ((kOutRows + kRowLanes - 1) / kRowLanes);
            printf("%-46s %.3f ms, %.1f cycles per wave and row iteration per SIMD (at 2.4 GHz), checksum %08x\n", names[form], ms,
                   ms * 1e-3 * 2.4e9 * 1024 / waveiters, sum);
        }
    }
    return 0;
}
