// orbx_hostutil.inc -- what every family's host side shares (part of orbslamm_hip.hip, behind HIPCHK): the create-time
// check, the grow-only device and pinned blocks, the packer of a staging block.

// HIPCHK inside a create function: records the error, then runs `cleanup` (destroy the half-built object) and returns
#define HIPCHK_OR(expr, cleanup)                                                             \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            int r_ = fail(ORBX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
            cleanup;                                                                         \
            return r_;                                                                       \
        }                                                                                    \
    } while (0)

// Grow-only device scratch: a block that is too small is freed and replaced by one of max(bytes * 3/2, floor) bytes; its
// content is not kept.  drain: a stream whose queued work may still use the old block, synchronised before the free
// (nullptr: the call site knows nothing is in flight, or is on a latency path and frees as the runtime orders it).
// counter: the handle's allocation counter, where the steady-state tests read one (orbm_alloc_stats).
template <class T>
static int grow_device(T*& p, size_t& cap, size_t bytes, size_t floor, const hipStream_t* drain = nullptr, std::atomic<int64_t>* counter = nullptr)
{
    if (bytes <= cap) return ORBX_OK;
    if (drain) HIPCHK(hipStreamSynchronize(*drain));
    if (p) HIPCHK(hipFree(p));
    p = nullptr; cap = 0;
    const size_t want = std::max<size_t>(bytes * 3 / 2, floor);
    HIPCHK(hipMalloc((void**)&p, want));
    if (counter) ++*counter;
    cap = want;
    return ORBX_OK;
}

// The same for pinned staging (floor 64 KB).  flagWord: the block is read and written by copy KERNELS where it lies and the
// host polls a flag behind it (stage_down_wait, orbv_transform): explicitly coherent, the capacity a multiple of 64 and a
// 64-byte flag word, zeroed here, at p + cap.
template <class T>
static int grow_pinned(T*& p, size_t& cap, size_t bytes, bool flagWord, const hipStream_t* drain = nullptr, std::atomic<int64_t>* counter = nullptr)
{
    if (bytes <= cap) return ORBX_OK;
    if (drain) HIPCHK(hipStreamSynchronize(*drain));
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr; cap = 0;
    size_t want = std::max<size_t>(bytes * 3 / 2, 1 << 16);
    if (flagWord) want = (want + 63) & ~(size_t)63;
    HIPCHK(hipHostMalloc((void**)&p, want + (flagWord ? 64 : 0), flagWord ? hipHostMallocCoherent : hipHostMallocDefault));
    if (counter) ++*counter;
    cap = want;
    if (flagWord) *(volatile int32_t*)((uint8_t*)p + want) = 0;
    return ORBX_OK;
}

struct Packer {  // lays host arrays out back to back (16-byte aligned) in a staging block
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; }
};
