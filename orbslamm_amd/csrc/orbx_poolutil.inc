// orbx_poolutil.inc -- what the host files of the map-point pool's families share (part of orbslamm_hip.hip, in front of
// orbw_host.inc, orbu_host.inc, orbn_host.inc, orbr_host.inc, orbe_host.inc and orbq_host.inc): the pool and the keyframe store as the host holds them, the
// steps of the concurrency rule (DESIGN.md §8q), the id and slot checks, the store's columns, made-once blocks and mark words, its
// generation tag, the last-wins staging and the repeated-key walk.

constexpr int kPoolChunk = 1 << 16;                    // records per pool setter launch: the pinned staging is 5 MB at the most
constexpr size_t kStoreStageBytes = (size_t)8 << 20;   // a store setter launch's staged records

static std::atomic<uint64_t> g_poolSerial{0};   // pools and the stores beside them: one number each, never given twice

// four device arrays (68 bytes a slot), one "set" bit per slot on the host, a mutex, a stream of its own for the setters, and one
// event per stream that has issued a search against it
struct orbw_pool {
    uint64_t serial = ++g_poolSerial;
    orbm_handle* h = nullptr;   // device; a reference is held
    int cap = 0;
    uint8_t* d_block = nullptr;
    orbw::PoolDev dev{};
    std::vector<uint64_t> setBits, seen;   // seen: a setter's scratch, all zero between calls
    std::mutex mu;
    hipStream_t stream = nullptr;
    uint8_t* h_stage = nullptr; size_t stageCap = 0;   // pinned and coherent: k_pool_scatter reads it where it lies
    struct Reader { hipStream_t stream; hipEvent_t ev; };
    std::vector<Reader> readers;   // per stream: behind the projection kernel of the last search issued on it
    bool isSet(int id) const { return (setBits[(size_t)id >> 6] >> (id & 63)) & 1; }
};

struct orbn_blocks; struct orbr_blocks; struct orbe_blocks;   // orbn_host.inc, orbr_host.inc, orbe_host.inc: a family's blocks, made at its first call
constexpr int kStoreFamilies = 3;   // each lists one block of mark words in the store, once

// an optional per-slot array of the store, made at the first call of its setter; has[k]: slot k was given it
template <class T>
struct orbu_column { T* d = nullptr; std::vector<uint8_t> has; };

// keyframe match lists, flags and graph records in HBM beside ONE map-point pool, whose mutex and stream it uses; a "set" byte per
// slot on the host; all blocks of a fixed size made at create, the staging grow-only.  The columns and the pool-sized d_refKf are
// the store's: orbu_host.inc's setters make and fill them, orbu_store_destroy frees them, whichever family reads them.  A family
// owns its blocks alone (covis, refresh, correct) and lists the mark words in them in `marks` for as long as the block lives
struct orbu_store {
    uint64_t serial = ++g_poolSerial;
    orbw_pool* pool = nullptr;
    int kfcap = 0, stride = 0, pitch = 0, maxc = 0, maxcP = 0, maxL = 0;
    uint8_t* d_block = nullptr;
    orbu::StoreDev dev{};
    orbu::Scratch scr{};
    orbu::Out out{};
    uint8_t* h_res = nullptr;                          // pinned, coherent: header | list | votes | L | seen
    uint8_t* h_stage = nullptr; size_t stageCap = 0;   // pinned, coherent: a setter's records, or a call's ids and list
    std::vector<uint8_t> kfSet;
    std::vector<uint64_t> kfSeen, idxSeen;             // the setters' scratch over slots and over indices, all zero between calls
    std::vector<int64_t> eOff, cOff;                   // orbu_kf_write's scratch: they keep their capacity between calls
    int hi = 0;                                        // the highest set slot + 1
    uint32_t gen = 0;
    bool updated = false; int nS = 0;                  // the last update completed: S holds nS ids
    uint32_t updates = 0;                              // updates begun so far: each overwrites S
    unsigned blocks = 1;                               // the point walk's grid at the most: one block a chunk of the whole store, <= 1 024
    int lastNkf = 0;                                   // the local keyframes of the last update: sizes the next update's grid
    orbu_column<uint8_t> oct;                          // orbu_kf_set_octaves: [kfcap * pitch] bytes
    uint8_t octSeen[256] = {};                         // the octave values the store has been given
    orbu_column<uint8_t> desc;                         // orbu_kf_set_descriptors*: [kfcap * pitch * 32] bytes
    orbu_column<float> ctr;                            // orbu_kf_set_centres: [kfcap * 3]
    int32_t* d_refKf = nullptr;                        // orbu_point_set_ref_kf: mpRefKF per pool id [pool capacity], null until the first call
    orbn_blocks* covis = nullptr;                      // orbn_*: null until the first call
    orbr_blocks* refresh = nullptr;                    // orbr_refresh_points: null until the first call (orbe_correct_sim3's included)
    orbe_blocks* correct = nullptr;                    // orbe_correct_sim3: null until the first call
    struct Marks { void* p; size_t bytes; };
    Marks marks[kStoreFamilies]; int nMarks = 0;       // the families' mark words: what orbu_next_generation clears at the wrap
};

static int orbw_pool_check(orbw_pool* p)
{
    if (!p) return fail(ORBX_E_INVALID, "null pool");
    if (!live_has(p)) return fail(ORBX_E_INVALID, "the pool was destroyed");
    HIPCHK(hipSetDevice(p->h->device));
    return ORBX_OK;
}

static int orbu_store_check(orbu_store* s)
{
    if (!s) return fail(ORBX_E_INVALID, "null store");
    if (!live_has(s)) return fail(ORBX_E_INVALID, "the store was destroyed");
    return orbw_pool_check(s->pool);
}

// ---- the concurrency rule (DESIGN.md §8q, "The pool's concurrency rule").  Whoever reads or writes the pool's arrays, a store's
// blocks or its S holds the pool's mutex while it checks and issues.  A reader that returns before its kernel has run leaves an
// event on its stream; a writer waits for every such event before its first launch, and synchronises before it lets go of the mutex.

// (the pool's mutex is held) stream `st` has just been given a kernel that reads the pool
static int orbw_mark_reader(orbw_pool* p, hipStream_t st)
{
    for (auto& r : p->readers) if (r.stream == st) { HIPCHK(hipEventRecord(r.ev, st)); return ORBX_OK; }
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    p->readers.push_back({st, ev});
    HIPCHK(hipEventRecord(ev, st));
    return ORBX_OK;
}

// (mutex held, arguments checked) a writer's last steps before it changes anything: its pinned staging holds `bytes`, every search issued so far has read
static int orbw_begin_write(orbw_pool* p, uint8_t*& stage, size_t& stageCap, size_t bytes)
{
    int rc = grow_pinned(stage, stageCap, bytes, true, nullptr, &p->h->nHostAlloc);
    if (rc) return rc;
    for (auto& r : p->readers) HIPCHK(hipEventSynchronize(r.ev));
    return ORBX_OK;
}

// ---- ids and slots.  (the pool's mutex is held: the set bits are read)

// The checkers run thousands of times a call: the test is inlined into the callers' loops, only the refusal with its message is a call.
__attribute__((noinline, cold)) static int orbw_refuse_id(const orbw_pool* p, const char* what, int i, int32_t v, int32_t id, bool inside)
{
    if (!inside) return fail(ORBX_E_INVALID, "%s[%d] = %d outside the pool of %d", what, i, v, p->cap);
    return fail(ORBX_E_INVALID, "%s[%d]: pool id %d was never set", what, i, id);
}

// what[i] = v is an id of the pool.  none: -1 passes; entry: v is a store entry, whose bit 30 (ORBU_ENTRY_NO_VOTE) is not part of
// the id; set: the id must have been set
__attribute__((always_inline)) static inline int orbw_check_id(const orbw_pool* p, const char* what, int i, int32_t v, bool none, bool entry = false, bool set = true)
{
    if (none && v == -1) return ORBX_OK;
    const int32_t id = entry ? v & ~ORBU_ENTRY_NO_VOTE : v;
    const bool inside = v >= 0 && id < p->cap;
    if (inside && (!set || p->isSet(id))) return ORBX_OK;
    return orbw_refuse_id(p, what, i, v, id, inside);
}

__attribute__((always_inline)) static inline int orbw_check_ids(const orbw_pool* p, const char* what, const int32_t* ids, int n, bool none, bool set = true)
{
    int rc = ORBX_OK;
    for (int i = 0; i < n && !rc; i++) rc = orbw_check_id(p, what, i, ids[i], none, false, set);
    return rc;
}

__attribute__((noinline, cold)) static int orbu_refuse_slot(const orbu_store* s, const char* what, int i, int k, bool inside)
{
    if (!inside) return fail(ORBX_E_INVALID, "%s[%d] = %d outside the store of %d", what, i, k, s->kfcap);
    return fail(ORBX_E_INVALID, "%s[%d]: keyframe slot %d was never set", what, i, k);
}

// what[i] = k is a slot of the store.  set: the keyframe must have been set; none: -1 passes
__attribute__((always_inline)) static inline int orbu_check_slot(const orbu_store* s, const char* what, int i, int k, bool set, bool none = false)
{
    if (none && k == -1) return ORBX_OK;
    const bool inside = k >= 0 && k < s->kfcap;
    if (inside && (!set || s->kfSet[k])) return ORBX_OK;
    return orbu_refuse_slot(s, what, i, k, inside);
}

// ---- (the pool's mutex is held) the store's next generation tag, for kernels on stream st: what stamp, first and the
// families' mark words hold under an older tag reads as empty, so nothing is cleared between calls
static int orbu_next_generation(orbu_store* s, hipStream_t st, uint32_t* tag)
{
    if (s->gen == 0xffffffffu) {   // the tag wraps: one clear, and the tags start over
        const size_t bytes = (size_t)s->pool->cap * 8;
        HIPCHK(hipMemsetAsync(s->scr.stamp, 0, bytes, st));
        HIPCHK(hipMemsetAsync(s->scr.first, 0xff, bytes, st));
        for (int i = 0; i < s->nMarks; i++) HIPCHK(hipMemsetAsync(s->marks[i].p, 0, s->marks[i].bytes, st));
        s->gen = 0;
    }
    *tag = ++s->gen;
    return ORBX_OK;
}

// a family's block is about to be freed: its mark words leave the list (each family's *_blocks_ensure added them, once)
static void orbu_marks_drop(orbu_store* s, const void* p)
{
    for (int i = 0; i < s->nMarks; i++)
        if (s->marks[i].p == p) { s->marks[i] = s->marks[--s->nMarks]; return; }
}

// ---- (the pool's mutex is held) a device block made once: `bytes` filled with `fill` on the pool's stream and counted in
// nDevAlloc, or ORBX_E_HIP with nothing leaked and d null.  The store's columns and d_refKf, the families' fixed blocks
template <class T>
static int orbu_block_once(orbw_pool* p, T*& d, size_t bytes, int fill)
{
    if (d) return ORBX_OK;
    HIPCHK(hipMalloc((void**)&d, bytes));
    p->h->nDevAlloc++;
    hipError_t e = hipMemsetAsync(d, fill, bytes, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) { (void)hipFree(d); d = nullptr; return fail(ORBX_E_HIP, "clearing a block of the store failed: %s", hipGetErrorString(e)); }
    return ORBX_OK;
}

// (the pool's mutex is held) every set keyframe has the columns the call reads.  (Inlined by force, as the checkers above: a walk
// over every slot a call, which the callers' constants cut down to the columns they ask for.)
__attribute__((always_inline)) static inline int orbu_check_columns(const orbu_store* s, bool desc, bool ctr, bool oct)
{
    for (int k = 0; k < s->hi; k++) {
        if (!s->kfSet[k]) continue;
        if (desc && !s->desc.has[k]) return fail(ORBX_E_INVALID, "keyframe slot %d has no descriptors (orbu_kf_set_descriptors)", k);
        if (ctr && !s->ctr.has[k]) return fail(ORBX_E_INVALID, "keyframe slot %d has no centre (orbu_kf_set_centres)", k);
        if (oct && !s->oct.has[k]) return fail(ORBX_E_INVALID, "keyframe slot %d has no octaves (orbu_kf_set_octaves)", k);
    }
    return ORBX_OK;
}

#include "orbx_lastwins.hpp"   // stage_last_wins: the last record of a repeated key wins, under the setters; first_repeated_key
