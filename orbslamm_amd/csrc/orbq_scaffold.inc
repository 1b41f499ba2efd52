// orbq_scaffold.inc -- what the four pool-fed tracking entries share on the host (part of orbslamm_hip.hip, in front of orbq_host.inc,
// orbq_reloc_host.inc and orbq_motion_host.inc; DESIGN.md §8s "The scaffold").  In the order an entry runs through them: the argument
// checks that need no handle, a job's frame set, the solver block of orbq::Args, the candidate arena of the two replayed chains, and
// the tail behind the last launch.  An entry keeps what is its own: its extra checks, its packed layout, its job records, its launches.
// orbq_track_pose takes the argument checks and the solver block from here and keeps its own frame-set check and tail (orbq_host.inc).

// What every entry refuses alike, needing neither a handle nor a GPU (zero jobs are settled by the caller before this).  The entry's own
// checks come behind it, "null handle, pool or store" last.  `tables`: every level table the entry takes is there; `noTable` and
// `nullArray`: the entry's words for one that is not, and for a job's null array
template <class Job>
static int orbq_check_shared(const Job* jobs, int n_jobs, const void* out, int32_t* const* ids_out, uint8_t* const* outlier_out, bool tables, int nlevels,
                             const char* noTable, const char* nullArray)
{
    if (n_jobs < 0) return fail(ORBX_E_INVALID, "negative job count");
    if (n_jobs > ORBO_MAX_FRAMES) return fail(ORBX_E_UNSUPPORTED, "%d jobs: above %d", n_jobs, ORBO_MAX_FRAMES);
    if (!jobs || !out || !ids_out || !outlier_out) return fail(ORBX_E_INVALID, "null argument");
    if (!tables || nlevels < 1 || nlevels > ORBX_MAX_LEVELS) return fail(ORBX_E_INVALID, "nlevels %d outside [1, %d] or %s", nlevels, ORBX_MAX_LEVELS, noTable);
    int64_t total = 0;
    for (int j = 0; j < n_jobs; j++) {
        const Job& J = jobs[j];
        if (!J.fs) return fail(ORBX_E_INVALID, "job %d: null frame set", j);
        if (J.n < 0) return fail(ORBX_E_INVALID, "job %d: negative feature count", j);
        if (J.n > ORBO_MAX_EDGES) return fail(ORBX_E_UNSUPPORTED, "job %d: %d features: above %d", j, J.n, ORBO_MAX_EDGES);
        if (J.n && (!ids_out[j] || !outlier_out[j])) return fail(ORBX_E_INVALID, "job %d: %s", j, nullArray);
        total += J.n;
        if (total > ORBO_MAX_CALL_EDGES) return fail(ORBX_E_UNSUPPORTED, "more than %d features in one call (reached at job %d)", ORBO_MAX_CALL_EDGES, j);
    }
    return ORBX_OK;
}

// Job j's frame set as orbq_track_reference, orbq_relocalize and orbq_track_motion_model check it: alive, the handle's own, the two
// slots inside it (the entry's own argument checks have refused a negative one), no more features than a frame of it holds (nq: the
// job's second count, -1 where it has none), the caps added up into sumCap -- a search's scratch goes by the set's CAP whatever n is,
// so they are bounded like the features -- and, for a set that builds on a stream of its own, the end of the builds that may still
// run there.  (orbq_track_pose has one slot, no search scratch and synchronises only where back < 0: it keeps its own text.)
static int orbq_check_frameset(orbm_handle* h, orbm_frameset* fs, int j, int slotA, int slotB, int n, int nq, size_t& sumCap)
{
    int rc = frameset_check(fs);
    if (rc) return rc;
    if (fs->owner != h) return fail(ORBX_E_INVALID, "job %d: the frame set belongs to another handle", j);
    if (slotA >= fs->slots || slotB >= fs->slots) return fail(ORBX_E_INVALID, "job %d: slot %d or %d outside the frame set", j, slotA, slotB);
    if (nq < 0) {
        if (n > fs->cap) return fail(ORBX_E_INVALID, "job %d: %d features for a frame of at most %d", j, n, fs->cap);
    } else if (n > fs->cap || nq > fs->cap) return fail(ORBX_E_INVALID, "job %d: %d and %d features for frames of at most %d", j, n, nq, fs->cap);
    if ((sumCap += (size_t)fs->cap) > (size_t)ORBO_MAX_CALL_EDGES)
        return fail(ORBX_E_UNSUPPORTED, "the jobs' frame sets hold more than %d features together (reached at job %d)", ORBO_MAX_CALL_EDGES, j);
    if (fs_stream(fs) != h->stream) HIPCHK(hipStreamSynchronize(fs_stream(fs)));
    return ORBX_OK;
}

// The solver block of an entry's arguments from the offsets of its packed block `d`: the edge arrays and the sigma table of orbo's
// solve, the pool, and the per-feature arrays of the merge and the loop behind the solve
static void orbq_fill_solver(orbq::Args& q, const orbw_pool* pool, uint8_t* d, size_t oPw, size_t oUv, size_t oFlags, size_t oMerged, size_t oIds, size_t oOutl,
                             const float* inv_level_sigma2, int nlevels)
{
    q.o.pw = (float4*)(d + oPw); q.o.uv = (float2*)(d + oUv); q.o.outlier = d + oFlags;
    for (int lv = 0; lv < ORBX_MAX_LEVELS; lv++) q.o.invSigma2[lv] = lv < nlevels ? inv_level_sigma2[lv] : 0.f;
    q.o.nlevels = nlevels;
    q.pool = pool->dev;
    q.merged = (int32_t*)(d + oMerged); q.idsOut = (int32_t*)(d + oIds); q.outlierOut = d + oOutl;
}

// ------------------------------------------------------------------ the candidate arena of a replayed chain
// orbq_relocalize and orbq_track_motion_model search through an arena of which each job has a share (orbm_handle::CandArena).  A search
// that overflowed its share says how many entries it needed (orbq::report_overflow); the arena grows to the largest need and the WHOLE
// call runs again, twice at the most: for (attempt = 0;; attempt++) { orbq_arena_reserve ... orbq_drain ... orbq_arena_grow }.
constexpr int kArenaMax = 1 << 24;   // entries a job: what an orbq_debug_*_arena takes at the most
static inline int pow2ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// the body of an entry's orbq_debug_*_arena
static int orbq_debug_arena(orbm_t* h, orbm_handle::CandArena orbm_handle::*arena, int entries_per_job, int* last_runs)
{
    if (entries_per_job < -1 || entries_per_job > kArenaMax) return fail(ORBX_E_INVALID, "%d entries a job outside [-1, %d]", entries_per_job, kArenaMax);
    int rc = orbm_check(h);
    if (rc) return rc;
    if (entries_per_job >= 0) (h->*arena).entries = entries_per_job;
    if (last_runs) *last_runs = (h->*arena).runs;
    return ORBX_OK;
}

// run `attempt` of the chain starts: `entries` a job this run (`dflt` while nothing has set or grown the arena), reserved in `slot`
static int orbq_arena_reserve(orbm_handle* h, orbm_handle::CandArena& ar, OrbmSlot slot, int attempt, size_t n_jobs, size_t dflt, size_t& entries)
{
    ar.runs = attempt + 1;
    entries = ar.entries > 0 ? (size_t)ar.entries : dflt;
    return orbm_reserve(h, slot, n_jobs * entries * sizeof(uint2));
}

// ... and ends, behind orbq_drain: need[job][2] as it came down.  again: a search overflowed and the arena has grown to the largest
// need -- nothing but the call's own scratch has been written, the caller runs the chain again
static int orbq_arena_grow(orbm_handle::CandArena& ar, int attempt, const int32_t* need, int n_jobs, bool& again)
{
    int maxNeed = 0;
    for (int j = 0; j < n_jobs; j++) maxNeed = std::max(maxNeed, std::max(need[2 * j], need[2 * j + 1]));
    again = maxNeed > 0;
    if (!again) return ORBX_OK;
    if (attempt == 2) return fail(ORBX_E_CAPACITY, "candidate arena overflow: %d entries a job asked for in the third run", maxNeed);
    if (maxNeed > kArenaMax) return fail(ORBX_E_CAPACITY, "candidate arena overflow: %d entries a job", maxNeed);
    ar.entries = maxNeed;
    return ORBX_OK;
}

// ------------------------------------------------------------------ the tail behind the last launch
// The copy down of what lies in one piece from dDown, the reader mark, the synchronise.  The pool's mutex is the caller's and the kernels
// in flight read the pool: whatever fails here, the stream is drained before the error is handed back and the mutex let go.  Then the
// refusal the kernels ask for: rounds < 0 in a job's record (rec: the records as they came down, an OrboResult at the head of each;
// alsoRefused: what else the entry's merge refuses that way, for the message)
static int orbq_drain(const char* entry, orbw_pool* pool, hipStream_t s, void* hs, const void* dDown, size_t downBytes, const void* rec, size_t recBytes,
                      int n_jobs, int nlevels, const char* alsoRefused)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hs, dDown, downBytes, hipMemcpyDeviceToHost, s);
    const int rcMark = orbw_mark_reader(pool, s);
    const hipError_t eSync = hipStreamSynchronize(s);
    if (e == hipSuccess) e = eSync;
    if (e != hipSuccess) return fail(ORBX_E_HIP, "%s's chain failed: %s", entry, hipGetErrorString(e));
    if (rcMark) return rcMark;
    for (int j = 0; j < n_jobs; j++)
        if (((const OrboResult*)((const uint8_t*)rec + (size_t)j * recBytes))->rounds < 0)
            return fail(ORBX_E_INVALID, "job %d: an edge's octave lies outside [0, %d), or a feature at or above the slot's device count%s holds a point", j, nlevels, alsoRefused);
    return ORBX_OK;
}

// ... and what an entry hands back behind it: the records, and per job its n ids and outlier bytes from where they lie in the pinned block
template <class Job>
static void orbq_hand_back(const Job* jobs, int n_jobs, void* out, const void* rec, size_t recBytes, const uint8_t* ids, const uint8_t* outl,
                           int32_t* const* ids_out, uint8_t* const* outlier_out)
{
    memcpy(out, rec, (size_t)n_jobs * recBytes);
    size_t f0 = 0;
    for (int j = 0; j < n_jobs; j++) {
        const size_t n = (size_t)jobs[j].n;
        if (n) { memcpy(ids_out[j], ids + f0 * 4, n * 4); memcpy(outlier_out[j], outl + f0, n); }
        f0 += n;
    }
}
