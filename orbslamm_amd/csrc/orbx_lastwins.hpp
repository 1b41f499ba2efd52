// orbx_lastwins.hpp -- the two walks over a call's keys and a bit vector: the last-wins staging under orbw_pool_write, orbu_kf_write
// and orbu_pairs_write, and the first repeated key of a call that takes each once (orbx_poolutil.inc includes it).  Plain C++ with
// no HIP in it, so tests/cpp/lastwins_host.cpp runs it on the host alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// The last record of a repeated key wins.  Records [0, n) are taken in windows of `window`; a window is walked backwards
// and only a key's first sighting, its last record, is staged: emit(i, m) writes record i as survivor m of the pinned staging,
// flush(m) launches the scatter over m survivors on the pool's stream and synchronises (the staging is the next launch's; the
// call returns with the update complete).  `seen`: one bit per key, all zero on entry and on exit, a failing flush (a return other than 0, which ends the call) included.
// Launches follow each other on one stream, so among windows the later one's record lands last as well: a window may be as
// short as one launch's staging (the pool's and the pair setters: window = perLaunch) or the whole call (orbu_kf_write: its
// records are large and its keys few, so it stages each slot once and needs a launch per perLaunch SURVIVORS).  Both are the
// same function of the input; within a window no key is staged twice, so the order of its launches does not matter.
template <class Emit, class Flush>
static int stage_last_wins(const int32_t* keys, int n, int window, int perLaunch, std::vector<uint64_t>& seen, Emit emit, Flush flush)
{
    int rc = 0;
    for (int c0 = 0, c1; c0 < n && !rc; c0 = c1) {
        c1 = c0 + std::min(window, n - c0);
        int m = 0;
        for (int i = c1 - 1; i >= c0 && !rc; i--) {
            uint64_t& w = seen[(size_t)keys[i] >> 6];
            const uint64_t bit = 1ull << (keys[i] & 63);
            if (w & bit) continue;
            w |= bit;
            emit(i, m);
            if (++m == perLaunch) { rc = flush(m); m = 0; }
        }
        for (int i = c0; i < c1; i++) seen[(size_t)keys[i] >> 6] = 0;
        if (m && !rc) rc = flush(m);
    }
    return rc;
}

// A key repeated within a call that takes each at most once (orbr_refresh_points' ids, orbe_correct_sim3's slots): the index of
// the first key that an earlier one equals, or -1.  `seen` as above: all zero on entry and on exit.  (Inlined by force: the walk
// runs once per key of the call and stands where the callers' own loops stood.)
__attribute__((always_inline)) static inline int first_repeated_key(const int32_t* keys, int n, std::vector<uint64_t>& seen)
{
    int dup = -1;
    for (int i = 0; i < n && dup < 0; i++) {
        uint64_t& w = seen[(size_t)keys[i] >> 6];
        const uint64_t bit = 1ull << (keys[i] & 63);
        if (w & bit) dup = i;
        w |= bit;
    }
    for (int i = 0; i < n; i++) seen[(size_t)keys[i] >> 6] = 0;
    return dup;
}
