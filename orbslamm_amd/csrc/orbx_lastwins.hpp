// orbx_lastwins.hpp -- the last-wins staging under orbw_pool_write, orbu_kf_write and orbu_pairs_write (orbx_poolutil.inc includes
// it).  Plain C++ with no HIP in it, so tests/cpp/lastwins_host.cpp runs it on the host alone under the sanitizers.
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
