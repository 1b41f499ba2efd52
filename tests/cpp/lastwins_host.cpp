// stage_last_wins (orbslamm_amd/csrc/orbx_lastwins.hpp) on the host alone, with in-memory emit and flush: every form the three
// setters use it in, held to "the last record of a key wins" computed directly; built with -fsanitize=address,undefined by
// tests/test_localmap_update_cpu.py.  A flush stores its survivors into `table` as the scatter kernels do: later launches land last.
// first_repeated_key of the same header: no repeat, a repeat at index 1 and at the last index, keys on both sides of a word, n = 0.
#include "../../orbslamm_amd/csrc/orbx_lastwins.hpp"

#include <cstdio>
#include <cstdlib>

static int run(int nkeys, int n, int window, int perLaunch, int failAt, unsigned seed)
{
    std::vector<int32_t> keys((size_t)n), want((size_t)nkeys, -1), table((size_t)nkeys, -1);
    for (int i = 0; i < n; i++) { seed = seed * 1664525u + 1013904223u; keys[i] = (int32_t)((seed >> 8) % (unsigned)nkeys); want[keys[i]] = i; }
    std::vector<uint64_t> seen(((size_t)nkeys + 63) / 64, 0);
    std::vector<int32_t> stage((size_t)perLaunch * 2, -7);   // exactly perLaunch survivors: one more is an overrun the sanitizer sees
    int launches = 0, most = 0;
    auto emit = [&](int i, int m) { stage[(size_t)m * 2] = keys[i]; stage[(size_t)m * 2 + 1] = i; };
    auto flush = [&](int m) -> int {
        if (m <= 0 || m > perLaunch) { fprintf(stderr, "a launch of %d survivors, at most %d\n", m, perLaunch); exit(1); }
        if (launches == failAt) return -3;
        for (int q = 0; q < m; q++) table[stage[(size_t)q * 2]] = stage[(size_t)q * 2 + 1];
        launches++; most = std::max(most, m);
        return 0;
    };
    const int rc = stage_last_wins(keys.data(), n, window, perLaunch, seen, emit, flush);
    for (uint64_t w : seen) if (w) { fprintf(stderr, "the scratch is not zero on exit (rc %d)\n", rc); exit(1); }
    if (failAt >= 0) { if (rc != -3 || launches != failAt) { fprintf(stderr, "a failing flush: rc %d after %d launches\n", rc, launches); exit(1); } return launches; }
    if (rc != 0 || table != want) { fprintf(stderr, "keys %d n %d window %d perLaunch %d: rc %d, the table differs\n", nkeys, n, window, perLaunch, rc); exit(1); }
    return launches;
}

// first_repeated_key over `keys`: the index it must return, and the scratch zero behind it
static void repeat(std::initializer_list<int32_t> keys, int want)
{
    std::vector<uint64_t> seen(2, 0);   // keys below 128: 63 and 64 lie in two words
    const int got = first_repeated_key(keys.begin(), (int)keys.size(), seen);
    if (got != want) { fprintf(stderr, "first_repeated_key over %zu keys: %d, not %d\n", keys.size(), got, want); exit(1); }
    for (uint64_t w : seen) if (w) { fprintf(stderr, "first_repeated_key over %zu keys leaves the scratch set\n", keys.size()); exit(1); }
}

int main()
{
    repeat({}, -1);                          // n = 0
    repeat({5}, -1);
    repeat({3, 1, 4, 15, 9, 2, 6}, -1);      // no repeat
    repeat({7, 7, 1, 2}, 1);                 // at index 1
    repeat({3, 1, 4, 15, 9, 2, 4}, 6);       // at the last index
    repeat({3, 1, 3, 1, 3}, 2);              // the first of several
    repeat({63, 64}, -1);                    // bit 63 of one word, bit 0 of the next: not each other's
    repeat({63, 64, 0, 127, 64}, 4);
    repeat({64, 63, 63}, 2);
    int total = 0;
    // the pool's and the pair setters' form: window == perLaunch; a repeated key on both sides of a window's end; n a multiple and not
    for (int n : {1, 7, 64, 65, 128, 1000}) for (int per : {1, 8, 64}) total += run(13, n, per, per, -1, (unsigned)(n * 31 + per));
    // orbu_kf_write's form: one window over the call, more survivors than a launch holds, so the flush INSIDE the window runs
    for (int nkeys : {5, 64, 200}) for (int per : {1, 3, 64, 199, 200, 201}) {
        const int launches = run(nkeys, 1000, 1000, per, -1, (unsigned)(nkeys * 7 + per));
        if (nkeys == 200 && per == 3 && launches < 60) { fprintf(stderr, "%d launches for about 200 survivors of 3 a launch\n", launches); return 1; }
        total += launches;
    }
    // windows longer than a launch and shorter than the call
    total += run(100, 1000, 300, 7, -1, 5u);
    // a failing flush, inside a window and at its end, first and later: the call ends there with the scratch zero
    for (int failAt : {0, 1, 5}) { run(200, 1000, 1000, 3, failAt, 9u); run(13, 1000, 8, 8, failAt, 9u); }
    printf("lastwins ok: %d launches\n", total);
    return 0;
}
