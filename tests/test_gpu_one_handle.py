"""Every entry that packs its call into a matcher handle's S_BLOCK and stages through its h_stage, the solvers made on a handle and
five older entries, interleaved on ONE handle (tests/one_handle_cases.py; DESIGN.md "Scratch blocks have names").  The expected bytes of
a call are those of the same call on a rig made for it alone -- a fresh matcher, a fresh world, then closed -- which are first held to
the entry's restatement where it has one.  No tolerance anywhere: everything is tobytes() equality.  A fresh hipMalloc is usually zero
and an entry's own earlier calls leave plausible bytes, so an entry that reads a word before writing it, a download that lands where
the next upload is staged, or a result region cleared only by luck shows only in company: behind a larger call of another family.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import threading

import numpy as np
import pytest

import one_handle_cases as oh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(gpu, oracle):
    """(name, size, index) -> the chunks of the call on a rig made for it alone, held to the restatement"""
    from orbslamm_amd import ORBextractor
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=oh.rc.W, max_height=oh.rc.H, max_batch=1, device=0)
    out = {}
    for c in oh.TABLE:
        rig = oh.Rig(oracle, gex)
        out[oh.key(c)] = rig.run(c)
        rig.close()
        if c.ref:
            ref = c.ref(oracle)
            assert set(ref) <= set(out[oh.key(c)]), (c.name, c.size)
            assert oh.first_difference(out[oh.key(c)], ref) is None, (c.name, c.size, "alone against the restatement", oh.first_difference(out[oh.key(c)], ref))
    gex.close()
    assert len({oh.joined(v) for v in out.values()}) > len(out) * 3 // 4      # (the calls do compute something: few results coincide)
    return out


@pytest.fixture(scope="module")
def H(gpu, oracle):
    rig = oh.Rig(oracle)
    yield rig
    rig.close()


def check(rig, c, want, tag):
    got = rig.run(c)
    w = want[oh.key(c)]
    assert oh.first_difference(got, w) is None and oh.joined(got) == oh.joined(w), (c.name, c.size, tag, oh.first_difference(got, w))


def run_all(rig, calls, want, tag):
    for i, c in enumerate(calls):
        check(rig, c, want, (tag, i, "behind", calls[i - 1].name if i else None, calls[i - 1].size if i else None))


def test_large_small_large_forwards_then_backwards(H, want):
    """the first pass leaves foreign bytes over every offset a small call uses; the last pass grows nothing"""
    for order in (1, -1):
        run_all(H, oh.size_order()[::order], want, "forwards" if order > 0 else "backwards")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_schedules(H, want, seed):
    run_all(H, oh.schedule(seed), want, ("schedule", seed))


def test_arena_overflows_in_the_middle_of_a_schedule(H, want):
    """a job's share of each candidate arena set to 64 entries before a relocalisation and before a motion-model call: the call runs its
    chain again behind the overflow and returns the unconstrained call's bytes; the grown arenas stay, and every later call is unchanged"""
    from orbslamm_amd.track_pose import debug_motion_arena, debug_reloc_arena
    sched = oh.schedule(2)
    run_all(H, sched[:20], want, "before")
    reloc, motion = oh.of("relocalize_raw", "large")[0], oh.of("track_motion_model", "large")[0]
    debug_reloc_arena(H.m, 64)
    check(H, reloc, want, "arena share 64")
    assert debug_reloc_arena(H.m) >= 2, "the relocalisation ran again behind the overflow"
    debug_motion_arena(H.m, 64)
    check(H, motion, want, "arena share 64")
    assert debug_motion_arena(H.m) >= 2, "the motion-model call ran again behind the overflow"
    run_all(H, sched[20:] + oh.of("relocalize_raw") + oh.of("track_motion_model"), want, "behind the grown arenas")
    assert debug_reloc_arena(H.m) == 1 and debug_motion_arena(H.m) == 1, "the grown arenas hold the calls that made them grow"


def test_a_block_entry_between_prepare_and_search_voids_the_hint(H, want):
    """ProjectionPrepare, one S_BLOCK entry, the search: the hint is dropped and the search uploads its own train side.  Which side
    the search read shows in its bytes once the arrays have changed in place behind the prepare: with nothing between, the
    search reads what was prepared (the hint is for the very next call); with an entry between, what the arrays hold now"""
    old = dict(oh._old_case(700))
    then = dict(old, pc=dict(old["pc"], tk=old["pc"]["tk"].copy(), td=old["pc"]["td"].copy()))
    now = dict(old, pc=dict(old["pc"], tk=np.ascontiguousarray(old["pc"]["tk"][::-1]), td=np.ascontiguousarray(old["pc"]["td"][::-1])))
    alone = oh.Rig()
    w_then, w_now = (oh.joined(oh.chunks(*oh.flat(oh.proj_search(alone.m, o)))) for o in (then, now))
    alone.close()
    assert w_then != w_now

    def prepared_search(between):
        live = dict(old, pc=dict(old["pc"], tk=then["pc"]["tk"].copy(), td=then["pc"]["td"].copy()))
        H.m.ProjectionPrepare(live["g"], live["pc"]["tk"], live["pc"]["td"])
        for c in between:
            check(H, c, want, "between prepare and search")
        live["pc"]["tk"][:] = now["pc"]["tk"]
        live["pc"]["td"][:] = now["pc"]["td"]
        return oh.joined(oh.chunks(*oh.flat(oh.proj_search(H.m, live))))
    assert prepared_search([]) == w_then, "nothing between: the prepared train side is the one searched"
    for c in oh.of("pose_optimize_raw host arrays", "small") + oh.of("relocalize_raw", "large") + oh.of("view_project", "small"):
        assert prepared_search([c]) == w_now, (c.name, "the hint outlived an S_BLOCK entry")


def test_a_legacy_projection_search_behind_an_orbq_chain(H, want):
    """the matches and orbm_last_search_stats (T_STATS: the candidate counter every resolve leaves zero) are the alone handle's"""
    old = oh._old_case(700)
    alone = oh.Rig()
    w = oh.joined(oh.chunks(*oh.flat(oh.proj_search(alone.m, old))))
    w_stats = alone.m.last_search_stats()
    alone.close()
    assert w_stats[1] > 0
    for size in ("large", "small"):
        run_all(H, [oh.of(n, size)[0] for n in oh.TRACKING], want, "the chain")
        assert oh.joined(oh.chunks(*oh.flat(oh.proj_search(H.m, old)))) == w, size
        assert H.m.last_search_stats() == w_stats, (size, H.m.last_search_stats(), w_stats)


def test_a_regrown_staging_block_takes_its_flag_word_along(gpu, oracle, want):
    """on a handle of its own: small users of stage_down_wait (stageSeq counts up, the flag word lies behind a 64 KB block), then the
    call whose staging need exceeds everything before it, directly followed by those users again"""
    rig = oh.Rig(oracle)
    users = oh.of("match_bruteforce", "small") + oh.of("search_by_projection prepared", "small")
    run_all(rig, users + users, want, "before")
    run_all(rig, oh.of("view_project_frame", "small"), want, "a small S_BLOCK entry")
    for big in oh.of("view_project", "large") + oh.of("track_motion_model", "large") + oh.of("fuse_batch", "large"):
        grown = oh.alloc_stats(rig.m)[1]
        rig.world(big)                      # (the pool's setter stages its records through h_stage as well: 2 008 records regrow it)
        run_all(rig, users, want, ("behind the world of", big.name))
        check(rig, big, want, "the large call")
        if big.name == "view_project":      # the records, or else the 95 000 bytes that 5 000 queries bring down, are above the block's 64 KB
            assert oh.alloc_stats(rig.m)[1] > grown, "h_stage was regrown"
        run_all(rig, users, want, ("behind", big.name))
    rig.close()


def test_steady_state(H, want):
    """after one full pass, a second identical pass leaves the handle's device and host allocation counters unchanged (the solvers'
    own blocks do not count there: each solver call of the table runs its object twice and compares)"""
    run_all(H, oh.size_order(("large", "small")), want, "first pass")
    before = oh.alloc_stats(H.m)
    run_all(H, oh.size_order(("large", "small")), want, "second pass")
    assert oh.alloc_stats(H.m) == before, (before, oh.alloc_stats(H.m))


def test_two_threads_two_rigs(gpu, oracle, want):
    """seeded schedule 1 on two rigs at once, each with its own world: the process-wide parts (the shared chain-stream pool,
    hipFuncSetAttribute bookkeeping, the last-error text) held to the same bytes"""
    failures = []

    def work(k):
        try:
            rig = oh.Rig(oracle)
            run_all(rig, oh.schedule(1), want, ("thread", k))
            rig.close()
        except BaseException as e:      # (an assertion in a thread is the test's to report)
            failures.append((k, repr(e)[:2000]))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
