"""The correction of LoopClosing::CorrectLoop / MultiMapper::UpdatePosesAndAdd on the device (orbe_*): every field
of every record of orbe_correct_sim3 against the restatement (tools/correct_ref.hpp), each call made twice, over every scene
family; K of 1, 63, 64, 65 and all of a 130 x 256 store; points of 17 .. 40 observers; the 1 024 / 1 025 observer boundary;
commit = 0 against orbw_debug_pool_get; what a commit writes and what it leaves; a shuffled list; ORBX_E_CAPACITY; a forced
generation wrap with the other entries around it; orbu_point_set_ref_kf; the refusals; the drop-in against the two loops written
serially.  Floats are compared as bytes, with no exclusions: the scenes give no NaN.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import ctypes as C

import numpy as np
import pytest

import correct_cases as cs
import dropin
import refresh_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.8, True, device=0)


def load(matcher, c, refs=True):
    """the scene in a pool and a store beside it, mpRefKF resident"""
    from orbslamm_amd import KeyFrameStore, MapPool
    r, s = c.r, c.s
    pool = MapPool(matcher, s.pool_cap)
    pool.set(np.arange(s.pool_cap), r.pool_records())
    store = KeyFrameStore(pool, s.kfcap, s.stride, 4, s.kfcap * s.stride)
    store.set(*s.records())
    slots = s.set_slots()
    for k in slots:
        store.set_octaves(k, s.octaves[k])
    store.set_centres(slots, r.centres[slots])
    if refs:
        store.set_ref_kf(np.arange(s.pool_cap), r.ref_kf)
    return pool, store


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(store, c, tag, slots=None, anchor=None, commit=False, turns=2):
    """the call against the restatement of the scene as it is now, twice; returns the restatement's records"""
    slots = c.slots if slots is None else np.asarray(slots, np.int32)
    anchor = c.anchor if anchor is None else anchor
    wkf, wpts, _ = cs.ref_correct(c, slots, anchor)
    for turn in range(turns):
        kf, pts = store.correct_sim3(slots, c.poses[slots], anchor, c.Scw, cs.SF, c.skip, commit)
        for name, got, want in (("kf", kf, wkf), ("points", pts, wpts)):
            assert len(got) == len(want), (tag, turn, name, len(got), len(want))
            if not same(got, want):
                i = next(k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes())
                bad = [n for n in got.dtype.names if got[n][i].tobytes() != want[n][i].tobytes()]
                raise AssertionError((tag, turn, name, i, bad, got[i], want[i]))
    return wkf, wpts


@pytest.mark.parametrize("family", sorted(cs.FAMILIES))
def test_every_family_equals_the_restatement(matcher, family):
    for seed in (1, 2):
        c = cs.family_scene(family, seed)
        pool, store = load(matcher, c)
        _, pts = check(store, c, (family, seed))
        assert len(pts) > 0
        store.close()
        pool.close()


@pytest.fixture(scope="module")
def dense(matcher):
    c = cs.dense_scene()
    pool, store = load(matcher, c)
    yield c, pool, store
    store.close()
    pool.close()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 0])
def test_list_sizes_around_a_workgroup_and_the_whole_store(matcher, dense, K):
    c, pool, store = dense
    rng = np.random.default_rng(10 + K)
    slots = c.s.set_slots() if K == 0 else rng.permutation(c.s.set_slots())[:K]
    slots = rng.permutation(slots)
    kf, pts = check(store, c, ("K", K), slots, int(rng.integers(len(slots))))
    assert len(kf) == (130 if K == 0 else K) and len(pts) > 100 and kf["n_points"].sum() == len(pts)


def test_points_of_17_to_40_observers_take_the_long_path(matcher):
    c = cs.observer_scene()
    pool, store = load(matcher, c)
    _, pts = check(store, c, "observers")
    for n in (16, 17, 18, 31, 32, 33, 40):
        o = pts[pts["id"] == c.named["n%d" % n]][0]
        assert o["n_obs"] == n
    assert (pts["status"] == cs.ST_DONE).sum() > 40
    store.close()
    pool.close()


def test_the_observation_ceiling_and_its_refusal(matcher):
    from orbslamm_amd import map_pool as mp
    from orbslamm_amd._lib import ORBX_E_UNSUPPORTED, lib, ptr
    c = cs.long_scene(rc.MAX_OBS)
    pool, store = load(matcher, c)
    _, pts = check(store, c, "1 024 observers")
    assert pts[pts["id"] == c.named["p"]][0]["n_obs"] == rc.MAX_OBS
    store.close()
    pool.close()
    c = cs.long_scene(rc.MAX_OBS + 1)
    pool, store = load(matcher, c)
    ids = np.arange(c.pool_cap, dtype=np.int32)
    before, K = pool.debug_get(ids), len(c.slots)
    kf, pts, n = np.zeros(K, mp.CORRECT_KF_DTYPE), np.zeros(c.pool_cap, mp.CORRECT_POINT_DTYPE), C.c_int(-77)
    kf.view(np.uint8)[:] = 0xAB
    pts.view(np.uint8)[:] = 0xCD
    Tiw, skip = c.Tiw, np.zeros(0, np.int32)
    code = lib().orbe_correct_sim3(store._h, ptr(c.slots), ptr(Tiw), K, c.anchor, ptr(c.Scw), ptr(skip), 0, ptr(cs.SF), cs.NLEVELS, 1, ptr(kf), ptr(pts), len(pts),
                                   C.byref(n))
    assert code == ORBX_E_UNSUPPORTED and b"observations" in lib().orbx_last_error()
    assert (kf.view(np.uint8) == 0xAB).all() and (pts.view(np.uint8) == 0xCD).all() and n.value == -77      # refused: nothing written
    assert pool.debug_get(ids).tobytes() == before.tobytes()
    rest = ids[ids != c.named["p"]][:30]
    got = store.refresh_points(rest, c.r.ref_kf[rest], cs.SF, rc.NORMAL_DEPTH, None, False)                 # ... nor to the centres
    assert rc.same_records(got, rc.Ref(c.r).refresh(rest, c.r.ref_kf[rest], rc.NORMAL_DEPTH))
    c.skip = np.array([c.named["p"]], np.int32)                       # without the point above the ceiling the call goes through
    check(store, c, "the point above the ceiling skipped", commit=False)
    store.close()
    pool.close()


def test_what_a_commit_writes_and_what_it_leaves(matcher):
    c = cs.family_scene("random", 4)
    r = c.r
    pool, store = load(matcher, c)
    for k in r.s.set_slots():
        store.set_descriptors(k, r.desc[k])
    ids = np.arange(c.pool_cap, dtype=np.int32)
    before = pool.debug_get(ids)
    assert before.tobytes() == r.pool_records().tobytes()
    check(store, c, "compute only", commit=False)
    assert pool.debug_get(ids).tobytes() == before.tobytes()         # commit = 0 leaves every record as it was
    plain = rc.Ref(r).refresh(ids, r.ref_kf, rc.BOTH)
    assert rc.same_records(store.refresh_points(ids, r.ref_kf, rc.SF, rc.BOTH, None, False), plain)      # ... and every centre
    wkf, wpts = check(store, c, "commit", commit=True, turns=1)
    c.apply(wkf, wpts)
    after = pool.debug_get(ids)
    assert after.tobytes() == r.pool_records().tobytes()             # positions, the DONE points' normals and bounds; every other byte as it was
    assert same(after["flags"], before["flags"]) and same(after["desc"], before["desc"]) and not same(after["pos"], before["pos"])
    moved = np.zeros(c.pool_cap, bool)
    moved[wpts["id"]] = True
    assert same(after[~moved], before[~moved]) and (wpts["status"] != cs.ST_DONE).any()
    # the new centres are what a following orbr_refresh_points reads, the unlisted keyframes' centres what they were, the
    # descriptors in the store untouched: the restatement of the scene after apply() has exactly those
    got = store.refresh_points(ids, r.ref_kf, rc.SF, rc.BOTH, None, False)
    want = rc.Ref(r).refresh(ids, r.ref_kf, rc.BOTH)
    assert rc.same_records(got, want) and not rc.same_records(want, plain)
    check(store, c, "a second correction from the committed state", commit=False)
    store.close()
    pool.close()


def test_a_shuffled_list_gives_the_same_bytes(matcher):
    c = cs.family_scene("several_holders_shuffled", 3)
    pool, store = load(matcher, c)
    kf, pts = check(store, c, "as listed")
    perm = np.random.default_rng(11).permutation(len(c.slots))
    kf2, pts2 = check(store, c, "shuffled", c.slots[perm], int(np.flatnonzero(perm == c.anchor)[0]))
    assert same(kf[perm], kf2) and same(pts, pts2)
    store.close()
    pool.close()


def test_capacity_is_refused_with_the_needed_count_and_nothing_written(matcher):
    from orbslamm_amd import map_pool as mp
    from orbslamm_amd._lib import ORBX_E_CAPACITY, ORBX_OK, lib, ptr
    c = cs.family_scene("random", 5)
    pool, store = load(matcher, c)
    _, wpts = check(store, c, "whole")
    ids = np.arange(c.pool_cap, dtype=np.int32)
    before, K, need = pool.debug_get(ids), len(c.slots), len(wpts)
    Tiw, skip = c.Tiw, np.zeros(0, np.int32)
    for cap in (0, need - 1):
        kf, pts, n = np.zeros(K, mp.CORRECT_KF_DTYPE), np.zeros(max(cap, 1), mp.CORRECT_POINT_DTYPE), C.c_int(-77)
        kf.view(np.uint8)[:] = 0xAB
        pts.view(np.uint8)[:] = 0xCD
        code = lib().orbe_correct_sim3(store._h, ptr(c.slots), ptr(Tiw), K, c.anchor, ptr(c.Scw), ptr(skip), 0, ptr(cs.SF), cs.NLEVELS, 1, ptr(kf),
                                       ptr(pts) if cap else None, cap, C.byref(n))
        assert code == ORBX_E_CAPACITY and n.value == need
        assert (kf.view(np.uint8) == 0xAB).all() and (pts.view(np.uint8) == 0xCD).all() and pool.debug_get(ids).tobytes() == before.tobytes()
    kf, pts = store.correct_sim3(c.slots, c.Tiw, c.anchor, c.Scw, cs.SF, c.skip, False, pts_cap=need)      # exactly enough
    assert same(pts, wpts)
    check(store, c, "after the refusals")
    store.close()
    pool.close()


def test_a_forced_generation_wrap_with_the_other_entries_around_it(matcher):
    from orbslamm_amd.map_pool import Connections
    c = cs.family_scene("random", 7)
    r = c.r
    pool, store = load(matcher, c)
    ids, tg = np.arange(c.pool_cap, dtype=np.int32), r.s.set_slots()
    frame = np.random.default_rng(9).integers(0, 600, 150).astype(np.int32)

    def others():
        u = store.update(frame)
        k = store.update_connections(tg)
        p = store.refresh_points(ids, r.ref_kf, rc.SF, rc.NORMAL_DEPTH, None, False)
        return [np.array([u.status, u.kf_max, u.nkf, u.nL, u.nS], np.int32), u.kf.copy(), u.L.copy(), u.seen.copy(), p.view(np.uint8)] + \
               [getattr(k, n) for n in Connections.NAMES]

    want = others()
    check(store, c, "before the wrap")
    store.debug_set_generation(0xffffffff - 1)                      # the next call takes the last tag, the one behind it wraps
    check(store, c, "across the wrap")
    for x, y in zip(want, others()):
        assert np.array_equal(x, y)
    store.debug_set_generation(0xffffffff)
    check(store, c, "at the wrap", turns=1)
    for x, y in zip(want, others()):
        assert np.array_equal(x, y)
    check(store, c, "after the wrap")
    store.close()
    pool.close()


def test_the_resident_reference_keyframes(matcher):
    from orbslamm_amd._lib import ORBX_E_INVALID, OrbError
    c = cs.family_scene("ref_higher_rank", 6)
    r = c.r
    pool, store = load(matcher, c, refs=False)
    true_refs = r.ref_kf.copy()
    r.ref_kf[:] = -1                                                 # never set: every id -1
    _, pts = check(store, c, "no reference keyframe set")
    assert (pts["status"] != cs.ST_DONE).all() and (pts["status"] == cs.ST_NO_REF).any()
    r.ref_kf[:] = true_refs
    pt = c.named["p"]
    ids = np.concatenate([np.arange(c.pool_cap), [pt, pt]]).astype(np.int32)      # a repeated id takes the last value
    store.set_ref_kf(ids, np.concatenate([r.ref_kf, [cs.T0 + 5, r.ref_kf[pt]]]))
    _, pts = check(store, c, "set, the last value of a repeated id")
    assert pts[pts["id"] == pt][0]["status"] == cs.ST_DONE
    store.set_ref_kf([pt, pt], [r.ref_kf[pt], -1])
    r.ref_kf[pt] = -1
    _, pts = check(store, c, "back to -1")
    assert pts[pts["id"] == pt][0]["status"] == cs.ST_NO_REF
    free = int(np.flatnonzero((r.s.kf_flags & cs.KF_SET) == 0)[0])
    store.set_ref_kf([pt], [free])                                    # an unset slot inside the store is a keyframe that does not observe
    r.ref_kf[pt] = free
    check(store, c, "an unset slot")
    for ids, ks in (([c.pool_cap], [0]), ([-1], [0]), ([0], [c.kfcap]), ([0], [-2])):
        with pytest.raises(OrbError) as e:
            store.set_ref_kf(ids, ks)
        assert e.value.code == ORBX_E_INVALID
    store.set_ref_kf([], [])
    check(store, c, "after the refusals")
    got = store.refresh_points([pt], [cs.T0 + 4], rc.SF, rc.NORMAL_DEPTH, None, False)      # orbr_refresh_points reads its own argument, not the array
    assert got[0]["st_normal_depth"] == rc.ST_DONE
    store.close()
    pool.close()


def test_the_refusals_with_a_store(matcher):
    from orbslamm_amd._lib import ORBX_E_INVALID, OrbError
    c = cs.family_scene("one_holder", 8)
    r = c.r
    slots = r.s.set_slots()
    free = int(np.flatnonzero((r.s.kf_flags & cs.KF_SET) == 0)[0])
    ids = np.arange(c.pool_cap, dtype=np.int32)
    pool, store = load(matcher, c)
    before = pool.debug_get(ids)
    T = lambda s: c.poses[np.clip(np.asarray(s), 0, c.kfcap - 1)]
    for s_, why in (([slots[0], free], "unset"), ([slots[0], c.kfcap], "out of range"), ([slots[0], -1], "negative"), ([slots[0], slots[1], slots[0]], "repeated")):
        with pytest.raises(OrbError) as e:
            store.correct_sim3(s_, T(s_), 0, c.Scw, cs.SF)
        assert e.value.code == ORBX_E_INVALID, why
    for skip in ([c.pool_cap], [-1]):
        with pytest.raises(OrbError) as e:
            store.correct_sim3(c.slots, c.Tiw, c.anchor, c.Scw, cs.SF, skip)
        assert e.value.code == ORBX_E_INVALID
    assert pool.debug_get(ids).tobytes() == before.tobytes()
    check(store, c, "after the refusals")
    store.close()
    pool.close()
    from orbslamm_amd import KeyFrameStore, MapPool
    pool = MapPool(matcher, 64)                                       # a pool with unset ids; a store whose keyframes lack centres, then octaves
    pool.set(np.arange(32), r.pool_records()[:32])
    store = KeyFrameStore(pool, 4, 8, 4, 32)
    none = [np.zeros(0, np.int32)] * 2
    store.set([0, 1], [0, 0], [np.arange(4, dtype=np.int32), np.arange(4, 8, dtype=np.int32)], none, [-1, -1], none)
    eye = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (2, 1))
    for step in ("no centre", "no octaves", "skip id never set"):
        with pytest.raises(OrbError) as e:
            store.correct_sim3([0, 1], eye, 0, c.Scw, cs.SF, [40] if step == "skip id never set" else [])
        assert e.value.code == ORBX_E_INVALID and (step == "skip id never set" or step in str(e.value)), (step, str(e.value))
        if step == "no centre":
            store.set_centres([0, 1], np.zeros((2, 3), np.float32) + 9)
        elif step == "no octaves":
            for k in (0, 1):
                store.set_octaves(k, np.zeros(8, np.uint8))
    kf, pts = store.correct_sim3([0, 1], eye, 0, c.Scw, cs.SF, [3])
    assert len(pts) == 7 and 3 not in pts["id"]
    store.close()
    pool.close()


def test_the_dropin_equals_the_loops_written_serially(matcher, gpu):
    """tests/cpp/correct_dropin_gpu.cpp: CorrectLoopPosesT::Run over the mocks against LoopClosing.cc:455-524 and
    MultiMapper.cc:523-595 written serially on the same mocks, their maps ordered by mnId"""
    dropin.run(dropin.build("correct_dropin_gpu", pthread=False), timeout=120, marker="correct drop-in: ok")
