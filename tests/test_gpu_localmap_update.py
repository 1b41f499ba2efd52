"""Tracking::UpdateLocalMap on the device (orbu_*): every output array of orbu_update_local_map / orbu_local_points
against the restatement (tools/localmap_update_ref.hpp), element for element, over every scene family, the keyframe counts 0, 1,
63, 64, 65 and 300, the strides 64, 65 and 2 048, voted groups on both sides of the `> 80` test, walks that end one entry before
and one entry behind a compaction chunk, the capacity edge, a forced generation wrap, the setters' semantics, two stores on one
pool, and the search from the resident list against orbw_track_local_map given the restatement's S.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import numpy as np
import pytest

import dropin
import localmap_cases as lc
import localmap_update_cases as uc

pytestmark = pytest.mark.gpu
CHUNK = 1024     # orbu::kChunk: positions per block of the ordered compaction


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.8, True, device=0)


def load(matcher, s, max_local_points=None, pool=None):
    """the scene in a pool (zero records carrying the bad bit) and a store beside it"""
    from orbslamm_amd import KeyFrameStore, MapPool
    from orbslamm_amd.map_pool import POINT_DTYPE
    if pool is None:
        pool = MapPool(matcher, s.pool_cap)
        pts = np.zeros(s.pool_cap, POINT_DTYPE)
        pts["flags"] = s.pt_bad
        pool.set(np.arange(s.pool_cap), pts)
    store = KeyFrameStore(pool, s.kfcap, s.stride, s.maxc, max_local_points or s.kfcap * s.stride)
    store.set(*s.records())
    return pool, store


def assert_equals_ref(got, ref, tag):
    assert np.array_equal(got.votes, ref["votes"]), (tag, "votes", np.flatnonzero(got.votes != ref["votes"])[:8])
    assert (got.status == uc_status(ref)), (tag, "status")
    if ref["no_votes"]:
        return
    assert got.kf_max == ref["kf_max"], (tag, "kf_max", got.kf_max, ref["kf_max"])
    assert np.array_equal(got.kf, ref["kf"]), (tag, "kf", got.kf, ref["kf"])
    assert_points(got, ref, tag)


def assert_points(got, ref, tag):
    assert got.nL == len(ref["L"]) and np.array_equal(got.L, ref["L"]), (tag, "L", got.nL, len(ref["L"]))
    assert np.array_equal(got.seen, ref["seen"]), (tag, "seen")
    assert got.nS == len(ref["S"]) and np.array_equal(got.S, ref["S"]), (tag, "S")
    # got.S is L[seen == 0] made on the host, so the line above follows from the two before it; the list the resident search reads
    # is the one k_points_write compacts on the device through its own prefix: copied down and held to the restatement as well
    assert np.array_equal(got.resident, ref["S"]), (tag, "the device-resident S")


def uc_status(ref):
    return 1 if ref["no_votes"] else 0


def check(matcher, s, tag):
    pool, store = load(matcher, s)
    ref = uc.ref_update(s)
    got = store.update(s.frame_ids, s.max_keyframes)
    assert_equals_ref(got, ref, tag)
    again = store.update(s.frame_ids, s.max_keyframes)        # the same call twice: the same answer under the next tag
    assert_equals_ref(again, ref, (tag, "again"))
    store.close()
    pool.close()
    return ref


@pytest.mark.parametrize("family", sorted(uc.FAMILIES))
def test_update_equals_the_restatement(matcher, family):
    for seed in (1, 2):
        ref = check(matcher, uc.family_scene(family, seed), (family, seed))
    if family == "no_votes":
        assert ref["no_votes"]
    if family == "all_voted_bad":
        assert ref["kf_max"] == -1 and len(ref["kf"]) == 0


@pytest.mark.parametrize("nkf", [0, 1, 63, 64, 65, 300])
def test_keyframe_counts(matcher, nkf):
    rng = np.random.default_rng(nkf)
    s = uc.base_scene(rng, nkf=nkf, kfcap=max(nkf, 1), npts=max(20 * nkf, 200), nframe=200, p_unset=0.0, spread=8.0)
    ref = check(matcher, s, nkf)
    assert ref["no_votes"] == (nkf == 0)
    if nkf >= 63:
        assert len(ref["kf"]) > 10 and len(ref["L"]) > CHUNK // 2


@pytest.mark.parametrize("stride,nkf", [(64, 40), (65, 40), (2048, 12)])
def test_strides_and_row_lengths(matcher, stride, nkf):
    """rows of 0 .. stride entries (a fifth of the rows draw their length), one empty row and one full row among the voted"""
    rng = np.random.default_rng(stride)
    s = uc.base_scene(rng, nkf=nkf, stride=stride, npts=stride * 12, nframe=300, p_unset=0.0, p_kf_bad=0.0, spread=4.0)
    g = s.group()
    s.entries[g[0], :] = np.arange(stride, dtype=np.int32)            # n == stride
    s.entries[g[1], :] = -1                                           # n == 0 (it leaves the group)
    s.entries[g[2], stride - 1] = s.frame_ids[s.frame_ids >= 0][0]    # the last slot of a row
    ref = check(matcher, s, stride)
    assert len(ref["kf"]) >= 3 and len(ref["L"]) > stride


@pytest.mark.parametrize("group", [79, 80, 81, 90])
def test_voted_groups_around_the_limit(matcher, group):
    s = uc._group_of(120, group, np.random.default_rng(group), max_keyframes=80)
    ref = check(matcher, s, group)
    b = ref["branches"]
    if group <= 80:      # size() > 80 is false at the first step: the expansion runs until it is true
        assert b["steps_run"] >= 1 and b["size_break"] == 1 and len(ref["kf"]) > 80
    else:                # no expansion at all
        assert b["steps_run"] == 0 and np.array_equal(ref["kf"], s.group())


def test_no_votes_then_local_points_over_the_old_list(matcher):
    s = uc.family_scene("no_votes", 4)
    pool, store = load(matcher, s)
    got = store.update(s.frame_ids)
    assert got.status == 1 and got.nkf == 0 and got.nL == 0 and np.array_equal(got.votes, np.zeros(s.kfcap, np.int32))
    old = np.concatenate([s.set_slots()[::-2], s.set_slots()[:2]]).astype(np.int32)      # unordered, with repeats
    pts = store.local_points(old, s.frame_ids)
    assert pts.status == 0 and pts.kf_max == -1 and np.array_equal(pts.kf, old) and pts.votes is None
    ref = uc.ref_points(s, old)
    assert_points(pts, ref, "old list")
    assert ref["seen"].any() and len(ref["S"]) > 50
    empty = store.local_points(np.zeros(0, np.int32), s.frame_ids)
    assert empty.nkf == 0 and empty.nL == 0 and empty.nS == 0
    store.close()
    pool.close()


@pytest.mark.parametrize("stride,nkfs", [(64, (15, 16, 17, 32, 33)), (65, (15, 16, 31))])
def test_walks_that_end_around_a_chunk_boundary(matcher, stride, nkfs):
    """rows are walked at a pitch of 4-entry multiples, so a walk of 16 rows of 64 ends at position 1023, the chunk's last, and the
    17th row starts the next chunk at 1024; rows of 65 (pitch 68) put row boundaries inside a chunk.  Every row is full and the
    boundary entries are first sightings, so an offset that is off by one across chunks moves an element"""
    rng = np.random.default_rng(stride)
    s = uc.Scene(40, stride, 0, 40 * stride + 8)
    s.kf_flags[:] = uc.KF_SET
    s.entries[:, :] = rng.permutation(40 * stride).reshape(40, stride).astype(np.int32)
    s.pt_bad[rng.permutation(40 * stride)[:100]] = 1
    s.frame_ids = rng.integers(0, 40 * stride, 300).astype(np.int32)
    pool, store = load(matcher, s)
    pitch = (stride + 3) & ~3
    for nkf in nkfs:
        lst = rng.permutation(40)[:nkf].astype(np.int32)
        got = store.local_points(lst, s.frame_ids)
        ref = uc.ref_points(s, lst)
        assert_points(got, ref, (stride, nkf, nkf * pitch))
        assert len(ref["L"]) > nkf * stride * 0.9
    assert 16 * 64 == CHUNK
    store.close()
    pool.close()


@pytest.fixture(scope="module")
def wide(matcher):
    """1 100 keyframes of stride 1 024 (a row is exactly one compaction chunk) over 300 000 points, so that most points are met in
    several rows and a first sighting depends on rows many chunks away: (scene, pool, store, the restatement over all rows)"""
    rng = np.random.default_rng(1100)
    nkf, stride, npts = 1100, 1024, 300000
    s = uc.Scene(nkf, stride, 0, npts)
    s.kf_flags[:] = uc.KF_SET
    e = rng.integers(0, npts, (nkf, stride)).astype(np.int32)
    e[rng.random((nkf, stride)) < 0.05] = -1
    nv = (rng.random((nkf, stride)) < 0.05) & (e >= 0)
    e[nv] |= uc.NO_VOTE
    s.entries[:, :] = e
    s.pt_bad[:] = rng.random(npts) < 0.03
    s.frame_ids = np.where(rng.random(2000) < 0.2, -1, rng.integers(0, npts, 2000)).astype(np.int32)
    pool, store = load(matcher, s, max_local_points=npts)
    yield s, pool, store
    store.close()
    pool.close()


@pytest.mark.parametrize("nkf", [255, 256, 257, 512, 513, 1024, 1025, 1100])
def test_walks_of_many_chunks(wide, nkf):
    """the carries of the ordered compaction: k_points_scan takes 256 chunks an iteration and carries its running totals into the
    next (walks of 255, 256 and 257 chunks, 512 and 513 for the third iteration); the mark, count and write kernels run one block a
    chunk up to 1 024 blocks and stride beyond (1 024, 1 025 and 1 100 chunks: the second pass of their loops reuses the LDS
    counters and wave totals of the first).  Rows in a shuffled order with repeats among them"""
    s, pool, store = wide
    rng = np.random.default_rng(nkf)
    lst = rng.permutation(s.kfcap)[:nkf].astype(np.int32)
    lst[rng.integers(0, nkf, 3)] = lst[0]            # a row walked again: nothing of it is a first sighting
    got = store.local_points(lst, s.frame_ids)
    ref = uc.ref_points(s, lst)
    assert_points(got, ref, nkf)
    assert len(ref["L"]) > 100 * nkf and ref["seen"].sum() > 50 and len(ref["S"]) < len(ref["L"])


def test_update_over_a_voted_group_of_many_chunks(wide):
    """orbu_update_local_map whose voted group is nearly the whole store (k_select's compaction loop runs five times, no expansion:
    the group is above max_keyframes), walked at more chunks than the walk has blocks; then a small update behind it, whose grid
    is sized from this one, and the large one again, whose grid is sized from the small one: the answer does not depend on the grid"""
    s, pool, store = wide
    big = uc.ref_update(s)
    assert len(big["kf"]) > 1024 and big["branches"]["steps_run"] == 0
    assert_equals_ref(store.update(s.frame_ids), big, "big")
    few = s.frame_ids[:3]
    small = uc.ref_update(s, frame_ids=few)
    assert 0 < len(small["kf"]) < 40
    assert_equals_ref(store.update(few), small, "small")
    assert_equals_ref(store.update(s.frame_ids), big, "big after small")


def test_capacity_edge(matcher):
    from orbslamm_amd import OrbError
    s = uc.family_scene("random", 5)
    ref = uc.ref_update(s)
    nL = len(ref["L"])
    assert nL > 100
    pool, store = load(matcher, s, max_local_points=nL)
    assert_equals_ref(store.update(s.frame_ids), ref, "exactly max_local_points")
    small = load(matcher, s, max_local_points=nL - 1, pool=pool)[1]
    with pytest.raises(OrbError) as e:
        small.update(s.frame_ids)
    assert e.value.code == -4 and str(nL) in str(e.value)
    store.close()
    small.close()
    pool.close()
    # nL == 0: no local keyframe at all, and local keyframes whose points are all bad
    allbad = uc.family_scene("all_voted_bad", 2)
    assert len(uc.ref_update(allbad)["L"]) == 0 and not uc.ref_update(allbad)["no_votes"]
    check(matcher, allbad, "nL == 0")
    z = uc.family_scene("random", 6)
    lst = z.set_slots()[:5]
    z.pt_bad[z.entries[lst][z.entries[lst] >= 0] & ~uc.NO_VOTE] = 1
    pool, store = load(matcher, z)
    got = store.local_points(lst, z.frame_ids)
    assert got.nL == 0 and got.nS == 0 and got.nkf == 5 and (z.entries[lst] >= 0).sum() > 100
    store.close()
    pool.close()


def test_generation_wrap(matcher):
    """the tag of the pool-sized scratch is forced to its last value: the next call clears once and starts over, exactly"""
    s = uc.family_scene("random", 7)
    pool, store = load(matcher, s)
    frames = [s.frame_ids, s.frame_ids[::2], np.roll(s.frame_ids, 7)[:50], s.frame_ids[::-1]]
    refs = [uc.ref_update(s, frame_ids=f) for f in frames]
    assert_equals_ref(store.update(frames[0]), refs[0], "before")
    store.debug_set_generation(0xfffffffe)
    for f, r, tag in zip(frames[1:] + frames[:2], refs[1:] + refs[:2], ("last tag", "wrap", "after", "after 2", "after 3")):
        assert_equals_ref(store.update(f), r, tag)
    from orbslamm_amd import OrbError
    with pytest.raises(OrbError):
        store.debug_set_generation(1)           # the tag only moves forward
    store.close()
    pool.close()


def test_set_update_set_entries_update(matcher):
    """AddMapPoint / EraseMapPointMatch / Replace through orbu_kf_set_entries, a keyframe and a point turning bad, a graph record
    replaced: each followed by an update held to the restatement over the changed arrays"""
    from orbslamm_amd import OrbError
    rng = np.random.default_rng(11)
    s = uc.family_scene("random", 8)
    pool, store = load(matcher, s)
    assert_equals_ref(store.update(s.frame_ids), uc.ref_update(s), "set")
    g = s.group()
    k = int(g[1])
    idx = rng.permutation(s.stride)[:20].astype(np.int32)
    vals = np.where(rng.random(20) < 0.3, -1, rng.integers(0, s.pool_cap, 20)).astype(np.int32)
    vals[3] |= uc.NO_VOTE if vals[3] >= 0 else 0
    # a repeated index takes the last value
    store.set_entries(k, np.concatenate([idx, idx[:5]]), np.concatenate([vals[::-1], vals[:5]]))
    store.set_entries(k, idx[5:], vals[5:])
    s.entries[k, idx] = vals
    ref = uc.ref_update(s)
    assert_equals_ref(store.update(s.frame_ids), ref, "set_entries")
    store.set_flags([g[0], g[0]], [0, uc.KF_BAD])
    s.kf_flags[g[0]] |= uc.KF_BAD
    assert_equals_ref(store.update(s.frame_ids), uc.ref_update(s), "set_flags")
    live = ref["L"][:30]
    fl = np.ones(len(live), np.uint8)
    pool.set_flags(live, fl)
    s.pt_bad[live] = 1
    assert_equals_ref(store.update(s.frame_ids), uc.ref_update(s), "pool.set_flags")
    k2 = int(g[2])
    free = s.free()
    s.neigh[k2, :] = -1
    s.neigh[k2, :2] = [g[3], free[0]]
    s.parent[k2] = -1
    s.set_children(k2, [free[1]])
    store.set_graph([k2], [s.neigh[k2]], [s.parent[k2]], [s.children[k2, :1]])
    assert_equals_ref(store.update(s.frame_ids), uc.ref_update(s), "set_graph")
    # a keyframe repeated within one orbu_kf_set takes the last record
    other = uc.family_scene("random", 9)
    slots, flags, ent, neigh, parent, children = s.records([k, k2])
    o = other.records([other.set_slots()[0]] * 2)
    store.set(np.concatenate([slots, slots]), np.concatenate([o[1], flags]), o[2] + ent, o[3] + neigh, np.concatenate([o[4], parent]), [c[:0] for c in o[5]] + children)
    assert_equals_ref(store.update(s.frame_ids), uc.ref_update(s), "repeated keyframe")
    # refusals: nothing is written
    for bad_call in (lambda: store.set_entries(k, [0], [s.pool_cap]), lambda: store.set_entries(s.kfcap, [0], [1]),
                     lambda: store.set_flags([s.kfcap], [0]), lambda: store.update([s.pool_cap]), lambda: store.update([-2]),
                     lambda: store.local_points([s.kfcap], s.frame_ids),
                     lambda: store.set([0], [0], [[1]], [[s.kfcap]], [-1], [[]]), lambda: store.set([0], [0], [[1]], [[]], [s.kfcap], [[]])):
        with pytest.raises(OrbError) as e:
            bad_call()
        assert e.value.code == -1
    for big in (lambda: store.set_entries(k, [s.stride], [1]), lambda: store.set([0], [0], [np.zeros(s.stride + 1, np.int32)], [[]], [-1], [[]]),
                lambda: store.set([0], [0], [[1]], [[]], [-1], [np.zeros(s.maxc + 1, np.int32)])):
        with pytest.raises(OrbError) as e:
            big()
        assert e.value.code == -5
    assert_equals_ref(store.update(s.frame_ids), uc.ref_update(s), "after the refusals")
    store.close()
    pool.close()


def small_pool(matcher, n=8):
    from orbslamm_amd import MapPool
    from orbslamm_amd.map_pool import POINT_DTYPE
    pool = MapPool(matcher, n)
    pool.set(np.arange(n), np.zeros(n, POINT_DTYPE))
    return pool


def last_of_each(keys):
    """the index of the last record of every key: the records that win a setter call"""
    keys = np.asarray(keys)
    return np.array([np.flatnonzero(keys == k)[-1] for k in np.unique(keys)])


def test_a_repeated_index_on_both_sides_of_a_staging_launch_of_pairs(matcher):
    """one orbu_kf_set_entries of 2^20 + 4 pairs (a setter launch stages 8 MB: 2^20 pairs) whose indices cycle over a stride of 8:
    indices 0 .. 3 repeat behind the launch's end.  A fresh store given the eight last pairs alone answers with the same bytes"""
    from orbslamm_amd import KeyFrameStore
    n = (1 << 20) + 4
    i = np.arange(n)
    idx = (i % 8).astype(np.int32)
    vals = ((i * 5 + i // 8) % 8).astype(np.int32)
    vals[i % 11 == 0] |= uc.NO_VOTE
    vals[i % 7 == 0] = -1
    win = last_of_each(idx)
    assert (win >= 1 << 20).sum() == 4 and (win < 1 << 20).sum() == 4
    assert (vals[win[win >= 1 << 20]] != vals[win[win >= 1 << 20] - 8]).any()        # were the first launch to land last, it would show
    pool = small_pool(matcher)
    got = []
    for whole in (True, False):
        store = KeyFrameStore(pool, 1, 8, 0, 16)
        store.set([0], [0], [np.full(8, 3, np.int32)], [[]], [-1], [[]])
        store.set_entries(0, idx if whole else idx[win], vals if whole else vals[win])
        r = store.local_points([0], [1, -1, 5])
        got.append((r.L.tobytes(), r.seen.tobytes(), r.nL, r.nS, r.resident.tobytes()))
        store.close()
    assert got[0] == got[1] and got[0][2] > 0
    pool.close()


def test_a_repeated_slot_on_both_sides_of_a_staging_launch_of_records(matcher):
    """one orbu_kf_set of 104 857 + 3 records (80 bytes each at stride 4 without children: 104 857 fill a launch's 8 MB) whose slots
    cycle over a store of 8.  A fresh store given the eight last records alone answers an update with the same bytes"""
    from orbslamm_amd import KeyFrameStore
    per = (8 << 20) // 80
    n = per + 3
    i = np.arange(n)
    slots = (i % 8).astype(np.int32)
    flags = np.where(i % 9 == 0, uc.KF_BAD, 0).astype(np.uint8)
    ent = np.where((i[:, None] + np.arange(4)) % 5 == 0, -1, (i[:, None] + 3 * np.arange(4)) % 8).astype(np.int32)
    neigh = ((i + 1) % 8).astype(np.int32).reshape(-1, 1)
    parent = np.full(n, -1, np.int32)
    win = last_of_each(slots)
    assert per == 104857 and (win >= per).any() and (win < per).any()
    pool = small_pool(matcher)
    got = []
    for w in (i, win):
        store = KeyFrameStore(pool, 8, 4, 0, 16)
        store.set(slots[w], flags[w], list(ent[w]), list(neigh[w]), parent[w], [()] * len(w))
        r = store.update([0, 1, -1, 2, 5, 7])
        got.append((r.status, r.kf.tobytes(), r.L.tobytes(), r.seen.tobytes(), r.votes.tobytes()))
        store.close()
    assert got[0] == got[1] and got[0][0] == 0 and len(got[0][1]) > 4
    pool.close()


def test_pool_ids_that_were_never_set_are_refused(matcher):
    from orbslamm_amd import KeyFrameStore, MapPool, OrbError
    from orbslamm_amd.map_pool import POINT_DTYPE
    pool = MapPool(matcher, 64)
    pool.set(np.arange(10), np.zeros(10, POINT_DTYPE))
    store = KeyFrameStore(pool, 4, 8, 0, 16)
    with pytest.raises(OrbError) as e:
        store.set([0], [0], [[3, 10]], [[]], [-1], [[]])
    assert e.value.code == -1
    with pytest.raises(OrbError):
        store.set_graph([1], [[]], [-1], [[]])                 # a graph record of a keyframe never set
    store.set([0], [0], [[3, 9 | uc.NO_VOTE]], [[]], [-1], [[]])
    with pytest.raises(OrbError):
        store.update([10])
    got = store.update([3, -1, 3])
    assert got.status == 0 and list(got.kf) == [0] and list(got.L) == [3, 9] and list(got.seen) == [1, 0] and got.votes[0] == 2 and got.kf_max == 0
    store.close()
    pool.close()


def test_two_stores_on_one_pool(matcher):
    a = uc.family_scene("random", 3)
    b = uc.family_scene("neighbour_bad", 3)
    b.pt_bad = a.pt_bad.copy()          # one pool: the points' bad bytes are shared
    assert a.pool_cap == b.pool_cap
    pool, sa = load(matcher, a)
    sb = load(matcher, b, pool=pool)[1]
    ra, rb = uc.ref_update(a), uc.ref_update(b)
    for _ in range(2):
        assert_equals_ref(sa.update(a.frame_ids), ra, "a")
        assert_equals_ref(sb.update(b.frame_ids), rb, "b")
    assert_equals_ref(sb.update(a.frame_ids), uc.ref_update(b, frame_ids=a.frame_ids), "b with a's frame")
    assert_equals_ref(sa.update(a.frame_ids), ra, "a again")
    sa.close()
    sb.close()
    pool.close()


def test_the_search_from_the_resident_list(gpu):
    """orbw_track_local_map_resident against orbw_track_local_map given the restatement's S: table, count and status bytes, read
    back with back = 0 .. 3; refused before the store's first update"""
    from test_gpu_localmap import Rig, local_map_of
    from orbslamm_amd import KeyFrameStore, MapPool, OrbError
    rig = Rig()
    view, pts = local_map_of(rig)
    n = len(pts)
    rng = np.random.default_rng(21)
    pts["flags"][rng.permutation(n)[:40]] |= lc.FLAG_BAD
    pool = MapPool(rig.m, n)
    pool.set(np.arange(n), pts)
    # twelve keyframes of 128 slots over the local map's points; the frame already holds a tenth of them
    s = uc.Scene(12, 128, 2, n)
    s.pt_bad[:] = pts["flags"] & 1
    s.kf_flags[:] = uc.KF_SET
    for k in range(12):
        s.entries[k, :100] = rng.permutation(n)[:100]
        s.neigh[k, :2] = [(k + 1) % 12, (k + 5) % 12]
    s.frame_ids = np.where(rng.random(200) < 0.3, -1, rng.integers(0, n, 200)).astype(np.int32)
    store = KeyFrameStore(pool, 12, 128, 2, n)
    store.set(*s.records())
    with pytest.raises(OrbError) as e:
        store.track_local_map(rig.fs, 2, view, 1.0, rig.sf, rig.breaks)
    assert e.value.code == -1
    wants = []
    frames = [s.frame_ids, s.frame_ids[:50], s.frame_ids[::-1][:120], s.frame_ids[5:]]
    ths = (1.0, 3.0, 5.0, 2.0)
    for f, th in zip(frames, ths):
        S = uc.ref_update(s, frame_ids=f)["S"]
        pool.track_local_map(rig.fs, 2, view, S, th, rig.sf, rig.breaks)
        a, nm = rig.fs.results()
        wants.append((a.copy(), int(nm[0]), pool.track_status(rig.fs).copy(), len(S)))
    assert wants[1][1] > 100 and len({w[3] for w in wants}) > 1
    for i, (f, th) in enumerate(zip(frames, ths)):
        got = store.update(f)
        assert got.nS == wants[i][3]
        store.track_local_map(rig.fs, 2, view, th, rig.sf, rig.breaks)
    for back in range(4):
        want, wn, wst, nS = wants[3 - back]
        a, nm = rig.fs.results(back)
        assert nm[0] == wn and np.array_equal(a, want), back
        st = pool.track_status(rig.fs, back)
        assert st.shape[0] == nS and st.tobytes() == wst.tobytes(), back
    assert (wants[0][2] == lc.ST_BAD).sum() == 0        # the list holds no bad point: UpdateLocalPoints dropped them
    store.close()
    pool.close()


def test_update_dropin_on_mock_tracking(gpu):
    """include/Tracking_hip.hpp (UpdateLocalMapT::SyncKeyFrame / Run) on mock keyframes, MapPoints and frames
    (tests/cpp/localmap_update_dropin_gpu.cpp) against the serial reference loop over the same mocks: both vectors, the stamps,
    mpReferenceKF, the nulled bad matches, the frame nobody votes for, a refusal"""
    dropin.run(dropin.build("localmap_update_dropin_gpu"), timeout=300, marker="localmap update dropin ok")


def test_resident_dropin_on_mock_tracking(gpu):
    """SearchLocalPointsT::RunResident (tests/cpp/localmap_resident_dropin_gpu.cpp) against the serial SearchLocalPoints"""
    dropin.run(dropin.build("localmap_resident_dropin_gpu"), timeout=300, marker="localmap resident dropin ok")
