"""KeyFrame::UpdateConnections and KeyFrameCulling's counts on the device (orbn_*): every output array of
orbn_update_connections / orbn_culling_counts against the restatement (tools/covis_ref.hpp), element for element, over every scene
family, the set-keyframe counts 1, 2, 63, 64, 65 and 300, the strides 64, 65 and 2 048, target counts around the kernels' chunk,
repeated targets, a target alone against the same target in a batch, ordered lists longer than the selection's LDS tile, a forced
generation wrap, the setters' effects between two calls, two stores on one pool, orbu_update_local_map around the calls, and both
drop-ins against the members written serially.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import numpy as np
import pytest

import covis_cases as cc
import dropin

pytestmark = pytest.mark.gpu
CHUNK = 31           # orbn::kChunk: targets per pass over the store
SORT_TILE = 256      # orbn::kSortTile: keys of the ordered list per LDS tile


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.8, True, device=0)


def load(matcher, s, pool=None, octaves=True):
    """the scene in a pool (zero records carrying the bad bit) and a store beside it"""
    from orbslamm_amd import KeyFrameStore, MapPool
    from orbslamm_amd.map_pool import POINT_DTYPE
    if pool is None:
        pool = MapPool(matcher, s.pool_cap)
        pts = np.zeros(s.pool_cap, POINT_DTYPE)
        pts["flags"] = s.pt_bad
        pool.set(np.arange(s.pool_cap), pts)
    store = KeyFrameStore(pool, s.kfcap, s.stride, 4, s.kfcap * s.stride)
    store.set(*s.records())
    if octaves:
        for k in s.set_slots():
            store.set_octaves(k, s.octaves[k])
    return pool, store


def assert_same(got, ref, names, tag):
    for n in names:
        a, b = getattr(got, n), ref[n]
        assert a.dtype == b.dtype and np.array_equal(a, b), (tag, n, a[:16], b[:16])


def check(store, s, targets, tag, th=cc.TH, th_obs=cc.TH_OBS, culling=True):
    """both entries over `targets` against the restatement of the scene as it is now, twice"""
    from orbslamm_amd.map_pool import Connections, Culling
    ref = cc.Ref(s)
    rc = ref.connections(targets, th)
    for turn in range(2):                                         # the same call twice: the same bytes under the next tags
        assert_same(store.update_connections(targets, th), rc, Connections.NAMES, (tag, "connections", turn))
    if culling:
        ru = ref.culling(targets, th_obs)
        for turn in range(2):
            assert_same(store.culling_counts(targets, th_obs), ru, Culling.NAMES, (tag, "culling", turn))
    return rc, ref


@pytest.mark.parametrize("family", sorted(cc.FAMILIES))
def test_both_entries_equal_the_restatement(matcher, family):
    for seed in (1, 2):
        s = cc.family_scene(family, seed)
        pool, store = load(matcher, s)
        rc, ref = check(store, s, s.set_slots(), (family, seed))
        store.close()
        pool.close()
    seen = ref.seen()
    for b in cc.FAMILIES[family]:
        assert seen[b] > 0, (family, b)


@pytest.mark.parametrize("nset", [1, 2, 63, 64, 65, 300])
def test_set_keyframe_counts(matcher, nset):
    s = cc.random_scene(np.random.default_rng(nset), nkf=nset, npts=max(15 * nset, 200), fill=0.9, p_unset=0.0, crafted=0)
    assert len(s.set_slots()) == nset
    pool, store = load(matcher, s)
    rc, _ = check(store, s, s.set_slots(), nset)
    if nset >= 63:
        assert rc["ord_start"][-1] > 2 * nset
    store.close()
    pool.close()


@pytest.mark.parametrize("stride,nkf", [(64, 40), (65, 40), (2048, 12)])
def test_strides_with_an_empty_and_a_full_row(matcher, stride, nkf):
    s = cc.random_scene(np.random.default_rng(stride), nkf=nkf, stride=stride, npts=stride * 6, spread=4.0, p_unset=0.0, crafted=0)
    n = (s.entries >= 0).sum(axis=1)
    assert (n == 0).any() and (n == stride).any()
    pool, store = load(matcher, s)
    check(store, s, s.set_slots(), stride)
    store.close()
    pool.close()


def test_target_counts_around_the_chunk_repeats_and_a_target_alone(matcher):
    """unset slots lie between the set ones; a target's rows are the same bytes alone, in any batch and at any position"""
    s = cc.random_scene(np.random.default_rng(5), nkf=80, npts=1200, p_unset=0.2, crafted=0)
    slots = s.set_slots()
    assert len(slots) >= CHUNK + 1 and len(slots) < 80
    pool, store = load(matcher, s)
    rng = np.random.default_rng(6)
    for K in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1):
        tg = rng.permutation(slots)[:K] if K <= len(slots) else rng.choice(slots, K)
        check(store, s, tg, ("K", K))
    rep = np.array([slots[3], slots[7], slots[3], slots[3]] + list(slots[:CHUNK]) + [slots[3]], np.int32)     # a target repeated, across chunks
    check(store, s, rep, "repeated")
    every = store.update_connections(slots)
    cull = store.culling_counts(slots)
    for t, k in enumerate(slots):
        alone, alone_c = store.update_connections([k]), store.culling_counts([k])
        for which in ("counter", "ordered"):
            a, b = getattr(alone, which)(0), getattr(every, which)(t)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, which)
        assert (alone.status[0], alone.kf_max[0], alone.n_max[0]) == (every.status[t], every.kf_max[t], every.n_max[t])
        assert (alone_c.n_mps[0], alone_c.n_redundant[0], alone_c.redundant[0]) == (cull.n_mps[t], cull.n_redundant[t], cull.redundant[t])
    store.close()
    pool.close()


def test_an_ordered_list_longer_than_the_lds_tile_with_equal_weights_across_its_edge(matcher):
    """299 keyframes hold the first 15 + j // 40 points of keyframe 0's 64: weights in runs of 40 equal ones, one of which lies
    across place SORT_TILE of the ordered list"""
    nkf = 300
    s = cc.Scene(nkf, 64, 200, np.random.default_rng(11))
    pts = s.fresh(64)
    for pt in pts:
        s.put(0, pt)
    for j in range(1, nkf):
        for pt in pts[:15 + j // 40]:
            s.put(j, pt)
    pool, store = load(matcher, s)
    rc, _ = check(store, s, np.array([0, 150, 299, 0], np.int32), "long")
    kf, w = cc.row(rc, 0, "ord")
    assert len(kf) == nkf - 1 > SORT_TILE > 64 and w[SORT_TILE - 1] == w[SORT_TILE] == w[SORT_TILE - 2]
    assert (np.diff(w) <= 0).all() and (np.diff(kf)[np.diff(w) == 0] < 0).all()
    store.close()
    pool.close()


def test_a_forced_generation_wrap(matcher):
    s = cc.family_scene("random", 3)
    pool, store = load(matcher, s)
    tg = s.set_slots()
    check(store, s, tg, "before the wrap")
    store.debug_set_generation(0xffffffff - 1)                   # the next chunk takes the last tag, the one behind it wraps
    check(store, s, tg, "across the wrap")
    store.debug_set_generation(0xffffffff)
    check(store, s, tg[:3], "at the wrap")
    store.close()
    pool.close()


def test_results_follow_the_setters(matcher):
    s = cc.family_scene("weights_14_and_15", 4)
    pool, store = load(matcher, s)
    a, tg = cc.T0, s.set_slots()
    check(store, s, tg, "as loaded")
    # one more shared point: 14 becomes 15 (orbu_kf_set_entries on both keyframes)
    (pt,) = s.fresh()
    for k in (a, a + 1):
        i = s.put(k, pt, 2)
        store.set_entries(k, [i], [pt])
        store.set_octaves(k, s.octaves[k])
    rc, _ = check(store, s, tg, "an entry added")
    t = int(np.flatnonzero(tg == a)[0])
    assert sorted(cc.row(rc, t, "ord")[1].tolist()) == [15, 15, 16]
    # a shared point goes bad (orbw_pool_set_flags)
    bad = int(s.entries[a][s.entries[a] >= 0][0]) & ~cc.NO_VOTE
    s.pt_bad[bad] = 1
    pool.set_flags([bad], [1])
    check(store, s, tg, "a point gone bad")
    # an entry becomes NO_VOTE, as SetBadFlag's EraseObservation leaves it
    i = int(np.flatnonzero(s.entries[a + 2] >= 0)[0])
    s.entries[a + 2, i] |= cc.NO_VOTE
    store.set_entries(a + 2, [i], [s.entries[a + 2, i]])
    check(store, s, tg, "an entry without its vote")
    # octaves change the culling alone
    s.octaves[a + 3, :] = 7
    store.set_octaves(a + 3, s.octaves[a + 3])
    check(store, s, tg, "octaves replaced")
    # orbu_kf_set rewrites a row: the octaves stay
    s.entries[a + 1, :] = -1
    s.entries[a + 1, :20] = s.entries[a][s.entries[a] >= 0][:20] & ~cc.NO_VOTE
    store.set(*s.records([a + 1]))
    check(store, s, tg, "a row rewritten")
    store.close()
    pool.close()


def test_two_stores_on_one_pool_and_the_local_map_around_the_calls(matcher):
    """orbu_update_local_map gives the bytes it gave without the new calls, before and after them"""
    import localmap_update_cases as uc
    s1, s2 = cc.family_scene("random", 5), cc.family_scene("two_at_the_maximum", 5)
    assert s1.pool_cap == s2.pool_cap
    s2.pt_bad[:] = s1.pt_bad
    pool, st1 = load(matcher, s1)
    _, st2 = load(matcher, s2, pool=pool)
    _, plain = load(matcher, s1, pool=pool, octaves=False)       # never sees an orbn call
    frame = np.random.default_rng(9).integers(0, 600, 150).astype(np.int32)

    def local_map(store):
        r = store.update(frame)
        return [np.array([r.status, r.kf_max, r.nkf, r.nL, r.nS], np.int32), r.votes.copy(), r.kf.copy(), r.L.copy(), r.seen.copy(), r.resident]

    want = local_map(plain)
    assert want[0][0] == 0 and want[0][3] > 50
    before = local_map(st1)
    check(st1, s1, s1.set_slots(), "store 1")
    check(st2, s2, s2.set_slots(), "store 2")
    check(st1, s1, s1.set_slots()[::-1], "store 1 again")
    after = local_map(st1)
    for x, y, z in zip(want, before, after):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    for st in (st1, st2, plain):
        st.close()
    pool.close()


def test_culling_is_refused_while_a_set_keyframe_lacks_octaves(matcher):
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError, lib, ptr
    from orbslamm_amd import map_pool as mp
    import ctypes as C
    s = cc.family_scene("ratio_edges", 2)
    pool, store = load(matcher, s, octaves=False)
    tg = s.set_slots()
    res = mp.OrbnCulling()
    res.K = 77
    one = np.array([tg[0]], np.int32)
    assert lib().orbn_culling_counts(store._h, ptr(one), 1, 3, C.byref(res)) == ORBX_E_INVALID and res.K == 77 and not res.n_mps
    for k in tg[:-1]:
        store.set_octaves(k, s.octaves[k])
    assert lib().orbn_culling_counts(store._h, ptr(one), 1, 3, C.byref(res)) == ORBX_E_INVALID and res.K == 77 and not res.n_mps
    assert b"no octaves" in lib().orbx_last_error()
    check(store, s, tg, "connections need none", culling=False)
    # the setter's own refusals
    with pytest.raises(OrbError) as e:
        store.set_octaves(tg[-1], np.zeros(s.stride + 1, np.uint8))
    assert e.value.code == ORBX_E_UNSUPPORTED
    free = np.flatnonzero((s.kf_flags & cc.KF_SET) == 0)
    for slot in ([int(free[0])] if len(free) else []) + [s.kfcap]:
        with pytest.raises(OrbError) as e:
            store.set_octaves(slot, s.octaves[0])
        assert e.value.code == ORBX_E_INVALID
    with pytest.raises(OrbError) as e:                           # more distinct values than the histograms have bins
        store.set_octaves(tg[-1], np.arange(40, 40 + mp.MAX_OCTAVE_VALUES, dtype=np.uint8))
    assert e.value.code == ORBX_E_UNSUPPORTED
    for bad in [[s.kfcap], [-1]] + ([[int(free[0])]] if len(free) else []):
        with pytest.raises(OrbError) as e:
            store.update_connections(bad)
        assert e.value.code == ORBX_E_INVALID
    store.set_octaves(tg[-1], s.octaves[tg[-1]])
    check(store, s, tg, "every keyframe has octaves")
    store.close()
    pool.close()


def test_the_dropins_equal_the_members_written_serially(matcher, gpu):
    """tests/cpp/covis_dropin_gpu.cpp: UpdateConnectionsT::RunAll over 30 keyframes and a KeyFrameCullingT::Run in which two keyframes
    are culled and the first cull changes the second one's verdict, against the two members over the same mocks"""
    dropin.run(dropin.build("covis_dropin_gpu", pthread=False), timeout=120, marker="covis drop-ins: ok")
