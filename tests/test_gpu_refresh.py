"""MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth on the device (orbr_*): every field of every
record of orbr_refresh_points against the restatement (tools/refresh_ref.hpp), each call made twice, over every scene family and
both halves; batches of 1, 63, 64, 65 and all points, shuffled, and every point alone; what a commit writes and what it leaves;
new positions; the setters' effects between two calls; descriptors from a frame set; a forced generation wrap; the refusals; the
drop-in against the two members written serially.
Floats are compared as bits; two NaNs are equal whatever their sign and payload, which IEEE 754 leaves to the implementation (a
point exactly at a camera centre: 0 * inf).
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import numpy as np
import pytest

import dropin
import refresh_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.8, True, device=0)


def load(matcher, r, descriptors=True, centres=True, octaves=True):
    """the scene in a pool and a store beside it"""
    from orbslamm_amd import KeyFrameStore, MapPool
    s = r.s
    pool = MapPool(matcher, s.pool_cap)
    pool.set(np.arange(s.pool_cap), r.pool_records())
    store = KeyFrameStore(pool, s.kfcap, s.stride, 4, s.kfcap * s.stride)
    store.set(*s.records())
    slots = s.set_slots()
    for k in slots:
        if octaves:
            store.set_octaves(k, s.octaves[k])
        if descriptors:
            store.set_descriptors(k, r.desc[k])
    if centres:
        store.set_centres(slots, r.centres[slots])
    return pool, store


def check(store, r, ids, tag, what=rc.BOTH, new_pos=None, commit=False):
    """the call over `ids` against the restatement of the scene as it is now, twice; returns the records"""
    ids = np.asarray(ids, np.int32)
    want = rc.Ref(r).refresh(ids, r.ref_kf[ids], what, new_pos)
    for turn in range(2):
        got = store.refresh_points(ids, r.ref_kf[ids], rc.SF, what, new_pos, commit)
        if not rc.same_records(got, want):
            i = next(k for k in range(len(ids)) if not rc.same_records(got[k:k + 1], want[k:k + 1]))
            bad = [n for n in rc.POINT_DTYPE.names if got[n][i].tobytes() != want[n][i].tobytes()]
            raise AssertionError((tag, turn, bad, int(ids[i]), got[i], want[i]))
    return want


def all_ids(r):
    return np.arange(r.pool_cap, dtype=np.int32)


@pytest.mark.parametrize("family", sorted(rc.FAMILIES))
def test_every_family_and_half_equals_the_restatement(matcher, family):
    for seed in (1, 2):
        r = rc.family_scene(family, seed)
        pool, store = load(matcher, r)
        for what in (rc.BOTH, rc.DESCRIPTOR, rc.NORMAL_DEPTH):
            check(store, r, all_ids(r), (family, seed, what), what)
        store.close()
        pool.close()


def test_batches_shuffled_orders_and_every_point_alone(matcher):
    r = rc.family_scene("observers_65", 3)
    pool, store = load(matcher, r)
    rng = np.random.default_rng(4)
    ids = all_ids(r)
    every = check(store, r, ids, "all")
    for n in (1, 63, 64, 65):
        check(store, r, rng.permutation(ids)[:n], ("batch", n))
    shuffled = rng.permutation(ids)
    got = check(store, r, shuffled, "shuffled")
    assert rc.same_records(got, every[shuffled])
    for pt in ids:                                                # a point's bytes are the same alone and in the batch
        alone = store.refresh_points([pt], [r.ref_kf[pt]], rc.SF, rc.BOTH, None, False)
        assert rc.same_records(alone, every[pt:pt + 1]), pt
    store.close()
    pool.close()


def view_and_breaks():
    from orbslamm_amd import level_breaks
    from orbslamm_amd import map_pool as mp
    v = mp.view(np.eye(3), [0.1, -0.2, 3.0], [-0.1, 0.2, -3.0], [500.0, 500.0, 320.0, 240.0], (0.0, 640.0, 0.0, 480.0))
    return v, level_breaks(float(np.log(np.float32(1.2))), rc.NLEVELS)


@pytest.mark.parametrize("what", [rc.BOTH, rc.DESCRIPTOR, rc.NORMAL_DEPTH])
def test_what_a_commit_writes_and_what_it_leaves(matcher, what):
    from orbslamm_amd import MapPool
    r = rc.family_scene("bad_keyframe_among", 4)
    pool, store = load(matcher, r)
    ids = all_ids(r)
    before = pool.debug_get(ids)
    assert before.tobytes() == r.pool_records().tobytes()
    check(store, r, ids, "compute only", what, commit=False)
    assert pool.debug_get(ids).tobytes() == before.tobytes()      # commit = 0 leaves every record as it was
    listed = np.random.default_rng(5).permutation(ids)[:len(ids) // 2]
    want = rc.Ref(r).refresh(listed, r.ref_kf[listed], what)
    got = store.refresh_points(listed, r.ref_kf[listed], rc.SF, what, None, True)
    assert rc.same_records(got, want)
    r.apply(listed, want, False)
    after = pool.debug_get(ids)
    expect = r.pool_records()
    assert after.tobytes() == expect.tobytes()                    # the listed ids as `out`, every other id and every flags byte unchanged
    assert after["flags"].tobytes() == before["flags"].tobytes() and after.tobytes() != before.tobytes()
    check(store, r, ids, "after the commit", what)                # the committed records are what the next call reads
    other = MapPool(matcher, r.pool_cap)
    other.set(ids, expect)
    v, br = view_and_breaks()
    for a, b, name in zip(pool.view_project(v, ids, 3.0, rc.SF, br), other.view_project(v, ids, 3.0, rc.SF, br), ("uvr", "lvl", "viewcos", "status")):
        assert a.tobytes() == b.tobytes(), name
    other.close()
    store.close()
    pool.close()


def test_new_positions_move_bad_points_too_and_the_normals_follow(matcher):
    r = rc.family_scene("bad_point", 5)
    pool, store = load(matcher, r)
    ids = all_ids(r)
    rng = np.random.default_rng(6)
    moved = (r.pos + rng.uniform(-0.5, 0.5, r.pos.shape)).astype(np.float32)
    plain = check(store, r, ids, "unmoved", rc.NORMAL_DEPTH)
    want = check(store, r, ids, "moved, compute only", rc.NORMAL_DEPTH, moved)
    done = want["st_normal_depth"] == rc.ST_DONE
    assert done.sum() > 100 and (want["normal"][done] != plain["normal"][done]).any(axis=1).all()
    assert pool.debug_get(ids).tobytes() == r.pool_records().tobytes()
    got = store.refresh_points(ids, r.ref_kf, rc.SF, rc.NORMAL_DEPTH, moved, True)
    assert rc.same_records(got, want)
    r.apply(ids, want, True)
    after = pool.debug_get(ids)
    assert after.tobytes() == r.pool_records().tobytes()
    bad = np.flatnonzero(r.s.pt_bad)
    assert len(bad) and after["pos"][bad].tobytes() == moved[bad].tobytes()      # SetWorldPos has no gate
    check(store, r, ids, "both halves from the moved pool", rc.BOTH)
    store.close()
    pool.close()


def test_results_follow_the_setters(matcher):
    r = rc.family_scene("observers_4", 6)
    pool, store = load(matcher, r)
    s, a, ids, pt = r.s, rc.T0, all_ids(r), r.named["p"]
    check(store, r, ids, "as loaded")
    (i,) = [i for k, i in r.observers(pt) if k == a + 1]          # orbu_kf_set_entries: an observation loses its vote, another appears
    s.entries[a + 1, i] |= rc.NO_VOTE
    store.set_entries(a + 1, [i], [s.entries[a + 1, i]])
    s.put(a + 4, pt, 2)
    store.set(*s.records([a + 4]))
    store.set_octaves(a + 4, s.octaves[a + 4])
    store.set_descriptors(a + 4, r.desc[a + 4])
    store.set_centres([a + 4], r.centres[[a + 4]])
    w = check(store, r, ids, "entries changed")
    assert w[pt]["n_obs"] == 4
    s.kf_flags[a + 2] |= rc.KF_BAD                                # orbu_kf_set_flags: a keyframe turns bad
    store.set_flags([a + 2], [rc.KF_BAD])
    w = check(store, r, ids, "a keyframe gone bad")
    assert (w[pt]["n_obs"], w[pt]["n_desc"]) == (4, 3)
    slots = s.set_slots()                                         # orbu_kf_set_centres: every keyframe moves; a repeated slot takes the last
    r.centres[slots] += np.float32(0.125)
    twice = np.concatenate([slots[:3], slots])
    store.set_centres(twice, np.concatenate([np.zeros((3, 3), np.float32), r.centres[slots]]))
    check(store, r, ids, "centres moved")
    r.desc[a] = np.random.default_rng(7).integers(0, 256, r.desc[a].shape, dtype=np.uint8)
    store.set_descriptors(a, r.desc[a][:s.stride - 5])            # orbu_kf_set_descriptors: the rows behind n become zero
    r.desc[a][s.stride - 5:] = 0
    check(store, r, ids, "descriptors replaced")
    s.pt_bad[pt] = 1                                              # orbw_pool_set_flags: the point turns bad
    pool.set_flags([pt], [r.pt_flags()[pt]])
    w = check(store, r, ids, "a point gone bad")
    assert w[pt]["st_descriptor"] == rc.ST_BAD
    store.close()
    pool.close()


def test_descriptors_from_a_frame_set_equal_the_host_setter(matcher):
    """three extracted frames resident in a frame set are three keyframes of two stores: one takes their descriptors device to
    device, the other from orbm_frameset_download's bytes"""
    import covis_cases as cc
    from orbslamm_amd import KeyFrameStore, MapPool, ORBextractor, make_grid, synth
    W, H = 640, 480
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=3, device=0)
    sf = np.array(gex.GetScaleFactors(), np.float32)
    fs = matcher.frame_set(4, gex.max_keypoints, [517.3, 516.5, 318.6, 255.3], [0, 0, 0, 0, 0], make_grid(0.0, 0.0, float(W), float(H)),
                           [0.0, float(W), 0.0, float(H)], sf)
    gex.extract_batch_device(*gex.upload_frames(synth.make_frames(W, H, 3, stream=17)))
    fs.build_from_extractor(0, gex)
    host = [fs.download(f) for f in range(3)]
    counts = [len(k) for k, _ in host]
    assert min(counts) > 100
    rng = np.random.default_rng(8)
    s = cc.Scene(3, fs.cap, 300, rng)
    r = rc.RScene(s, rng)
    r.desc[:] = 0
    for k in range(3):
        r.desc[k, :counts[k]] = host[k][1]
        s.octaves[k, :counts[k]] = host[k][0]["octave"]
        s.kf_flags[k] |= rc.KF_SET
    for pt in s.fresh(250):                                       # points in two or three of the frames, at features below the counts
        for k in rng.permutation(3)[:int(rng.integers(2, 4))]:
            free = np.flatnonzero(s.entries[k, :counts[k]] == -1)
            s.entries[k, free[rng.integers(len(free))]] = pt
    r.default_refs()
    pool = MapPool(matcher, s.pool_cap)
    pool.set(np.arange(s.pool_cap), r.pool_records())
    stores = [KeyFrameStore(pool, 3, fs.cap, 4, 3 * fs.cap) for _ in range(2)]
    for st in stores:
        st.set(*s.records())
        st.set_centres([0, 1, 2], r.centres)
        for k in range(3):
            st.set_octaves(k, s.octaves[k])
    for k in range(3):
        stores[0].set_descriptors_frame(k, fs, k)
        stores[1].set_descriptors(k, host[k][1])
    ids = all_ids(r)
    a = check(stores[0], r, ids, "from the frame set")
    b = check(stores[1], r, ids, "from the host")
    assert rc.same_records(a, b) and (a["st_descriptor"] == rc.ST_DONE).sum() >= 250
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError
    narrow = KeyFrameStore(pool, 3, 64, 4, 3 * 64)                # the slot's count is above this store's stride
    narrow.set([0], [0], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [-1], [np.zeros(0, np.int32)])
    with pytest.raises(OrbError) as e:
        narrow.set_descriptors_frame(0, fs, 0)
    assert e.value.code == ORBX_E_UNSUPPORTED
    for slot, fslot in ((1, 0), (0, 4), (0, -1)):                 # an unset keyframe, slots outside the frame set
        with pytest.raises(OrbError) as e:
            narrow.set_descriptors_frame(slot, fs, fslot)
        assert e.value.code == ORBX_E_INVALID
    for st in stores + [narrow]:
        st.close()
    pool.close()
    fs.close()


def test_a_forced_generation_wrap_with_the_other_entries_around_it(matcher):
    from orbslamm_amd.map_pool import Connections
    r = rc.family_scene("random", 7)
    pool, store = load(matcher, r)
    ids, tg = all_ids(r), r.s.set_slots()
    frame = np.random.default_rng(9).integers(0, 600, 150).astype(np.int32)

    def others():
        u = store.update(frame)
        c = store.update_connections(tg)
        return [np.array([u.status, u.kf_max, u.nkf, u.nL, u.nS], np.int32), u.kf.copy(), u.L.copy(), u.seen.copy()] + [getattr(c, n) for n in Connections.NAMES]

    want = others()
    check(store, r, ids, "before the wrap")
    store.debug_set_generation(0xffffffff - 1)                   # the next call takes the last tag, the one behind it wraps
    check(store, r, ids, "across the wrap")
    for x, y in zip(want, others()):
        assert np.array_equal(x, y)
    store.debug_set_generation(0xffffffff)
    check(store, r, ids[:5], "at the wrap")
    for x, y in zip(want, others()):
        assert np.array_equal(x, y)
    check(store, r, ids, "after the wrap")
    store.close()
    pool.close()


def test_the_observation_ceiling_and_its_refusal(matcher):
    from orbslamm_amd import map_pool as mp
    from orbslamm_amd._lib import ORBX_E_UNSUPPORTED, lib, ptr
    r = rc.long_scene(rc.MAX_OBS)
    pool, store = load(matcher, r)
    w = check(store, r, all_ids(r), "1 024 observers")
    assert w[r.named["p"]]["n_obs"] == rc.MAX_OBS and w[r.named["p"]]["st_descriptor"] == rc.ST_DONE
    store.close()
    pool.close()
    r = rc.long_scene(rc.MAX_OBS + 1)
    pool, store = load(matcher, r)
    ids = all_ids(r)
    before = pool.debug_get(ids)
    out = np.zeros(len(ids), mp.REFRESH_DTYPE)
    out.view(np.uint8)[:] = 0xAB
    ref = np.ascontiguousarray(r.ref_kf)
    code = lib().orbr_refresh_points(store._h, ptr(ids), ptr(ref), None, len(ids), rc.BOTH, ptr(rc.SF), rc.NLEVELS, 1, ptr(out))
    assert code == ORBX_E_UNSUPPORTED and b"observations" in lib().orbx_last_error()
    assert (out.view(np.uint8) == 0xAB).all() and pool.debug_get(ids).tobytes() == before.tobytes()      # refused: nothing written
    rest = ids[ids != r.named["p"]]
    check(store, r, rest, "without the point above the ceiling", commit=True)
    store.close()
    pool.close()


def test_the_refusals_with_a_store(matcher):
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError
    r = rc.family_scene("observers_3", 8)
    ids = all_ids(r)
    slots = r.s.set_slots()
    free = int(np.flatnonzero((r.s.kf_flags & rc.KF_SET) == 0)[0])
    for lack, what_fails in (("descriptors", (rc.DESCRIPTOR, rc.BOTH)), ("centres", (rc.NORMAL_DEPTH, rc.BOTH)), ("octaves", (rc.NORMAL_DEPTH, rc.BOTH))):
        pool, store = load(matcher, r, **{lack: False})
        last = int(slots[-1])
        for k in slots[:-1]:                                      # every keyframe but one has it: still refused
            if lack == "descriptors":
                store.set_descriptors(k, r.desc[k])
            elif lack == "octaves":
                store.set_octaves(k, r.s.octaves[k])
        if lack == "centres":
            store.set_centres(slots[:-1], r.centres[slots[:-1]])
        before = pool.debug_get(ids)
        for what in (rc.DESCRIPTOR, rc.NORMAL_DEPTH, rc.BOTH):
            if what in what_fails:
                with pytest.raises(OrbError) as e:
                    store.refresh_points(ids, r.ref_kf, rc.SF, what)
                assert e.value.code == ORBX_E_INVALID and ("slot %d has no" % last) in str(e.value)
            else:
                check(store, r, ids, (lack, what), what)
        assert pool.debug_get(ids).tobytes() == before.tobytes()
        store.close()
        pool.close()
    pool, store = load(matcher, r)
    bad_calls = [dict(ids=[0, 1, 0], ref=[-1, -1, -1]), dict(ids=[r.pool_cap], ref=[-1]), dict(ids=[-1], ref=[-1]), dict(ids=[0], ref=[free]),
                 dict(ids=[0], ref=[r.kfcap]), dict(ids=[0], ref=[-2])]
    for kw in bad_calls:
        with pytest.raises(OrbError) as e:
            store.refresh_points(kw["ids"], kw["ref"], rc.SF)
        assert e.value.code == ORBX_E_INVALID, kw
    with pytest.raises(OrbError) as e:
        store.refresh_points(np.zeros(r.pool_cap + 1, np.int32), np.full(r.pool_cap + 1, -1, np.int32), rc.SF)
    assert e.value.code == ORBX_E_UNSUPPORTED
    for call, code in ((lambda: store.set_descriptors(slots[0], np.zeros((r.stride + 1, 32), np.uint8)), ORBX_E_UNSUPPORTED),
                       (lambda: store.set_descriptors(free, r.desc[0]), ORBX_E_INVALID), (lambda: store.set_descriptors(r.kfcap, r.desc[0]), ORBX_E_INVALID),
                       (lambda: store.set_centres([slots[0], free], np.zeros((2, 3))), ORBX_E_INVALID),
                       (lambda: store.set_centres([r.kfcap], np.zeros((1, 3))), ORBX_E_INVALID), (lambda: pool.debug_get([r.pool_cap]), ORBX_E_INVALID)):
        with pytest.raises(OrbError) as e:
            call()
        assert e.value.code == code
    assert len(store.refresh_points([], [], rc.SF)) == 0
    check(store, r, ids, "after the refusals")
    store.close()
    pool.close()


def test_the_dropin_equals_the_members_written_serially(matcher, gpu):
    """tests/cpp/refresh_dropin_gpu.cpp: RefreshMapPointsT::Run over the mocks against ComputeDistinctiveDescriptors and
    UpdateNormalAndDepth written serially on the same mocks, their maps ordered by mnId"""
    dropin.run(dropin.build("refresh_dropin_gpu", pthread=False), timeout=120, marker="refresh drop-in: ok")
