"""orbq_track_motion_model on the device: every output byte against the restatement (tools/motionmodel_ref.hpp) over
the scene families, and against the existing path fed with the device's Tcw_pred (orbw_track_frame_pose, orbm_track_results, the
retry issued by the host, orbq_track_pose); the track ring left alone; batches over two frame sets, a TOO_FEW, a wide and a plain job
in one call, the same call twice; the arena overflow replayed on a 2 000-feature pair; the refusals that need handles and the one a
kernel finds; a pool update between two calls; the drop-in on mocks.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import numpy as np
import pytest

import dropin
import localmap_cases as lc
import motionmodel_cases as mc

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def rig(gpu):
    return mc.Rig()


def existing_path(rig, pool, fs, last_slot, cur_slot, case, Tcw_pred, th=mc.TH, min_matches=mc.MIN_MATCHES, check_ori=True, n=None):
    """the parent's way, from the predicted pose on: (assign, status (2, nq), n_search, wide, track_pose's raw tuple or None)"""
    from orbslamm_amd.track_pose import pack_jobs, track_pose_raw
    n = case["n"] if n is None else n
    nq = case["nq"]
    view = mc.view_of_pose(np.asarray(Tcw_pred, np.float32).reshape(4, 4), case["K"], case.get("bounds", lc.BOUNDS))
    occ = (np.arange(fs.cap) >= n).astype(np.uint8)
    status = np.full((2, nq), mc.ST_NOT_RUN, np.uint8)

    def search(k, thx):
        pool.track_frame_pose(fs, cur_slot, last_slot, view, case["last_ids"], thx, lc.SF, occ, th_dist=100, nnratio=0.9, check_ori=check_ori, mode=4)
        a, nm = fs.results()
        status[k] = pool.track_status(fs)
        return a[0, :n].copy(), int(nm[0])
    assign, nm = search(0, np.float32(th))
    n_search, wide = [nm, -1], 0
    if nm < min_matches:
        assign, nm = search(1, np.float32(2.0) * np.float32(th))
        n_search[1], wide = nm, 1
    track = None
    if nm >= min_matches:
        rec, keep = pack_jobs([dict(fs=fs, slot=cur_slot, back=0, base_ids=None, n=n, discard=1, Tcw=np.asarray(Tcw_pred).reshape(4, 4), K=case["K"])])
        track = track_pose_raw(rig.m._h, pool._h, rec, rig.sig)
        assert track[0] == 0
    return assign, status, n_search, wide, track


def assert_job_equals_existing_path(got, j, ex, case, tag):
    code, out, ids, flags, assign, status = got
    eassign, estatus, n_search, wide, track = ex
    assert (list(out["n_search"][j]), int(out["wide"][j])) == (n_search, wide), (tag, out["n_search"][j], n_search)
    assert assign[j].tobytes() == eassign.tobytes(), (tag, "assign", np.flatnonzero(assign[j] != eassign)[:8])
    assert status[j].tobytes() == estatus.tobytes(), (tag, "status")
    if track is None:
        assert out["status"][j] == mc.TOO_FEW
        assert np.array_equal(ids[j], np.where(eassign >= 0, case["last_ids"][np.maximum(eassign, 0)], -1)) and not flags[j].any()
    else:
        assert out["status"][j] == mc.TRACKED
        assert out["track"][j].tobytes() == track[1][0].tobytes(), (tag, "OrbqResult", out["track"][j], track[1][0])
        assert ids[j].tobytes() == track[2][0].tobytes() and flags[j].tobytes() == track[3][0].tobytes(), (tag, "ids / outlier")


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_families_equal_the_restatement_and_the_existing_path(rig, family):
    case = mc.family_case(family)
    fs = rig.cfs[0]
    pool = mc.new_pool(rig, case["pool"])
    rig.put_case(fs, 0, 1, case)
    oris = (True, False) if family == "rotation_pruned" else (True,)
    for ori in oris:
        ref = mc.ref_run(case, check_ori=ori)
        assert mc.BRANCH[family](ref[6], ref[1][0]) or not ori, (family, ref[6])
        got = mc.call(rig, pool, [mc.job(fs, 0, 1, case)], check_ori=ori)
        mc.assert_job_equals_ref(got, 0, ref, (family, ori))
        if family != "fewer_device_keys":   # (the ring's table behind the slot's device count is not the search's to write)
            ex = existing_path(rig, pool, fs, 0, 1, case, got[1]["Tcw_pred"][0], check_ori=ori)
            assert_job_equals_existing_path(got, 0, ex, case, (family, ori))
    pool.close()


def test_the_track_ring_is_left_alone(rig):
    """a search issued on the set's track ring before the call is still readable, with the same table and status bytes, behind it"""
    case = mc.family_case("first_enough")
    fs = rig.cfs[0]
    pool = mc.new_pool(rig, case["pool"])
    rig.put_case(fs, 0, 1, case)
    view = mc.view_of_pose(mc.model_pose_product(case["velocity"], case["last_Tcw"]), case["K"])
    pool.track_frame_pose(fs, 1, 0, view, case["last_ids"], 15.0, lc.SF)
    a, nm = fs.results()
    before = (a.copy(), nm.copy(), pool.track_status(fs).copy())
    assert before[1][0] >= 70
    got = mc.call(rig, pool, [mc.job(fs, 0, 1, case)] * 3)
    assert got[0] == 0
    a, nm = fs.results()
    assert np.array_equal(a, before[0]) and np.array_equal(nm, before[1]) and np.array_equal(pool.track_status(fs), before[2])
    assert np.array_equal(got[4][0], before[0][0, :case["n"]])
    pool.close()


def test_batches(rig):
    """jobs over two frame sets and the same slots twice; a TOO_FEW, a wide and a plain job in one call, each equal to itself alone and
    to the restatement; the same call twice"""
    fams = ("too_few", "wide_rescues", "first_enough", "outliers_discarded")
    cases = [mc.family_case(f) for f in fams]
    # one pool for all: case k's records lie at ids k * stride ..
    stride = max(len(c["pool"]) for c in cases)
    records = np.zeros(stride * len(cases), lc.POINT_DTYPE)
    shifted = []
    for k, c in enumerate(cases):
        records[k * stride:k * stride + len(c["pool"])] = c["pool"]
        shifted.append(dict(c, last_ids=np.where(c["last_ids"] >= 0, c["last_ids"] + k * stride, -1).astype(np.int32)))
    pool = mc.new_pool(rig, records)
    where = [(rig.cfs[0], 0, 1), (rig.cfs[1], 0, 1), (rig.cfs[0], 2, 3), (rig.cfs[1], 2, 3)]
    for (fs, ls, cs), c in zip(where, shifted):
        rig.put_case(fs, ls, cs, c)
    jobs = [mc.job(fs, ls, cs, c) for (fs, ls, cs), c in zip(where, shifted)]
    order = [0, 1, 2, 3, 2, 0]
    got = mc.call(rig, pool, [jobs[k] for k in order])
    assert got[0] == 0
    assert list(got[1]["status"]) == [mc.TOO_FEW, mc.TRACKED, mc.TRACKED, mc.TRACKED, mc.TRACKED, mc.TOO_FEW] and list(got[1]["wide"]) == [1, 1, 0, 0, 0, 1]
    assert mc.same_call(got, mc.call(rig, pool, [jobs[k] for k in order])), "the same call twice: the same bytes"
    for j, k in enumerate(order):
        alone = mc.call(rig, pool, [jobs[k]])
        assert alone[0] == 0 and got[1][j].tobytes() == alone[1][0].tobytes(), (j, "record")
        assert all(got[i][j].tobytes() == alone[i][0].tobytes() for i in (2, 3, 4, 5)), (j, "arrays")
        ref = mc.ref_run(cases[k])
        # (the restatement ran on the case's own pool: its ids are the batch's less the shift)
        unshift = [a for a in got]
        unshift[2] = [np.where(x >= 0, x - k * stride, -1).astype(np.int32) if i == j else x for i, x in enumerate(got[2])]
        mc.assert_job_equals_ref(tuple(unshift), j, ref, (fams[k], j))
    pool.close()


def test_the_arena_overflow_is_replayed_whole(rig):
    """one 2 000-feature pair at 1241 x 376: 1 000 points where they are seen, 500 more that only the wide search finds, min_matches one
    above the first count (taken from the restatement), a job's share of the arena set to 64 entries.  The first run overflows in
    search 1, the second in search 2, the third returns: last_runs is 3 and every byte is the unconstrained run's"""
    from orbslamm_amd import make_grid
    from orbslamm_amd.track_pose import debug_motion_arena
    case = mc.big_case()
    first = int(mc.ref_run(case)[1]["n_search"][0][0])
    assert first >= 900
    ref = mc.ref_run(case, min_matches=first + 1)
    assert ref[1]["wide"][0] == 1 and ref[1]["status"][0] == mc.TRACKED and ref[1]["n_search"][0][1] >= first + 300
    fs = rig.m.frame_set(2, mc.BIG_N, mc.BIG_K, mc.rc.D0, make_grid(0.0, 0.0, float(mc.BIG_W), float(mc.BIG_H)), list(case["bounds"]), lc.SF)
    pool = mc.new_pool(rig, case["pool"])
    rig.put_case(fs, 0, 1, case)
    debug_motion_arena(rig.m, 0)
    free = mc.call(rig, pool, [mc.job(fs, 0, 1, case)], min_matches=first + 1)
    assert free[0] == 0 and debug_motion_arena(rig.m) == 1
    mc.assert_job_equals_ref(free, 0, ref, "unconstrained")
    debug_motion_arena(rig.m, 64)
    tight = mc.call(rig, pool, [mc.job(fs, 0, 1, case)], min_matches=first + 1)
    assert tight[0] == 0 and debug_motion_arena(rig.m) == 3
    assert mc.same_call(tight, free)
    assert debug_motion_arena(rig.m, 0) == 3
    again = mc.call(rig, pool, [mc.job(fs, 0, 1, case)], min_matches=first + 1)
    assert debug_motion_arena(rig.m) == 1 and mc.same_call(again, free)
    ex = existing_path(rig, pool, fs, 0, 1, case, free[1]["Tcw_pred"][0], min_matches=first + 1)
    assert_job_equals_existing_path(free, 0, ex, case, "big")
    # 2 098 jobs on this set: fewer than ORBO_MAX_FRAMES, 8 392 features, caps that add up past ORBO_MAX_CALL_EDGES
    many = mc.call(rig, pool, [mc.job(fs, 0, 1, case, n=4)] * 2098, fill=9, want_tables=False)
    assert many[0] == E_UNSUPPORTED and many[1].tobytes() == bytes(many[1].nbytes) and all((a == 9).all() for k in (2, 3) for a in many[k])
    pool.close()
    fs.close()


def test_refusals_that_need_handles_and_the_one_the_kernel_finds(rig):
    from orbslamm_amd import MapPool, ORBmatcher
    case = mc.family_case("first_enough")
    fs = rig.cfs[0]
    pool = mc.new_pool(rig, case["pool"])
    rig.put_case(fs, 0, 1, case)
    good = mc.job(fs, 0, 1, case)

    def refused(code, what, jobs, **kw):
        got = mc.call(rig, kw.pop("pool", pool), jobs, fill=9, **kw)
        assert got[0] == code, (what, got[0])
        assert got[1].tobytes() == bytes(got[1].nbytes) and all((a == 9).all() for k in (2, 3, 4, 5) for a in got[k] if a.size), what
    assert mc.call(rig, pool, [good])[0] == 0
    refused(E_INVALID, "cur_slot outside the set", [dict(good, cur_slot=4)])
    refused(E_INVALID, "last_slot outside the set", [dict(good, last_slot=4)])
    refused(E_INVALID, "n above the cap", [dict(good, n=mc.CAP + 1)])
    refused(E_INVALID, "nq above the cap", [dict(good, last_ids=np.full(mc.CAP + 1, -1, np.int32))])
    ids = case["last_ids"].copy()
    ids[np.flatnonzero(ids >= 0)[0]] = len(case["pool"])
    refused(E_INVALID, "an id outside the pool", [dict(good, last_ids=ids)])
    ids[ids == len(case["pool"])] = -2
    refused(E_INVALID, "an id below -1", [dict(good, last_ids=ids)])
    sparse = MapPool(rig.m, len(case["pool"]))
    sparse.set(np.arange(8), case["pool"][:8])
    refused(E_INVALID, "an id never set", [good], pool=sparse)
    sparse.close()
    other = ORBmatcher(0.9, True, device=0)
    refused(E_INVALID, "a frame set of another handle", [good], m=other)
    other.close()
    # found by the kernel: the call says two levels, and last-frame features of octave 1 hold the points of current features of octave
    # 2, which lie inside their level window: the match becomes an edge whose octave has no sigma
    true = case["groups"]["true"]
    up = true[case["keys"]["octave"][case["src"][true]] == 2][:5]
    assert len(up) == 5
    two = dict(case, lkeys=case["lkeys"].copy())
    two["lkeys"]["octave"][up] = 1
    rig.put_case(fs, 2, 3, two)
    assert mc.ref_run(two, sig=rig.sig[:2], nlevels=2)[0] == -1, "the restatement refuses it"
    refused(E_INVALID, "an edge's octave outside [0, nlevels)", [mc.job(fs, 2, 3, two)], sig=rig.sig[:2], nlevels=2)
    got = mc.call(rig, pool, [mc.job(fs, 2, 3, two)])
    mc.assert_job_equals_ref(got, 0, mc.ref_run(two), "eight levels: the same frames are tracked")
    assert mc.call(rig, pool, [good])[0] == 0, "the handle is good for the next call"
    pool.close()


def test_a_pool_update_between_two_calls(rig):
    """orbw_pool_set between two calls: the second call sees the new records, the first call's returned bytes stay"""
    case = mc.family_case("first_enough")
    fs = rig.cfs[0]
    pool = mc.new_pool(rig, case["pool"])
    rig.put_case(fs, 0, 1, case)
    first = mc.call(rig, pool, [mc.job(fs, 0, 1, case)])
    kept = [first[1].copy()] + [[a.copy() for a in first[k]] for k in (2, 3, 4, 5)]
    moved = case["pool"].copy()
    ids = case["last_ids"][case["groups"]["true"][:30]]
    for pid in ids:
        mc.rc.move_in_image(moved, pid, case["view"], 6.0, 0.0)
    moved["flags"][ids[:10]] = 0
    pool.set(ids, moved[ids])
    second = mc.call(rig, pool, [mc.job(fs, 0, 1, case)])
    mc.assert_job_equals_ref(second, 0, mc.ref_run(case, pool=moved), "after the update")
    assert second[1]["track"]["n_matches_map"][0] < first[1]["track"]["n_matches_map"][0]
    assert first[1].tobytes() == kept[0].tobytes() and all(a.tobytes() == b.tobytes() for k, i in enumerate((2, 3, 4, 5)) for a, b in zip(first[i], kept[k + 1]))
    mc.assert_job_equals_ref(first, 0, mc.ref_run(case), "the first call's bytes")
    pool.close()


def test_motionmodel_dropin_on_mock_tracking(gpu):
    """include/Tracking_hip.hpp (TrackWithMotionModelT::Run) on mocks (tests/cpp/motionmodel_dropin_gpu.cpp) against Tracking.cc:917-978
    written serially over the same mocks (tests/cpp/ref_motionmodel_loops.hpp): a tracked, a retried and a `return false` frame, and
    only-tracking"""
    dropin.run(dropin.build("motionmodel_dropin_gpu"), timeout=120, marker="motionmodel dropin ok")
