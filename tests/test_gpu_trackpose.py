"""orbq_track_pose on the device: every output byte against the restatement (tools/trackpose_ref.hpp) and against
orbo_pose_optimize_frames given the host-made edge list of the same merge, over the scene families, the feature counts 0, 1, 63,
64, 65, 129 and the set's cap, the prefix carries of the ordered compaction inside one step of the kernel's walk and, on frames of
2 000 features, from step to step, each of the three pool searches as the source, back of
0 .. 3, 1 / 2 / 9 jobs over two frame sets, the same call twice, each ORBX_E_CAPACITY case provoked by its cause, the refusals found
by the kernel, a pool update between two calls, and the drop-in on mocks.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import numpy as np
import pytest

import dropin
import localmap_cases as lc
import localmap_update_cases as uc
import trackpose_cases as tc
from trackpose_cases import CAP, Rig, call, job, new_pool

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def rig(gpu):
    return Rig()


def search(rig, pool, fs, slot, case, ids=None):
    """the case's query list through orbw_track_local_map, received: (table over the frame's features, back) or (None, -1)"""
    ids = case["ids"] if ids is None else ids
    if not len(ids):
        return None, -1
    pool.track_local_map(fs, slot, case["view"], ids, 1.0, rig.sf, rig.breaks)
    assign, nm = fs.results()
    return assign[0, :case["n"]].copy(), 0


def assert_job_equals_ref(got, j, ref, tag):
    rc, out, ids, flags = got
    rrc, rout, rids, routl, br = ref
    assert rc == 0 and rrc == 0, (tag, rc, rrc)
    assert out[j].tobytes() == rout[0].tobytes(), (tag, "OrbqResult", out[j], rout[0])
    assert ids[j].tobytes() == rids.tobytes(), (tag, "ids_out", np.flatnonzero(ids[j] != rids)[:8])
    assert flags[j].tobytes() == routl.tobytes(), (tag, "outlier_out", np.flatnonzero(flags[j] != routl)[:8])


def assert_equals_orbo(rig, frame, case, assign, got, j, tag):
    """orbo_pose_optimize_frames on the host-made edge list of the same merge: the same core, so the same bytes"""
    from orbslamm_amd import pose_optimization
    merged, feat = tc.model_merge(case, assign)
    r = pose_optimization(rig.m, case["Tcw"], case["K"], None, feat.astype(np.int32), case["pool"]["pos"][merged[feat]], rig.sig, frame=frame)
    o = got[1]["opt"][j]
    assert o["Tcw"].tobytes() == r["Tcw"].astype(np.float32).tobytes(), (tag, "pose")
    assert (o["n_initial"], o["n_good"], o["rounds"]) == (r["n_initial"], r["n_good"], r["rounds"]), tag
    for k in ("iterations", "trials", "lambda_", "chi2"):
        assert o[k].tobytes() == r[k].tobytes(), (tag, k)
    assert np.array_equal(got[3][j][feat] != 0, r["outlier"]) and not got[3][j][merged < 0].any(), (tag, "outlier")


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_families_equal_the_restatement_and_the_edge_list_path(rig, family):
    for case in tc.family_cases(family):
        tag = (family, case["seed"])
        pool = new_pool(rig, case["pool"])
        frame = rig.put(rig.cfs[0], 1, case["keys"], case["desc"], resident=True)
        assign, back = search(rig, pool, rig.cfs[0], 1, case)
        if case["assign"] is not None:    # the lattice and the random descriptors leave the search no choice
            assert np.array_equal(assign, case["assign"]), (tag, np.flatnonzero(assign != case["assign"])[:8])
        refs = [tc.ref_run(case, d, assign=assign) for d in (0, 1)]
        got = call(rig, pool, [job(rig.cfs[0], 1, case, back, 0), job(rig.cfs[0], 1, case, back, 1)])
        for d in (0, 1):
            assert_job_equals_ref(got, d, refs[d], tag + (d,))
        assert tc.BRANCH[family](refs[0][4], refs[1][4], refs[0][1][0], refs[1][1][0]), (tag, refs[0][4], refs[1][4])
        assert_equals_orbo(rig, frame, case, assign, got, 0, tag)
        rig.m.frame_destroy(frame)
        pool.close()


def test_feature_counts_in_one_call(rig):
    """n of 0, 1, 63, 64, 65, 129 and the set's cap over one frame of `cap` features, merged from a search and a base"""
    s = tc.make_scene(77, CAP)
    feat = s["rng"].permutation(CAP)
    case = tc.with_lists(s, "counts", base_feat=feat[:90], query_feat=feat[60:260])
    pool = new_pool(rig, case["pool"])
    rig.put(rig.cfs[0], 2, case["keys"], case["desc"])
    assign, back = search(rig, pool, rig.cfs[0], 2, case)
    assert (assign >= 0).sum() > 150
    counts = (0, 1, 63, 64, 65, 129, CAP)
    got = call(rig, pool, [job(rig.cfs[0], 2, case, back, k % 2, n=n) for k, n in enumerate(counts)])
    for k, n in enumerate(counts):
        assert_job_equals_ref(got, k, tc.ref_run(case, k % 2, assign=assign, n=n), ("n", n))
    assert got[1]["opt"]["n_initial"][-1] > 180
    pool.close()


def placements():
    """(name, features holding a point) over a frame of CAP = 5 x 64 features"""
    out = []
    for c in (63, 64, 65, 127, 128, 129):
        out.append(("first %d" % c, np.arange(c)))
        out.append(("last %d" % c, np.arange(CAP - c, CAP)))
        out.append(("from 30, %d" % c, np.arange(30, 30 + c)))
    out.append(("last chunk only", np.arange(CAP - 64, CAP)))
    out.append(("last chunk but its first", np.arange(CAP - 63, CAP)))
    out.append(("first chunk only", np.arange(64)))
    out.append(("every 64th", np.arange(0, CAP, 64)))
    out.append(("every 64th from 63", np.arange(63, CAP, 64)))
    out.append(("every 64th and the last chunk", np.concatenate([np.arange(0, CAP - 64, 64), np.arange(CAP - 64, CAP)])))
    return out


def test_prefix_carries_of_the_ordered_compaction(rig):
    s = tc.make_scene(78, CAP)
    base = tc.with_lists(s, "placement", base_of={})
    pool = new_pool(rig, base["pool"])
    rig.put(rig.cfs[0], 3, base["keys"], base["desc"])
    cases = []
    for name, feat in placements():
        c = dict(base)
        c["base_ids"] = np.full(CAP, -1, np.int32)
        c["base_ids"][feat] = base["own"][feat]
        cases.append((name, c, len(feat)))
    got = call(rig, pool, [job(rig.cfs[0], 3, c, -1, k % 2) for k, (name, c, ne) in enumerate(cases)])
    for k, (name, c, ne) in enumerate(cases):
        assert_job_equals_ref(got, k, tc.ref_run(c, k % 2, assign=None), name)
        assert got[1]["opt"]["n_initial"][k] == ne, name
    pool.close()


BIG = 2000                     # a frame of the size bench.py extracts: four steps of the kernel's 8 x 64-feature walk (STEP features a step)
STEP = 512


def big_placements(rng):
    """(name, features holding a point) over a frame of BIG features: what crosses, or avoids, the walk's steps"""
    out = [("only beyond the first step", np.arange(STEP, STEP + 150)),
           ("only below it", np.arange(STEP - 150, STEP)),
           ("only in the last, partial step", np.arange(3 * STEP, BIG)),
           ("the last feature alone with the first", np.array([0, BIG - 1])),
           ("one point a step, at its first feature", np.arange(0, BIG, STEP)),
           ("one point a step, at its last feature", np.array([STEP - 1, 2 * STEP - 1, 3 * STEP - 1, BIG - 1])),
           ("every 64th", np.arange(0, BIG, 64)), ("every 64th from 63", np.arange(63, BIG, 64)),
           ("every feature", np.arange(BIG)), ("a random half", np.sort(rng.permutation(BIG)[:BIG // 2]))]
    for c in (63, 64, 65, 127, 128, 129):
        out.append(("%d across 512" % c, np.arange(STEP - c // 2, STEP - c // 2 + c)))
        out.append(("%d across 1 024" % c, np.arange(2 * STEP - c // 3, 2 * STEP - c // 3 + c)))
        out.append(("%d in two runs two steps apart" % c, np.concatenate([np.arange(STEP - 20, STEP - 20 + c // 2), np.arange(3 * STEP - 10, 3 * STEP - 10 + c - c // 2)])))
    return out


def test_frames_of_2000_features_cross_the_steps_of_the_walk(rig):
    """the kernel walks the features 512 a step and carries the edge count, the epilogue's edge index and both counts from step to
    step: placements on either side of and across features 512, 1 024 and 1 536, both discard modes, and merges of a search of 1 000
    queries with a base, against the restatement and against orbo_pose_optimize_frames on the host-made edge list"""
    s = tc.make_scene(79, BIG)
    rng = s["rng"]
    feat = rng.permutation(BIG)
    case = tc.with_lists(s, "big", base_feat=feat[:500], query_feat=feat[300:1300])
    wrong = feat[:120]                                   # gross outliers on both sides of every step: another feature's point
    case["base_ids"][wrong] = case["own"][feat[1500:1620]]
    pool = new_pool(rig, case["pool"])
    fs = rig.new_set(BIG)
    frame = rig.put(fs, 0, case["keys"], case["desc"], resident=True)
    # the placements: base ids alone, every job twice (discard 0 and 1), in one call
    cases = []
    for name, f in big_placements(rng):
        c = dict(case, ids=np.zeros(0, np.int32), assign=None)
        c["base_ids"] = np.full(BIG, -1, np.int32)
        c["base_ids"][f] = case["own"][f]
        c["base_ids"][f[::7]] = case["own"][(f[::7] + BIG // 2) % BIG]      # every seventh of them wrong
        cases.append((name, c, len(f)))
    got = call(rig, pool, [job(fs, 0, c, -1, d) for name, c, ne in cases for d in (0, 1)])
    for k, (name, c, ne) in enumerate(cases):
        for d in (0, 1):
            assert_job_equals_ref(got, 2 * k + d, tc.ref_run(c, d, assign=None), (name, d))
        assert got[1]["opt"]["n_initial"][2 * k] == ne, name
        if ne >= 60:
            assert got[3][2 * k].any() and not np.array_equal(got[2][2 * k], got[2][2 * k + 1]), name      # outliers: the modes differ
        if k % 4 == 0:
            assert_equals_orbo(rig, frame, c, None, got, 2 * k, name)
    # the merge of a search with a base, at n of one step, one step and a feature, two steps and a feature, and the whole frame
    assign, back = search(rig, pool, fs, 0, case)
    assert (assign >= 0).sum() > 950 and (assign[3 * STEP:] >= 0).sum() > 100
    counts = (STEP, STEP + 1, 2 * STEP + 1, BIG)
    got = call(rig, pool, [job(fs, 0, case, back, d, n=n) for n in counts for d in (0, 1)])
    for k, n in enumerate(counts):
        for d in (0, 1):
            assert_job_equals_ref(got, 2 * k + d, tc.ref_run(case, d, assign=assign, n=n), ("merge", n, d))
    assert got[1]["opt"]["n_initial"][-1] > 1200 and 50 < got[3][-1].sum() < 400
    assert_equals_orbo(rig, frame, case, assign, got, len(counts) * 2 - 2, "merge")
    rig.m.frame_destroy(frame)
    fs.close()
    pool.close()


def real_local_map(rig, seed):
    """slot 2's own features and those of frame 0 as MapPoints under a slightly moved camera: (case-like dict, records)"""
    rng = np.random.default_rng(300 + seed)
    R, t = lc.rot_axis_angle([0.2, 1.0, 0.1], 0.01), np.array([0.02, -0.01, 0.03])
    view = lc.make_view(R, t)
    keys = np.concatenate([rig.host[2][0], rig.host[0][0]])
    desc = np.concatenate([rig.host[2][1], rig.host[0][1]])
    pts = lc.points_from_keys(rng, view, keys, lc.SF, desc, jitter=0.5)
    k2 = rig.host[2][0]
    return dict(n=len(k2), keys=k2, view=view, Tcw=tc.pc.tcw_of(lc.rot_axis_angle([1, 0, 0.3], 0.003) @ R, t + 0.005), K=lc.K_A.copy(), pool=pts), pts


def test_each_of_the_three_searches_as_the_source(rig):
    from orbslamm_amd import KeyFrameStore
    case, pts = real_local_map(rig, 1)
    n, P = case["n"], len(pts)
    assert 300 <= n <= 520
    rng = np.random.default_rng(5)
    pool = new_pool(rig, pts)
    base = np.where(rng.random(n) < 0.15, rng.integers(0, P, n), -1).astype(np.int32)
    case["base_ids"] = base
    # (1) orbw_track_local_map with host ids
    ids = rng.permutation(P)[:P * 3 // 4].astype(np.int32)
    case["ids"] = ids
    pool.track_local_map(rig.fs, 2, case["view"], ids, 3.0, rig.sf, rig.breaks, t_occ=(base >= 0).astype(np.uint8))
    assign = rig.fs.results()[0][0, :n].copy()
    assert (assign >= 0).sum() > 150
    got = call(rig, pool, [job(rig.fs, 2, case, 0, 0)])
    assert_job_equals_ref(got, 0, tc.ref_run(case, 0, assign=assign), "host ids")
    assert got[1]["n_matches"][0] > 100 and got[2][0].tobytes() != np.where(assign >= 0, ids[np.maximum(assign, 0)], -1).astype(np.int32).tobytes()
    # (2) orbw_track_local_map_resident after an orbu_update_local_map
    s = uc.Scene(12, 128, 2, P)
    s.pt_bad[:] = pts["flags"] & 1
    s.kf_flags[:] = uc.KF_SET
    for k in range(12):
        s.entries[k, :100] = rng.permutation(P)[:100]
        s.neigh[k, :2] = [(k + 1) % 12, (k + 5) % 12]
    store = KeyFrameStore(pool, 12, 128, 2, P)
    store.set(*s.records())
    lm = store.update(base)
    assert lm.nS > 300
    store.track_local_map(rig.fs, 2, case["view"], 3.0, rig.sf, rig.breaks, t_occ=(base >= 0).astype(np.uint8))
    assign = rig.fs.results()[0][0, :n].copy()
    case["ids"] = store.resident_list()
    assert (assign >= 0).sum() > 100
    got = call(rig, pool, [job(rig.fs, 2, case, 0, 0)])
    assert_job_equals_ref(got, 0, tc.ref_run(case, 0, assign=assign), "resident")
    store.close()
    # (3) orbw_track_frame_pose: LastFrame = slot 0 holding points that CurrentFrame = slot 1's pose sees near slot 0's features
    keys0, desc0 = rig.host[0]
    n0, n1 = len(keys0), len(rig.host[1][0])
    view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.004), [0.01, 0.0, -0.02])
    pts0 = lc.points_from_keys(rng, view, keys0, lc.SF, desc0, jitter=1.0)
    pool0 = new_pool(rig, pts0)
    last_ids = np.where(rng.random(n0) < 0.85, np.arange(n0), -1).astype(np.int32)
    pool0.track_frame_pose(rig.fs, 1, 0, view, last_ids, 15.0, rig.sf)
    assign = rig.fs.results()[0][0, :n1].copy()
    assert (assign >= 0).sum() > 100
    c3 = dict(n=n1, keys=rig.host[1][0], Tcw=tc.pc.tcw_of(view[0]["Rcw"].reshape(3, 3).astype(np.float64), view[0]["tcw"].astype(np.float64)), K=lc.K_A.copy(),
              pool=pts0, base_ids=None, ids=last_ids)
    got = call(rig, pool0, [job(rig.fs, 1, c3, 0, 1)])
    assert_job_equals_ref(got, 0, tc.ref_run(c3, 1, assign=assign), "frame pose")
    # the search came from pool0: refused with the other pool
    assert call(rig, pool, [job(rig.fs, 1, c3, 0, 1)])[0] == E_INVALID
    pool0.close()
    pool.close()


def test_back_0_to_3_after_four_searches(rig):
    case = tc.family_cases("search_overwrites_base")[0]
    pool = new_pool(rig, case["pool"])
    fs = rig.cfs[1]
    rig.put(fs, 0, case["keys"], case["desc"])
    lists = [case["ids"], case["ids"][::2], case["ids"][::-1][:25], case["ids"][5:]]
    for ids in lists:
        pool.track_local_map(fs, 0, case["view"], ids, 1.0, rig.sf, rig.breaks)
    tables = [fs.results(3 - k)[0][0, :case["n"]].copy() for k in range(4)]          # search k lies `3 - k` back
    assert len({t.tobytes() for t in tables}) == 4
    got = call(rig, pool, [job(fs, 0, case, 3 - k, k % 2) for k in range(4)])
    for k in range(4):
        assert_job_equals_ref(got, k, tc.ref_run(case, k % 2, assign=tables[k], ids=lists[k]), ("back", 3 - k))
    pool.close()


def test_jobs_over_two_frame_sets_and_the_same_call_twice(rig):
    cases = [tc.family_cases(f)[1] for f in ("search_only", "gross_outliers", "search_overwrites_base")]
    big = np.concatenate([c["pool"] for c in cases])
    off = np.cumsum([0] + [len(c["pool"]) for c in cases])
    pool = new_pool(rig, big)
    shifted, jobs = [], []
    for k, c in enumerate(cases):
        c = dict(c)
        c["pool"] = big
        c["ids"] = c["ids"] + off[k]
        c["base_ids"] = None if c["base_ids"] is None else np.where(c["base_ids"] >= 0, c["base_ids"] + off[k], -1).astype(np.int32)
        fs, slot = rig.cfs[k % 2], 1 + k // 2
        rig.put(fs, slot, c["keys"], c["desc"])
        assign, back = search(rig, pool, fs, slot, c)
        shifted.append((c, assign))
        jobs.append((fs, slot, c))
    # searches on one set: cases 0 and 2 share cfs[0] -- case 0's lies one back
    nine = [job(*jobs[k % 3], back=(1 if k % 3 == 0 else 0), discard=(k // 3) % 2) for k in range(9)]
    alone = [call(rig, pool, [j]) for j in nine]
    for k, a in enumerate(alone):
        c, assign = shifted[k % 3]
        assert_job_equals_ref(a, 0, tc.ref_run(c, (k // 3) % 2, assign=assign), ("alone", k))
    for count in (1, 2, 9):
        got = call(rig, pool, nine[:count])
        again = call(rig, pool, nine[:count])
        assert got[0] == 0 and got[1].tobytes() == again[1].tobytes()
        for k in range(count):
            assert got[1][k].tobytes() == alone[k][1][0].tobytes(), (count, k)
            assert got[2][k].tobytes() == alone[k][2][0].tobytes() == again[2][k].tobytes(), (count, k)
            assert got[3][k].tobytes() == alone[k][3][0].tobytes() == again[3][k].tobytes(), (count, k)
    pool.close()


def last_error():
    from orbslamm_amd import _lib
    return _lib.lib().orbx_last_error().decode()


def test_capacity_refusals_each_by_its_cause(rig):
    from orbslamm_amd import KeyFrameStore
    case = tc.family_cases("search_only")[0]
    pool = new_pool(rig, np.concatenate([case["pool"], np.zeros(1200, lc.POINT_DTYPE)]))
    fs = rig.new_set()
    rig.put(fs, 0, case["keys"], case["desc"])
    rig.put(fs, 1, case["keys"], case["desc"])
    j = job(fs, 0, case, 0, 0)
    # a larger search reallocates the staging of all four result sets
    assign, _ = search(rig, pool, fs, 0, case)
    assert call(rig, pool, [j])[0] == 0
    pool.track_local_map(fs, 1, case["view"], np.arange(len(case["pool"]), len(case["pool"]) + 1200, dtype=np.int32), 1.0, rig.sf, rig.breaks)
    fs.results()
    rc = call(rig, pool, [dict(j, back=1)], fill=7)
    assert rc[0] == E_CAPACITY and "staging" in last_error() and (rc[2][0] == 7).all() and (rc[3][0] == 7).all(), last_error()
    # a slot rebuild
    assign, _ = search(rig, pool, fs, 0, case)
    assert call(rig, pool, [j])[0] == 0
    rig.put(fs, 0, case["keys"], case["desc"])
    assert call(rig, pool, [j])[0] == E_CAPACITY and "rebuilt" in last_error(), last_error()
    # a store update behind a resident search
    P = len(case["pool"])
    s = uc.Scene(2, 128, 0, P + 1200)
    s.kf_flags[:] = uc.KF_SET
    s.entries[0, :len(case["ids"])] = case["ids"]
    store = KeyFrameStore(pool, 2, 128, 0, P)
    store.set(*s.records())
    frame_ids = np.full(case["n"], -1, np.int32)
    frame_ids[0] = case["ids"][0]
    assert store.update(frame_ids).nS == len(case["ids"]) - 1
    store.track_local_map(fs, 0, case["view"], 1.0, rig.sf, rig.breaks)
    assign = fs.results()[0][0, :case["n"]].copy()
    c2 = dict(case, ids=store.resident_list(), base_ids=frame_ids)
    assert_job_equals_ref(call(rig, pool, [job(fs, 0, c2, 0, 0)]), 0, tc.ref_run(c2, 0, assign=assign), "resident before the update")
    store.update(frame_ids)
    assert call(rig, pool, [job(fs, 0, c2, 0, 0)])[0] == E_CAPACITY and "update" in last_error(), last_error()
    # the store destroyed and another made in its place with as many updates behind it: wherever the new one lies, it is another store
    store.track_local_map(fs, 0, case["view"], 1.0, rig.sf, rig.breaks)
    fs.results()
    assert call(rig, pool, [job(fs, 0, c2, 0, 0)])[0] == 0
    store.close()
    store = KeyFrameStore(pool, 2, 128, 0, P)
    store.set(*s.records())
    store.update(frame_ids)
    store.update(frame_ids)
    assert call(rig, pool, [job(fs, 0, c2, 0, 0)])[0] == E_CAPACITY and "destroyed" in last_error(), last_error()
    store.close()
    fs.close()
    pool.close()


def test_refusals_found_by_the_kernel_and_by_the_handles(rig):
    case = tc.family_cases("search_overwrites_base")[0]
    pool = new_pool(rig, case["pool"])
    other = new_pool(rig, case["pool"][:4])
    fs = rig.cfs[1]
    rig.put(fs, 2, case["keys"], case["desc"])
    assign, back = search(rig, pool, fs, 2, case)
    j = job(fs, 2, case, 0, 0)
    assert call(rig, pool, [j])[0] == 0
    # an octave outside nlevels (the keys reach octave 3): found by the kernel, reported behind it, the outputs untouched
    assert case["keys"]["octave"].max() == 3
    rc = call(rig, pool, [j], sig=rig.sig[:3], fill=7)
    assert rc[0] == E_INVALID and "octave" in last_error()
    assert rc[1].tobytes() == bytes(rc[1].nbytes) and (rc[2][0] == 7).all() and (rc[3][0] == 7).all()
    # a point at a feature the resident frame does not hold: 100 features on the device, a base id at feature 110
    rig.put(fs, 3, case["keys"][:100], case["desc"][:100])
    base = np.full(case["n"], -1, np.int32)
    base[[3, 50, 99]] = case["own"][[3, 50, 99]]
    assert call(rig, pool, [job(fs, 3, case, -1, 0, base=base)])[0] == 0
    base[110] = case["own"][110]
    rc = call(rig, pool, [job(fs, 3, case, -1, 0, base=base)], fill=7)
    assert rc[0] == E_INVALID and (rc[2][0] == 7).all()
    # the host's checks
    assert call(rig, pool, [dict(j, n=CAP + 1, base_ids=None)])[0] == E_INVALID and "features for a frame" in last_error()                      # above the set's cap
    assert call(rig, pool, [dict(j, slot=4)])[0] == E_INVALID
    assert call(rig, pool, [dict(j, slot=3)])[0] == E_INVALID and "slot" in last_error()   # the search ran against slot 2
    assert call(rig, other, [j])[0] == E_INVALID and "another pool" in last_error()
    for bad in (len(case["pool"]), -2):
        b = case["base_ids"].copy()
        b[0] = bad
        assert call(rig, pool, [job(fs, 2, case, 0, 0, base=b)])[0] == E_INVALID and "outside the pool" in last_error()
    assert call(rig, other, [job(fs, 2, case, -1, 0, base=np.full(case["n"], 2, np.int32))])[0] == 0
    from orbslamm_amd import MapPool
    empty = MapPool(rig.m, 8)
    assert call(rig, empty, [job(fs, 2, case, -1, 0, base=np.full(case["n"], 2, np.int32))])[0] == E_INVALID and "never set" in last_error()
    empty.close()
    # a search that has not been received, and one that was not issued from a pool
    pool.track_local_map(fs, 2, case["view"], case["ids"], 1.0, rig.sf, rig.breaks)
    assert call(rig, pool, [j])[0] == E_INVALID and "received" in last_error()
    fs.results()
    assert call(rig, pool, [j])[0] == 0
    ref = lc.ref_local(case["view"], case["pool"], case["ids"], 1.0)
    fs.track_local_points(2, ref["uvr"], ref["lvl"], case["pool"]["desc"][case["ids"]], ref["valid"], ref["obs"])
    fs.results()
    assert call(rig, pool, [j])[0] == E_INVALID and "map-point pool" in last_error()
    assert call(rig, pool, [dict(j, back=1)])[0] == 0
    # the pool destroyed and another made with the same records: wherever the new one lies, the search was not issued from it
    pool.close()
    pool = new_pool(rig, case["pool"])
    assert call(rig, pool, [dict(j, back=1)])[0] == E_INVALID and "another pool" in last_error(), last_error()
    other.close()
    pool.close()


def test_a_pool_update_between_two_calls(rig):
    case = dict(tc.family_cases("search_only")[1])
    pool = new_pool(rig, case["pool"])
    fs = rig.cfs[0]
    rig.put(fs, 0, case["keys"], case["desc"])
    assign, back = search(rig, pool, fs, 0, case)
    first = call(rig, pool, [job(fs, 0, case, 0, 1)])
    assert_job_equals_ref(first, 0, tc.ref_run(case, 1, assign=assign), "before")
    inl = np.flatnonzero((first[2][0] >= 0))[:12]
    moved = first[2][0][inl]
    pts2 = case["pool"].copy()
    pts2["pos"][moved] += np.float32(0.5)
    pts2["flags"][moved[:4]] = 0
    pool.set(moved, pts2[moved])
    second = call(rig, pool, [job(fs, 0, case, 0, 1)])
    assert_job_equals_ref(second, 0, tc.ref_run(case, 1, assign=assign, pool=pts2), "after")
    assert second[3][0][inl].all() and not first[3][0][inl].any() and second[1].tobytes() != first[1].tobytes()
    pool.close()


def test_trackpose_dropin_on_mock_tracking(gpu):
    """include/Tracking_hip.hpp (TrackWithMotionModelT::Finish, TrackLocalMapT::Run) on mocks (tests/cpp/trackpose_dropin_gpu.cpp) against
    the reference loops written serially over the same mocks"""
    dropin.run(dropin.build("trackpose_dropin_gpu"), timeout=300, marker="trackpose dropin ok")
