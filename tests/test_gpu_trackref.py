"""orbq_track_reference on the device: the match table and its count against the oracle's SearchByBoW with the
validity array, every other output byte against the restatement (tools/trackref_ref.hpp), the solve against
orbo_pose_optimize_frames on the host-made edge list -- over the scene families at 300 features (the register path of the set
search) and one frame of 2 000 features on the 6-node vocabulary (its memory path; four steps of the feature walk); check_ori and
nnratio; solve and min_matches; 1, 2 and 9 jobs over two frame sets with keyframes and frames shared between jobs; the same call
twice; the BoW ring left alone; a pool update between two calls; the refusals that need handles; and the drop-in on mocks.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import numpy as np
import pytest

import dropin
import localmap_cases as lc
import trackpose_cases as tc
import trackref_cases as rc

from trackref_cases import CAP, Rig, call, job, new_world

pytestmark = pytest.mark.gpu
E_INVALID = -1
@pytest.fixture(scope="module")
def rig(gpu, oracle):
    return Rig(oracle)


def assert_job_equals_ref(got, j, whole, tag):
    """whole: trackref_cases.ref_whole's tuple"""
    rcode, out, ids, flags, match = got
    wm, nb, (rrc, rout, rids, routl, br), valid = whole
    assert rcode == 0 and rrc == 0, (tag, rcode, rrc)
    assert out["n_bow"][j] == nb and np.array_equal(match[j], wm[:len(match[j])]), (tag, "table", out["n_bow"][j], nb, np.flatnonzero(match[j] != wm[:len(match[j])])[:8])
    assert out[j].tobytes() == rout[0].tobytes(), (tag, "OrbqRefResult", out[j], rout[0])
    assert ids[j].tobytes() == rids.tobytes(), (tag, "ids_out", np.flatnonzero(ids[j] != rids)[:8])
    assert flags[j].tobytes() == routl.tobytes(), (tag, "outlier_out", np.flatnonzero(flags[j] != routl)[:8])


def assert_equals_orbo(rig, frame, case, match, got, j, tag, pool=None, entries=None):
    """orbo_pose_optimize_frames on the host-made edge list of the same merge: the same core, so the same bytes"""
    from orbslamm_amd import pose_optimization
    recs = case["pool"] if pool is None else pool
    _, ids = rc.model_validity(case, recs, entries)
    merged = np.where(match >= 0, ids[np.maximum(match, 0)], -1)
    feat = np.flatnonzero(merged >= 0)
    r = pose_optimization(rig.m, case["Tcw"], case["K"], None, feat.astype(np.int32), recs["pos"][merged[feat]], rig.sig, frame=frame)
    o = got[1]["track"]["opt"][j]
    assert o["Tcw"].tobytes() == r["Tcw"].astype(np.float32).tobytes(), (tag, "pose")
    assert (o["n_initial"], o["n_good"], o["rounds"]) == (r["n_initial"], r["n_good"], r["rounds"]), tag
    for k in ("iterations", "trials", "lambda_", "chi2"):
        assert o[k].tobytes() == r[k].tobytes(), (tag, k)
    assert np.array_equal(got[3][j][feat] != 0, r["outlier"]) and not got[3][j][merged < 0].any(), (tag, "outlier")


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_families_equal_the_oracle_the_restatement_and_the_edge_list_path(rig, family):
    case = rc.family_case(family)
    fs = rig.cfs[0]
    frame = rig.put_pair(fs, 0, 1, case, resident=True)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])
    whole = [rc.ref_whole(rig.oracle, case, solve, voc=rig.O) for solve in (1, 0)]
    got = call(rig, pool, store, [job(fs, 0, 1, 0, case, 1), job(fs, 0, 1, 0, case, 0)])
    for j in (0, 1):
        assert_job_equals_ref(got, j, whole[j], (family, "solve", 1 - j))
    assert rc.BRANCH[family](whole[0][2][4], whole[0][2][1][0]), (family, whole[0][2][4])
    if family != "empty_kf":
        assert got[1]["status"][0] == rc.TRACKED and got[1]["status"][1] == rc.SEARCH_ONLY
        assert_equals_orbo(rig, frame, case, whole[0][0], got, 0, family)
    if family == "all_valid":
        fs.search_by_bow([0], [1], nnratio=0.7, check_ori=True)
        table, nm = fs.bow_results()
        assert nm[0] == got[1]["n_bow"][0] and np.array_equal(table[0, :case["n"]], got[4][0]), "the all-valid table is orbm_bow_frames' own"
    rig.m.frame_destroy(frame)
    store.close(); pool.close()


def test_a_frame_of_2000_features_takes_the_memory_path(rig):
    """... and one call over that set of 2 048 features a slot and a set of 320: the per-job scratch offsets across sets of different
    caps, the search launched once per run of jobs on one set"""
    n = 2000
    case = rc.make_case("mixed", 3, n=n)
    small = dict(rc.family_case("null_entries"))
    fs, f0 = rig.new_set(2048), rig.cfs[0]
    rig.put_pair(fs, 2, 0, case)
    rig.put_pair(f0, 0, 1, small)
    fvq = rig.O.transform(case["kdesc"], rc.LEVELSUP)[1]
    assert np.diff(fvq[1]).max() > 256, "a node of more than 256 features: bow_pair_body's memory path"
    records = np.concatenate([case["pool"], small["pool"]])
    small["entries"] = np.where(small["entries"] >= 0, small["entries"] + len(case["pool"]), -1).astype(np.int32)
    small["pool"] = case["pool"] = records
    pool, store = new_world(rig, records, [case["entries"], small["entries"]], n)
    whole, wsmall = rc.ref_whole(rig.oracle, case, voc=rig.O), rc.ref_whole(rig.oracle, small, voc=rig.O)
    assert whole[1] > 1000 and wsmall[1] > 150
    got = call(rig, pool, store, [job(fs, 2, 0, 0, case)])
    assert_job_equals_ref(got, 0, whole, "2000")
    got = call(rig, pool, store, [job(f0, 0, 1, 1, small), job(fs, 2, 0, 0, case), job(f0, 0, 1, 1, small, 0), job(fs, 2, 0, 0, case, 0)])
    assert_job_equals_ref(got, 0, wsmall, "320 | 2048 | 320 | 2048: 0")
    assert_job_equals_ref(got, 1, whole, "320 | 2048 | 320 | 2048: 1")
    assert_job_equals_ref(got, 2, rc.ref_whole(rig.oracle, small, 0, voc=rig.O), "320 | 2048 | 320 | 2048: 2")
    assert_job_equals_ref(got, 3, rc.ref_whole(rig.oracle, case, 0, voc=rig.O), "320 | 2048 | 320 | 2048: 3")
    store.close(); pool.close(); fs.close()


def test_n_below_the_slots_feature_count(rig):
    """the search runs over the whole slot; the count, the gate, the merge and the solve over the job's n features"""
    case = rc.make_case("mixed", 6)
    fs = rig.cfs[1]
    rig.put_pair(fs, 0, 2, case)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])
    valid, _ = rc.ref_validity(case)
    match, nb = rc.oracle_search(rig.oracle, case, valid, voc=rig.O)
    ns = (0, 1, 63, 64, 65, 200, case["n"])
    for mm in (15, int((match[:200] >= 0).sum()) + 1):     # the second gate lies between the count over 200 features and the whole frame's
        got = call(rig, pool, store, [job(fs, 0, 2, 0, case, n=n) for n in ns], min_matches=mm)
        assert got[0] == 0
        for j, n in enumerate(ns):
            r = rc.ref_run(case, match, 1, mm, n=n)
            cnt = int((match[:n] >= 0).sum())
            assert r[0] == 0 and got[1]["n_bow"][j] == cnt == r[1]["n_bow"][0], (n, got[1]["n_bow"][j], cnt)
            assert got[1]["status"][j] == (rc.TOO_FEW if cnt < mm else rc.TRACKED)
            assert got[1][j].tobytes() == r[1][0].tobytes() and got[2][j].tobytes() == r[2].tobytes() and got[3][j].tobytes() == r[3].tobytes(), (mm, n)
            assert np.array_equal(got[4][j], match[:n])
    assert nb >= mm > (match[:200] >= 0).sum()
    store.close(); pool.close()


def test_check_ori_nnratio_solve_and_min_matches(rig):
    case = rc.make_case("ratio_ori", 2)
    fs = rig.cfs[1]
    rig.put_pair(fs, 1, 3, case)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])
    tables = {}
    for ori in (False, True):
        for ratio in (0.7, 0.75):
            whole = rc.ref_whole(rig.oracle, case, nnratio=ratio, check_ori=ori, voc=rig.O)
            got = call(rig, pool, store, [job(fs, 1, 3, 0, case)], nnratio=ratio, check_ori=ori)
            assert_job_equals_ref(got, 0, whole, (ori, ratio))
            tables[ori, ratio] = whole[1]
    assert tables[False, 0.75] >= tables[False, 0.7] + 3 and tables[False, 0.7] >= tables[True, 0.7] + 5 and tables[True, 0.75] >= tables[True, 0.7] + 3, tables
    nb = tables[True, 0.7]
    for mm, status in ((0, rc.TRACKED), (15, rc.TRACKED), (nb, rc.TRACKED), (nb + 1, rc.TOO_FEW)):
        for solve in (1, 0):
            whole = rc.ref_whole(rig.oracle, case, solve, mm, voc=rig.O)
            got = call(rig, pool, store, [job(fs, 1, 3, 0, case, solve)], min_matches=mm)
            assert_job_equals_ref(got, 0, whole, (mm, solve))
            assert got[1]["status"][0] == (status if solve or status == rc.TOO_FEW else rc.SEARCH_ONLY)
            if got[1]["status"][0] != rc.TRACKED:
                assert got[1]["track"]["opt"]["rounds"][0] == 0 and not got[3][0].any() and got[1]["track"]["n_matches"][0] == nb
    # no table asked for: the same bytes otherwise
    full = call(rig, pool, store, [job(fs, 1, 3, 0, case)])
    for wm in (False, [False]):
        bare = call(rig, pool, store, [job(fs, 1, 3, 0, case)], want_match=wm)
        assert bare[0] == 0 and bare[4][0] is None and bare[1].tobytes() == full[1].tobytes() and bare[2][0].tobytes() == full[2][0].tobytes()
    store.close(); pool.close()


def pair_case(kfc, frc):
    """keyframe of one case against the frame of another"""
    c = dict(frc)
    c.update(kkeys=kfc["kkeys"], kdesc=kfc["kdesc"], entries=kfc["entries"], stride=kfc["stride"], nk=kfc["nk"])
    return c


def test_batches_over_two_frame_sets(rig):
    """1, 2 and 9 jobs; one keyframe against several frames, several keyframes against one frame; each job equal to itself alone; the
    same call twice; the set's BoW ring left as it was; a moved point between two calls"""
    A, B, Cc = (rc.make_case(f, 4 + i) for i, f in enumerate(("mixed", "no_vote", "gross_outliers")))
    sizes = [len(c["pool"]) for c in (A, B, Cc)]
    base = np.concatenate([[0], np.cumsum(sizes)])
    records = np.concatenate([A["pool"], B["pool"], Cc["pool"]])
    rows = [np.where(c["entries"] >= 0, c["entries"] + base[i], -1).astype(np.int32) for i, c in enumerate((A, B, Cc))]
    for c, row in zip((A, B, Cc), rows):
        c["entries"], c["pool"] = row, records
    f0, f1 = rig.cfs
    rig.put_pair(f0, 0, 1, A)
    rig.put_pair(f0, 2, 3, B)
    rig.put_pair(f1, 0, 1, Cc)
    # a frame of A's in the second set too: one keyframe (C) against two frames
    rig.put(f1, 2, A["keys"], A["desc"])
    f1.compute_bow(rig.G, 2, 1, rc.LEVELSUP)
    pool, store = new_world(rig, records, rows, rc.N)
    f0.search_by_bow([0, 2], [1, 3], nnratio=0.7, check_ori=True)
    ring = [(t.copy(), n.copy(), t.ctypes.data) for t, n in [f0.bow_results()]][0]
    AB, BA, CA = pair_case(A, B), pair_case(B, A), pair_case(Cc, A)
    spec = [(f0, 0, 1, 0, A, 1), (f0, 0, 3, 0, AB, 1), (f1, 0, 1, 2, Cc, 1), (f0, 2, 3, 1, B, 1), (f0, 2, 1, 1, BA, 0), (f1, 0, 2, 2, CA, 1),
            (f0, 0, 1, 0, A, 0), (f0, 2, 3, 1, B, 0), (f1, 0, 1, 2, Cc, 0)]
    jobs = [job(*s[:5], solve=s[5]) for s in spec]
    wholes = [rc.ref_whole(rig.oracle, s[4], s[5], voc=rig.O) for s in spec]
    assert wholes[0][1] > 150 and wholes[1][1] < 15 and wholes[1][2][1]["status"][0] == rc.TOO_FEW
    for k in (1, 2, 9):
        got = call(rig, pool, store, jobs[:k])
        for j in range(k):
            assert_job_equals_ref(got, j, wholes[j], ("batch", k, j))
    again = call(rig, pool, store, jobs)
    assert again[1].tobytes() == got[1].tobytes() and all(a.tobytes() == b.tobytes() for x, y in zip(again[2:], got[2:]) for a, b in zip(x, y))
    for j in range(9):
        alone = call(rig, pool, store, [jobs[j]])
        assert alone[1][0].tobytes() == got[1][j].tobytes() and all(alone[k][0].tobytes() == got[k][j].tobytes() for k in (2, 3, 4)), ("alone", j)
    t, n = f0.bow_results()
    assert t.ctypes.data == ring[2] and np.array_equal(t, ring[0]) and np.array_equal(n, ring[1]), "orbm_bow_results returns what it returned before"
    # orbw_pool_set of a moved point between two calls: the second result is the restatement's on the moved pool
    hit = np.flatnonzero(got[2][0] >= 0)
    moved = records.copy()
    pid = got[2][0][hit[:12]]
    moved["pos"][pid] += np.float32(0.7)
    pool.set(pid, moved[pid])
    A2 = dict(A, pool=moved)
    after = call(rig, pool, store, [jobs[0]])
    w2 = rc.ref_whole(rig.oracle, A2, voc=rig.O)
    assert_job_equals_ref(after, 0, w2, "moved")
    assert after[1][0].tobytes() != got[1][0].tobytes() and after[3][0][hit[:12]].sum() >= 8
    store.close(); pool.close()


def test_refusals_that_need_handles(rig):
    from orbslamm_amd import MapPool, ORBmatcher
    from orbslamm_amd.map_pool import KeyFrameStore
    case = rc.family_case("all_valid")
    fs = rig.cfs[0]
    rig.put_pair(fs, 0, 1, case)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])

    def refused(jobs, what, **kw):
        got = call(rig, *kw.pop("world", (pool, store)), jobs, fill=9, **kw)
        assert got[0] == E_INVALID, (what, got[0])
        assert got[1].tobytes() == bytes(got[1].nbytes) and all((a == 9).all() for k in (2, 3, 4) for a in got[k]), what
    good = job(fs, 0, 1, 0, case)
    assert call(rig, pool, store, [good])[0] == 0
    refused([job(fs, 0, 1, 0, case, n=CAP + 1)], "n above the set's cap")
    refused([job(fs, 4, 1, 0, case)], "keyframe slot outside the set")
    refused([job(fs, 0, 4, 0, case)], "slot outside the set")
    refused([job(fs, 0, 1, 4, case)], "kf outside the store")
    refused([job(fs, 0, 1, 1, case)], "kf not set")
    refused([good, job(fs, 0, 1, 1, case)], "a later job's kf not set")
    bare = rig.new_set()
    refused([job(bare, 0, 1, 0, case)], "orbm_frameset_compute_bow has not run")
    bare.close()
    # the sets' caps add up beyond ORBO_MAX_CALL_EDGES, whatever n is: the search's scratch grows with the cap
    wide = rig.new_set(2048)
    rig.put_pair(wide, 0, 1, case)
    got = call(rig, pool, store, [job(wide, 0, 1, 0, case, n=0)] * 2049, fill=9)
    assert got[0] == -5 and got[1].tobytes() == bytes(got[1].nbytes), got[0]
    wide.close()
    pool2 = MapPool(rig.m, 16)
    store2 = KeyFrameStore(pool2, 2, 8, 0, 16)
    refused([good], "a store of another pool", world=(pool, store2))
    m2 = ORBmatcher(0.7, True, device=0)
    refused([good], "a frame set of another handle", m=m2)
    m2.close()
    # found by the kernel, reported behind it: an edge's octave outside [0, nlevels)
    refused([good], "octave outside nlevels", sig=rig.sig[:1])
    assert call(rig, pool, store, [good])[0] == 0
    store2.close(); pool2.close(); store.close(); pool.close()


def test_trackref_dropin_on_mock_tracking(gpu):
    """include/Tracking_hip.hpp (TrackReferenceKeyFrameT::Run) on mocks (tests/cpp/trackref_dropin_gpu.cpp, mock_trackref.hpp) against
    Tracking::TrackReferenceKeyFrame written serially over the same mocks"""
    dropin.run(dropin.build("trackref_dropin_gpu"), timeout=120, marker="trackref dropin ok")
