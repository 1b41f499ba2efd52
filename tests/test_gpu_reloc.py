"""orbq_relocalize on the device: every output byte -- the result records, the ids, the outlier bytes and the status
bytes of both projections -- against the restatement (tools/reloc_ref.hpp), over the exit, gate and search families at 300 features
against 250 row entries, each call made twice; 1, 2 and 9 jobs over two frame sets with keyframes, frames and points shared between
jobs, each job equal to its one-job call; solve 1 against orbo_pose_optimize_frames on the host-made edge list; the wide search
against orbm_track_frame_projected, mode 5, and against the matcher drop-in's own member (its host gates and
orbm_search_by_projection_frame), with the track and BoW rings left alone; check_ori 0 and 1; a pool update between two calls; one frame of 2 000 features; the arena's overflow path from a debug starting size; the refusals that
need handles.  A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import numpy as np
import pytest

import localmap_cases as lc
import reloc_cases as rc
from reloc_cases import assert_job_equals_ref, call, job, kf_keys, new_world, same_call

pytestmark = pytest.mark.gpu
W, H = lc.W, lc.H
CAP = rc.CAP
E_INVALID, E_CAPACITY, E_UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def rig(gpu):
    return rc.Rig()


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_families_equal_the_restatement(rig, family):
    case = rc.family_case(family)
    fs = rig.cfs[0]
    rig.put_case(fs, 0, 1, case)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])
    ref = rc.ref_run(case)
    assert rc.BRANCH[family](ref[5], ref[1][0]), (family, ref[5])
    got = call(rig, pool, store, [job(fs, 0, 1, 0, case)], log_sf=case["log_sf"])
    assert_job_equals_ref(got, 0, ref, family)
    assert same_call(got, call(rig, pool, store, [job(fs, 0, 1, 0, case)], log_sf=case["log_sf"])), (family, "the same call twice")
    if family in rc.EXIT_OF:
        assert got[1]["exit"][0] == rc.EXIT_OF[family]
    if family == "contention":
        qa, qb = sorted(np.flatnonzero(np.isin(case["entries"], np.setdiff1d(np.arange(len(case["pool"])), case["own"]))))[:2]
        assert (got[2][0] == case["entries"][qa]).sum() == 1 and (got[2][0] == case["entries"][qb]).sum() == 1, "both contenders hold a feature"
    store.close(); pool.close()


def test_solve_1_equals_the_edge_list_path(rig):
    """orbo_pose_optimize_frames on the host-made edge list of the same ids: the same core, so the same bytes"""
    from orbslamm_amd import pose_optimization
    case = rc.family_case("second_high")
    fs = rig.cfs[1]
    frame = rig.put_case(fs, 0, 1, case, resident=True)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])
    got = call(rig, pool, store, [job(fs, 0, 1, 0, case)])
    feat = np.flatnonzero(case["ids"] >= 0)
    r = pose_optimization(rig.m, case["Tcw"], case["K"], None, feat.astype(np.int32), case["pool"]["pos"][case["ids"][feat]], rig.sig, frame=frame)
    o = got[1]["opt"][0][0]
    assert o["Tcw"].tobytes() == r["Tcw"].astype(np.float32).tobytes(), "pose"
    assert (o["n_initial"], o["n_good"], o["rounds"]) == (r["n_initial"], r["n_good"], r["rounds"])
    for k in ("iterations", "trials", "lambda_", "chi2"):
        assert o[k].tobytes() == r[k].tobytes(), k
    rig.m.frame_destroy(frame)
    store.close(); pool.close()


def test_check_ori_0_and_1(rig):
    case = rc.family_case("rotation_pruned")
    fs = rig.cfs[1]
    rig.put_case(fs, 2, 3, case)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])
    outs = {}
    for ori in (False, True):
        ref = rc.ref_run(case, check_ori=ori)
        got = call(rig, pool, store, [job(fs, 2, 3, 0, case)], check_ori=ori)
        assert_job_equals_ref(got, 0, ref, ("check_ori", ori))
        outs[ori] = (int(got[1]["n_additional"][0][0]), ref[5]["nRotPruned"])
    assert outs[False][1] == 0 and outs[True][1] >= 3 and outs[False][0] >= outs[True][0] + 3, outs
    # no status asked for: the same bytes otherwise
    full = call(rig, pool, store, [job(fs, 2, 3, 0, case)])
    for ws in (False, [False]):
        bare = call(rig, pool, store, [job(fs, 2, 3, 0, case)], want_status=ws)
        assert bare[0] == 0 and bare[4][0] is None and bare[1].tobytes() == full[1].tobytes() and bare[2][0].tobytes() == full[2][0].tobytes()
    store.close(); pool.close()


def shifted(case, base, records):
    """the case on the shared pool: its ids and entries moved by `base`"""
    c = dict(case)
    c["entries"] = np.where(case["entries"] >= 0, case["entries"] + base, -1).astype(np.int32)
    c["ids"] = np.where(case["ids"] >= 0, case["ids"] + base, -1).astype(np.int32)
    c["pool"] = records
    return c


def test_batches_over_two_frame_sets(rig):
    """1, 2 and 9 jobs; one keyframe against several frames' id lists, several jobs on one frame and one keyframe whose sFound differ;
    each job equal to the restatement and to itself alone; the same call twice; a moved point between two calls"""
    fams = ("third_succeeds", "second_low", "first", "wide_short")
    cases = [rc.make_case(f, 3 + i) for i, f in enumerate(fams)]
    base = np.concatenate([[0], np.cumsum([len(c["pool"]) for c in cases])])
    records = np.concatenate([c["pool"] for c in cases])
    A, B, Cc, Dd = (shifted(c, base[i], records) for i, c in enumerate(cases))
    f0, f1 = rig.cfs
    rig.put_case(f0, 0, 1, A)
    rig.put_case(f0, 2, 3, B)
    rig.put_case(f1, 0, 1, Cc)
    rig.put_case(f1, 2, 3, Dd)
    pool, store = new_world(rig, records, [c["entries"] for c in (A, B, Cc, Dd)], rc.NK)
    # A's frame and keyframe with fewer of PnP's ids: another sFound over the same points, and another exit
    A2 = dict(A, ids=np.where(np.arange(A["n"]) % 2 == 0, A["ids"], -1).astype(np.int32))
    A3 = dict(A, ids=np.full(A["n"], -1, np.int32))
    spec = [(f0, 0, 1, 0, A), (f0, 2, 3, 1, B), (f1, 0, 1, 2, Cc), (f0, 0, 1, 0, A2), (f1, 2, 3, 3, Dd), (f0, 0, 1, 0, A3), (f0, 2, 3, 1, B), (f0, 0, 1, 0, A),
            (f1, 0, 1, 2, Cc)]
    jobs = [job(*s) for s in spec]
    refs = [rc.ref_run(s[4]) for s in spec]
    exits = [int(r[1]["exit"][0]) for r in refs]
    assert exits[0] == rc.THIRD and exits[1] == rc.SECOND and exits[2] == rc.FIRST and exits[4] == rc.WIDE_SHORT and exits[5] == rc.REJECTED and refs[3][1].tobytes() != refs[0][1].tobytes(), exits
    for k in (1, 2, 9):
        got = call(rig, pool, store, jobs[:k])
        for j in range(k):
            assert_job_equals_ref(got, j, refs[j], ("batch", k, j))
    assert same_call(got, call(rig, pool, store, jobs)), "the same call twice"
    for j in range(9):
        alone = call(rig, pool, store, [jobs[j]])
        assert alone[1][0].tobytes() == got[1][j].tobytes() and all(alone[k][0].tobytes() == got[k][j].tobytes() for k in (2, 3, 4)), ("alone", j)
    # orbw_pool_set of moved points between two calls: the second result is the restatement's on the moved pool
    hit = np.flatnonzero(got[2][0] >= 0)
    moved = records.copy()
    pid = got[2][0][hit[:12]]
    moved["pos"][pid] += np.float32(0.7)
    pool.set(pid, moved[pid])
    after = call(rig, pool, store, [jobs[0]])
    assert_job_equals_ref(after, 0, rc.ref_run(dict(A, pool=moved)), "moved")
    assert after[1][0].tobytes() != got[1][0].tobytes()
    store.close(); pool.close()


def test_a_frame_of_2000_features_and_the_arena_overflow(rig):
    """one frame of 2 000 features against a row of 1 700, beside a 300-feature job in another set of 2 048 a slot; then the same call
    from an arena of 8 entries a job: the searches overflow, the host grows the arena and runs the whole call again, and the result is
    the roomy call's"""
    from orbslamm_amd.track_pose import debug_reloc_arena
    n, nk = 2000, 1700
    big = rc.make_case("third_succeeds", 5, n=n, nk=nk, counts=rc.EXIT_FAMILIES["third_succeeds"])
    small = rc.family_case("narrow_short")
    records = np.concatenate([big["pool"], small["pool"]])
    small = shifted(small, len(big["pool"]), records)
    big = dict(big, pool=records)
    row = np.full(nk, -1, np.int32)
    row[:len(small["entries"])] = small["entries"]
    small["entries"], small["stride"] = row, nk
    fs, f2 = rig.new_set(2048), rig.new_set(2048)
    rig.put_case(fs, 2, 0, big)
    rig.put_case(f2, 0, 1, small)
    pool, store = new_world(rig, records, [big["entries"], row], nk)
    rbig, rsmall = rc.ref_run(big), rc.ref_run(small)
    assert rbig[1]["exit"][0] == rc.THIRD and rbig[1]["n_additional"][0][1] >= 10 and rsmall[1]["exit"][0] == rc.NARROW_SHORT
    jobs = [job(f2, 0, 1, 1, small), job(fs, 2, 0, 0, big)]
    roomy = call(rig, pool, store, jobs)
    assert debug_reloc_arena(rig.m) == 1
    assert_job_equals_ref(roomy, 0, rsmall, "2048 | 2048: 0")
    assert_job_equals_ref(roomy, 1, rbig, "2048 | 2048: 1")
    debug_reloc_arena(rig.m, 8)
    tight = call(rig, pool, store, jobs)
    assert same_call(roomy, tight), "the overflow path returns the roomy call's bytes"
    # (the wide search's need is settled by the first re-run; the narrow one's needs a second only where it lists more than the wide one did)
    assert 2 <= debug_reloc_arena(rig.m, 0) <= 3, "the call ran again behind the overflow"
    assert same_call(roomy, call(rig, pool, store, jobs)) and debug_reloc_arena(rig.m) == 1
    store.close(); pool.close(); fs.close(); f2.close()


def test_refusals_that_need_handles(rig):
    from orbslamm_amd import MapPool, ORBmatcher
    from orbslamm_amd.map_pool import KeyFrameStore
    case = rc.family_case("second_high")
    fs = rig.cfs[0]
    rig.put_case(fs, 0, 1, case)
    pool, store = new_world(rig, case["pool"], [case["entries"]], case["stride"])

    def refused(jobs, what, code=E_INVALID, **kw):
        got = call(rig, *kw.pop("world", (pool, store)), jobs, fill=9, **kw)
        assert got[0] == code, (what, got[0])
        assert got[1].tobytes() == bytes(got[1].nbytes) and all((a == 9).all() for k in (2, 3, 4) for a in got[k]), what
    good = job(fs, 0, 1, 0, case)
    assert call(rig, pool, store, [good])[0] == 0
    refused([job(fs, 0, 1, 0, case, n=CAP + 1, ids=np.full(CAP + 1, -1, np.int32))], "n above the set's cap")
    refused([job(fs, 4, 1, 0, case)], "keyframe slot outside the set")
    refused([job(fs, 0, 4, 0, case)], "slot outside the set")
    refused([job(fs, 0, 1, 4, case)], "kf outside the store")
    refused([job(fs, 0, 1, 1, case)], "kf not set")
    refused([good, job(fs, 0, 1, 1, case)], "a later job's kf not set")
    ids = case["ids"].copy()
    ids[np.flatnonzero(ids >= 0)[0]] = len(case["pool"])
    refused([job(fs, 0, 1, 0, case, ids=ids)], "an id outside the pool")
    pool2 = MapPool(rig.m, 16)
    store2 = KeyFrameStore(pool2, 2, 8, 0, 16)
    refused([good], "a store of another pool", world=(pool, store2))
    wide = KeyFrameStore(pool, 2, CAP + 8, 0, 16)
    wide.set(np.arange(1), np.zeros(1, np.uint8), [case["entries"]], [[]], [-1], [[]])
    refused([good], "a stride above the frame set's cap", world=(pool, wide))
    m2 = ORBmatcher(0.9, True, device=0)
    refused([good], "a frame set of another handle", m=m2)
    m2.close()
    # found by the kernels, reported behind them: an edge's octave outside [0, nlevels); a feature with a point at or above the
    # slot's device count; a row entry with a point at or above the keyframe slot's device count
    refused([good], "octave outside nlevels", sig=rig.sig[:1], nlevels=1, brk=rc.breaks()[:2])
    rig.put(fs, 2, case["keys"][:200], case["desc"][:200])
    assert (case["ids"][200:] >= 0).any()
    refused([job(fs, 0, 2, 0, case)], "a point at a feature the resident frame does not hold")
    rig.put(fs, 3, kf_keys(case)[:100], np.zeros((100, 32), np.uint8))
    assert (case["entries"][100:] >= 0).any()
    refused([job(fs, 3, 1, 0, case)], "a row entry with a point beyond the keyframe slot's keys")
    assert call(rig, pool, store, [good])[0] == 0
    wide.close(); store2.close(); pool2.close(); store.close(); pool.close()


def host_member_equals_the_device(case, got, cur):
    """ORBmatcherT::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, 10, 100) of include/ORBmatcher_hip.hpp on mocks filled from the
    case (tests/cpp/reloc_hostproj_gpu.cpp): its host gates (:549-571, the tree's own PredictScale) in front of
    orbm_search_by_projection_frame, at the pose solve 1 left, with the frame's points behind the discard.  The row entries it pushes as
    queries are the device's IN_VIEW ones, its count is n_additional[0] and the frame's points behind it are ids_out"""
    import os
    import tempfile
    import dropin
    g, pool_rec, n, nk = rc.grid(), case["pool"], case["n"], case["stride"]
    found = np.zeros(len(pool_rec), np.uint8)
    found[case["ids"][case["ids"] >= 0]] = 1
    row = np.full(nk, -1, np.int32)
    row[:len(case["entries"])] = case["entries"]
    parts = [np.array([n, nk, len(pool_rec), lc.NLEVELS, 10, 100], np.int32),
             np.array(list(case["K"]) + list(lc.BOUNDS) + [g.invW, g.invH], np.float32), np.asarray(got[1]["opt"][0][0]["Tcw"], np.float32),
             np.array([case["log_sf"]], np.float32), np.asarray(lc.SF, np.float32), np.ascontiguousarray(case["keys"][:n]), np.ascontiguousarray(case["desc"][:n], np.uint8),
             cur.astype(np.int32), found, row, np.asarray(case["kang"], np.float32)[:nk], np.ascontiguousarray(pool_rec["pos"], np.float32),
             np.ascontiguousarray(pool_rec["min_distance"], np.float32), np.ascontiguousarray(pool_rec["max_distance"], np.float32),
             np.ascontiguousarray(pool_rec["flags"], np.uint8), np.ascontiguousarray(pool_rec["desc"], np.uint8)]
    d = tempfile.mkdtemp(prefix="reloc_hostproj_")
    with open(os.path.join(d, "in.bin"), "wb") as f:
        for a in parts:
            f.write(a.tobytes())
    dropin.run(dropin.build("reloc_hostproj_gpu"), os.path.join(d, "in.bin"), os.path.join(d, "out.bin"), timeout=120, marker="reloc hostproj ok")
    raw = open(os.path.join(d, "out.bin"), "rb").read()
    nmatches, nq = np.frombuffer(raw, np.int32, 2)
    ids = np.frombuffer(raw, np.int32, n, 8)
    pushed = np.frombuffer(raw, np.uint8, nk, 8 + 4 * n)
    assert np.array_equal(pushed != 0, got[4][0][0] == rc.ST_IN_VIEW) and nq == (got[4][0][0] == rc.ST_IN_VIEW).sum(), "the host gates push the entries the device has in view"
    assert nmatches == got[1]["n_additional"][0][0] and ids.tobytes() == got[2][0].tobytes(), (nmatches, np.flatnonzero(ids != got[2][0])[:8])


def test_the_wide_search_is_the_resident_mode_5_search_and_the_track_and_bow_rings_are_left_alone(rig):
    """orbm_track_frame_projected, mode 5, fed by a host projection at the pose solve 1 left (the model's, which the restatement's
    status bytes are held to): the same core, so the same table; and a call of orbq_relocalize behind it leaves the set's result
    ring as it was"""
    case = rc.family_case("wide_short")
    fs = rig.cfs[1]
    pool_rec, n, stride = case["pool"], case["n"], case["stride"]
    row = case["entries"].astype(np.int64)
    kfdesc = np.where((row >= 0)[:, None], pool_rec["desc"][np.maximum(row & ~rc.NO_VOTE, 0)], 0).astype(np.uint8)
    rig.put(fs, 0, kf_keys(case), kfdesc)
    rig.put(fs, 1, case["keys"], case["desc"])
    pool, store = new_world(rig, pool_rec, [case["entries"]], stride)
    got = call(rig, pool, store, [job(fs, 0, 1, 0, case)])
    ref = rc.ref_run(case)
    assert_job_equals_ref(got, 0, ref, "wide_short")
    assert got[1]["exit"][0] == rc.WIDE_SHORT
    cur = np.where((case["ids"] >= 0) & (got[3][0] != 1), case["ids"], -1)          # the point list behind solve 1's discard
    st, uvr, lvl, qid = rc.model_project(case, pool_rec, got[1]["opt"][0][0]["Tcw"], case["K"], set(int(i) for i in case["ids"][case["ids"] >= 0]), 10.0, rc.breaks())
    assert st.tobytes() == got[4][0][0].tobytes(), "the model's gates are the device's"
    fs.track_projected(1, 0, uvr, lvl, qvalid=(st == rc.ST_IN_VIEW).astype(np.uint8), t_occ=(cur >= 0).astype(np.uint8), th_dist=100, check_ori=True, mode=5)
    table, nm = fs.results()
    assign = table[0][:n].copy()
    assert nm[0] == got[1]["n_additional"][0][0] > 0
    want = np.where(assign >= 0, qid[np.maximum(assign, 0)], cur).astype(np.int32)
    assert want.tobytes() == got[2][0].tobytes(), np.flatnonzero(want != got[2][0])[:8]
    before = (table.copy(), nm.copy(), table.ctypes.data)
    host_member_equals_the_device(case, got, cur)
    # ... and the set's BoW ring: a SearchByBoW of the two slots issued in front of the call
    import trackref_cases as trc
    from orbslamm_amd import ORBVocabulary
    v = trc.vocabulary()
    G = ORBVocabulary(trc.VOC_K, trc.VOC_L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)
    for s in (0, 1):
        fs.compute_bow(G, s, 1, trc.LEVELSUP)
    fs.search_by_bow([0], [1], nnratio=0.75, check_ori=True)
    bt, bn = fs.bow_results()
    bow = (bt.copy(), bn.copy(), bt.ctypes.data)
    assert bn[0] > 0, "the BoW ring holds a table with matches in it"
    assert same_call(got, call(rig, pool, store, [job(fs, 0, 1, 0, case)]))
    t2, n2 = fs.results()
    assert t2.ctypes.data == before[2] and np.array_equal(t2, before[0]) and np.array_equal(n2, before[1]), "orbm_track_results returns what it returned before"
    b2, m2 = fs.bow_results()
    assert b2.ctypes.data == bow[2] and np.array_equal(b2, bow[0]) and np.array_equal(m2, bow[1]), "orbm_bow_results returns what it returned before"
    store.close(); pool.close()
