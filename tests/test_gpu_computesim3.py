"""orby_compute_sim3 on the device: every output byte against the restatement (tools/computesim3_ref.hpp) over the scene
families -- result records, match_out, ids_out, removed, the status bytes and the two vnMatch tables; the solve against the existing
path (the matcher's resident window_best run twice, host agreement and walk, optimize_sim3 on the host-made list); one pair of 2 000
features; 8 jobs over two frame sets against the 8 single calls, and the same call twice; a pool update between two calls; the
refusals that need handles; and the drop-in on mocks.  A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import numpy as np
import pytest

import computesim3_cases as cc
import dropin
import localmap_cases as lc

from computesim3_cases import CAP, Rig, call, job, new_world

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -5
@pytest.fixture(scope="module")
def rig(gpu, oracle):
    return Rig(oracle)


def assert_job_equals_ref(got, j, ref, tag):
    rcode, out, match, ids, removed, status, vn = got
    assert rcode == 0, (tag, rcode)
    assert np.array_equal(vn[j], ref["vn"]), (tag, "vnMatch", np.flatnonzero(vn[j] != ref["vn"])[:8])
    assert status[j].tobytes() == ref["status"].tobytes(), (tag, "status", np.flatnonzero(status[j] != ref["status"])[:8])
    assert out[j].tobytes() == ref["res"][0].tobytes(), (tag, "OrbyResult", out[j], ref["res"][0])
    assert match[j].tobytes() == ref["match"].tobytes(), (tag, "match_out", np.flatnonzero(match[j] != ref["match"])[:8])
    assert ids[j].tobytes() == ref["ids"].tobytes(), (tag, "ids_out", np.flatnonzero(ids[j] != ref["ids"])[:8])
    assert removed[j].tobytes() == ref["removed"].tobytes(), (tag, "removed")


def assert_equals_existing_path(rig, frames, case, got, j, tag):
    """the matcher's resident window_best twice, the host agreement and walk, optimize_sim3 on the host-made list: the same core, so the
    same OrbzResult and removed bytes"""
    from orbslamm_amd import optimize_sim3

    def search(to, uvr, level, qdesc):
        return rig.m.window_best_frame(uvr, level, qdesc, None, frames[to - 1])
    m = cc.model_run(rig.oracle, case, search=search)
    o = got[1]["opt"][j]
    assert np.array_equal(got[6][j], m["vn"]), (tag, "the two tables of the existing searches")
    r = optimize_sim3(rig.m, m["item"], rig.sig)
    assert (int(o["written"]), int(o["n_corr"]), int(o["n_bad"]), int(o["n_in"])) == (int(r["written"]), r["n_corr"], r["n_bad"], r["n_in"]), tag
    q, t, s = r["S12"]
    assert o["q"].tobytes() == np.asarray(q, np.float64).tobytes() and o["t"].tobytes() == np.asarray(t, np.float64).tobytes() and o["s"] == s, (tag, "Sim3")
    for k in ("iterations", "trials", "lambda_", "chi2"):
        assert o[k].tobytes() == np.asarray(r[k]).tobytes(), (tag, k)
    assert np.array_equal(got[4][j][:r["n_corr"]], r["removed"]) and not got[4][j][r["n_corr"]:].any(), (tag, "removed")


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_families_equal_the_restatement_and_the_existing_path(rig, family):
    case, ref = cc.family_case(family), cc.family_ref(family)
    fs = rig.cfs[0]
    frames = rig.put_pair(fs, 0, 1, case, resident=True)
    pool, store = new_world(rig, case["pool"], [case["entries1"], case["entries2"]], case["stride"])
    got = call(rig, pool, store, [job(fs, 0, 1, 0, 1, case)])
    assert_job_equals_ref(got, 0, ref, family)
    assert cc.BRANCH[family](ref["br"], ref["res"][0]), (family, ref["br"])
    assert_equals_existing_path(rig, frames, case, got, 0, family)
    # without the debug copy-down: the same bytes otherwise
    bare = call(rig, pool, store, [job(fs, 0, 1, 0, 1, case)], debug=False)
    assert bare[0] == 0 and bare[5] is None and all(bare[k][0].tobytes() == got[k][0].tobytes() for k in (2, 3, 4)) and bare[1].tobytes() == got[1].tobytes()
    for f in frames:
        rig.m.frame_destroy(f)
    store.close(); pool.close()


def test_a_pair_of_2000_features(rig):
    """more than one edge per lane in the solve, 32 tiles a direction in the search, 32 chunks in the per-job walk"""
    n = 2000
    case = cc.make_case("inliers_in", 3, n=n)
    ref = cc.ref_run(case)
    assert ref["res"]["n_corr"][0] > 1000 and ref["res"]["opt"]["n_in"][0] > 500
    fs = rig.new_set(2048)
    rig.put_pair(fs, 2, 0, case)
    pool, store = new_world(rig, case["pool"], [case["entries1"], case["entries2"]], n)
    got = call(rig, pool, store, [job(fs, 2, 0, 0, 1, case)])
    assert_job_equals_ref(got, 0, ref, "2000")
    store.close(); pool.close(); fs.close()


def offset_case(case, base, records):
    c = dict(case, pool=records)
    for k in ("entries1", "entries2"):
        e = case[k]
        c[k] = np.where(e >= 0, e + base, -1).astype(np.int32)
    if case["m12_id"] is not None:
        c["m12_id"] = np.where(case["m12_id"] >= 0, case["m12_id"] + base, -1).astype(np.int32)
    return c


def test_batches_over_two_frame_sets_and_a_pool_update(rig):
    """8 jobs over two frame sets, keyframes named several times (also swapped: keyframe 2 as the current one); each job equal to itself
    alone; the same call twice; orbw_pool_set of moved points between two calls is seen by the second"""
    fams = ("inliers_in", "no_vote", "gross_outliers")
    cases = [cc.make_case(f, 4 + i) for i, f in enumerate(fams)]
    base = np.concatenate([[0], np.cumsum([len(c["pool"]) for c in cases])])
    records = np.concatenate([c["pool"] for c in cases])
    A, B, Cc = (offset_case(c, int(base[i]), records) for i, c in enumerate(cases))
    f0, f1 = rig.cfs
    rig.put_pair(f0, 0, 1, A)
    rig.put_pair(f0, 2, 3, B)
    rig.put_pair(f1, 0, 1, Cc)
    pool, store = new_world(rig, records, [A["entries1"], A["entries2"], B["entries1"], B["entries2"], Cc["entries1"], Cc["entries2"]], cc.N, kfcap=8)
    # a foreign pair: A's keyframe 1 against B's keyframe 2 under A's Sim3 (few matches: the early return)
    AB = dict(A, keys2=B["keys2"], desc2=B["desc2"], entries2=B["entries2"], m12_id=None, m12_idx2=None)
    empty = dict(A, n1=0, n2=0, keys1=A["keys1"][:0], keys2=A["keys2"][:0], desc1=A["desc1"][:0], desc2=A["desc2"][:0], m12_id=None, m12_idx2=None)
    spec = [(f0, 0, 1, 0, 1, A), (f0, 2, 3, 2, 3, B), (f1, 0, 1, 4, 5, Cc), (f0, 0, 3, 0, 3, AB), (f0, 0, 1, 0, 1, A), (f1, 0, 1, 4, 5, Cc),
            (f0, 0, 1, 0, 1, empty), (f0, 2, 3, 2, 3, B)]
    jobs = [job(*s) for s in spec]
    refs = [cc.ref_run(s[5]) for s in spec]
    assert refs[3]["res"]["opt"]["written"][0] == 0 and refs[6]["res"]["n_corr"][0] == 0 and refs[0]["res"]["opt"]["n_in"][0] >= 20
    got = call(rig, pool, store, jobs)
    for j in range(8):
        assert_job_equals_ref(got, j, refs[j], ("batch", j))
    again = call(rig, pool, store, jobs)
    assert again[1].tobytes() == got[1].tobytes() and all(a.tobytes() == b.tobytes() for k in range(2, 7) for a, b in zip(again[k], got[k]))
    for j in range(8):
        alone = call(rig, pool, store, [jobs[j]])
        assert alone[1][0].tobytes() == got[1][j].tobytes() and all(alone[k][0].tobytes() == got[k][j].tobytes() for k in range(2, 7)), ("alone", j)
    # moved points between two calls
    hit = np.flatnonzero(got[3][0] >= 0)[:12]
    moved = records.copy()
    pid = got[3][0][hit]
    moved["pos"][pid] += np.float32(0.7)
    pool.set(pid, moved[pid])
    after = call(rig, pool, store, [jobs[0]])
    assert_job_equals_ref(after, 0, cc.ref_run(A, pool=moved), "moved")
    assert after[1][0].tobytes() != got[1][0].tobytes()
    store.close(); pool.close()


def test_refusals_that_need_handles(rig):
    from orbslamm_amd import MapPool, ORBmatcher
    from orbslamm_amd.map_pool import KeyFrameStore
    case = cc.family_case("inliers_in")
    fs = rig.cfs[0]
    rig.put_pair(fs, 0, 1, case)
    pool, store = new_world(rig, case["pool"], [case["entries1"], case["entries2"]], case["stride"])

    def refused(jobs, what, code=E_INVALID, **kw):
        got = call(rig, *kw.pop("world", (pool, store)), jobs, fill=9, **kw)
        assert got[0] == code, (what, got[0])
        assert got[1].tobytes() == bytes(got[1].nbytes) and all((a == 9).all() for k in range(2, 7) for a in got[k]), what
    good = job(fs, 0, 1, 0, 1, case)
    assert call(rig, pool, store, [good])[0] == 0
    big = cc.make_case("all_new", 1, n=CAP + 1)
    refused([job(fs, 0, 1, 0, 1, big)], "n above the set's cap")
    refused([job(fs, 4, 1, 0, 1, case)], "slot1 outside the set")
    refused([job(fs, 0, 4, 0, 1, case)], "slot2 outside the set")
    refused([job(fs, 0, 1, 4, 1, case)], "kf1 outside the store")
    refused([job(fs, 0, 1, 0, 2, case)], "kf2 not set")
    refused([good, job(fs, 0, 1, 2, 1, case)], "a later job's kf1 not set")
    ids = case["m12_id"].copy()
    ids[np.flatnonzero(ids >= 0)[0]] = len(case["pool"])
    refused([job(fs, 0, 1, 0, 1, case, m12_id=ids)], "an m12_id outside the pool")
    pool2 = MapPool(rig.m, len(case["pool"]))
    store2 = KeyFrameStore(pool2, 2, 8, 0, 16)
    refused([good], "a store of another pool", world=(pool, store2))
    m2 = ORBmatcher(0.7, True, device=0)
    refused([good], "a frame set of another handle", m=m2)
    m2.close()
    # found by the kernel, reported behind it: an edge's octave outside [0, nlevels); a matched feature at or above a slot's device count
    refused([good], "octave outside nlevels", sig=rig.sig[:1], nlevels=1)
    short = dict(case)
    rig.put(fs, 2, case["keys2"][:200], case["desc2"][:200])
    refused([job(fs, 0, 2, 0, 1, short)], "an entering match at a feature the slot does not hold")
    assert call(rig, pool, store, [good])[0] == 0
    store2.close(); pool2.close(); store.close(); pool.close()


def test_computesim3_dropin_on_mock_keyframes(gpu):
    """include/LoopClosing_hip.hpp (ComputeSim3T::RunAll) on mocks (tests/cpp/computesim3_dropin_gpu.cpp, mock_computesim3.hpp) over three
    candidates against ORBmatcherT::SearchBySim3 + OptimizeSim3T::Run per candidate, the early-return job among them"""
    dropin.run(dropin.build("computesim3_dropin_gpu"), timeout=120, marker="computesim3 dropin ok")
