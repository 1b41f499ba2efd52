"""orbq_track_reference without a GPU: tools/trackref_ref.hpp, the restatement the device is held to, against an
independent numpy model of the validity rule, the masked merge, the gate and the loop -- by equality over every scene family, each
asserted to force the branch it is named after; the search between the two is the oracle's SearchByBoW with the validity array;
the gate at 14 and 15 matches, the verdict at 9 and 10 observed inliers; the records' sizes; and every refusal of the built library
that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import trackref_cases as rc
from orbslamm_amd import _lib
from orbslamm_amd.track_pose import REF_JOB_DTYPE, REF_RESULT_DTYPE, REF_SEARCH_ONLY, REF_TOO_FEW, REF_TRACKED, pack_ref_jobs, track_reference_raw

import trackpose_cases as tc


def assert_ref_equals_model(oracle, case, tag, solve=1, min_matches=15, **kw):
    match, nb, (rrc, out, ids_out, outl, br), valid = rc.ref_whole(oracle, case, solve, min_matches, **kw)
    mv, _ = rc.model_validity(case, kw.get("pool"), kw.get("entries"))
    assert np.array_equal(valid, mv), (tag, "validity", np.flatnonzero(valid != mv)[:8])
    m = rc.model_run(case, match, solve, min_matches, kw.get("pool"), kw.get("entries"))
    r = out[0]
    assert (int(r["status"]), int(r["n_bow"])) == (m["status"], m["n_bow"]), (tag, "status", r["status"], r["n_bow"], m["status"], m["n_bow"])
    if m["opt"] is None:
        want = np.zeros(1, tc.REF_RESULT["opt"])
        want["Tcw"][0] = np.asarray(case["Tcw"], np.float32).reshape(16)
        assert r["track"]["opt"].tobytes() == want[0].tobytes(), (tag, "no solve: zero but the pose as it came")
    else:
        assert r["track"]["opt"].tobytes() == m["opt"].tobytes(), (tag, "OrboResult")
    assert np.array_equal(ids_out, m["ids_out"]), (tag, "ids", np.flatnonzero(ids_out != m["ids_out"])[:8])
    assert np.array_equal(outl, m["outlier_out"]), (tag, "outlier")
    assert (int(r["track"]["n_matches"]), int(r["track"]["n_matches_map"])) == (m["n_matches"], m["n_matches_map"]), (tag, "counts")
    return match, nb, r, ids_out, outl, br, valid


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_restatement_equals_the_model_and_the_family_forces_its_branch(oracle, family):
    case = rc.family_case(family)
    match, nb, r, ids_out, outl, br, valid = assert_ref_equals_model(oracle, case, family)
    assert rc.BRANCH[family](br, r), (family, br, r)
    hit = match >= 0
    assert (match[hit] == case["src"][hit]).all(), "every match is the right one"
    assert valid[match[hit]].all(), "no match names a feature the rule skips"
    if family != "empty_kf":
        assert r["status"] == rc.TRACKED and nb > 150 and r["track"]["opt"]["rounds"] == 4 and r["track"]["n_matches_map"] >= 10
        assert_ref_equals_model(oracle, case, (family, "search only"), solve=0)
        assert_ref_equals_model(oracle, case, (family, "gate above"), min_matches=nb + 1)
    if family == "bad_points":
        # §8s's edges ignore the bad flag; the search does not: no matched id is a bad point
        assert not (case["pool"]["flags"][ids_out[ids_out >= 0]] & rc.FLAG_BAD).any()
    if family == "no_vote":
        assert (case["entries"][match[hit]] & rc.NO_VOTE).any() and (ids_out < rc.NO_VOTE).all()


def test_a_skipped_feature_changes_the_table(oracle):
    """the issue's check: with 80 % of the keyframe's features valid the all-valid table differs from the exact one; and where a
    skipped feature has a valid twin behind it in the same node, the exact table is not the all-valid one with holes either: the
    twin takes the frame feature the skipped one would have taken (ORBmatcher.cc:205-211)"""
    case = rc.make_case("mixed", 1)
    valid, _ = rc.ref_validity(case)
    assert valid.sum() == rc.N * 4 // 5
    m0, n0 = rc.oracle_search(oracle, case, None)
    m1, n1 = rc.oracle_search(oracle, case, valid)
    assert n1 > 150 and (m1 != m0).sum() > 20
    qa = np.flatnonzero(valid == 0)[:10]
    qb = np.flatnonzero(valid != 0)[-10:]
    assert (qa < qb).all()
    case["kdesc"][qb] = case["kdesc"][qa]
    case["kkeys"]["angle"][qb] = case["kkeys"]["angle"][qa]
    m0, n0 = rc.oracle_search(oracle, case, None)
    m1, n1 = rc.oracle_search(oracle, case, valid)
    masked = np.where((m0 >= 0) & (valid[np.maximum(m0, 0)] != 0), m0, -1)
    assert np.isin(m1, qb).sum() >= 5 and not np.isin(masked, qb).any()


def test_the_gate_at_14_and_15_matches(oracle):
    """validity cleared at matched keyframe features one at a time until the oracle counts 15, then 14"""
    for seed in (1, 2, 3):
        case = rc.make_case("all_valid", seed, n=40, nflip=20)
        voc = rc.oracle_voc(oracle, 8, 3)

        def search(v):
            O = voc
            fvq, fvt = O.transform(case["kdesc"], 1)[1], O.transform(case["desc"], 1)[1]
            m, n = oracle.search_by_bow(case["kdesc"], case["kkeys"]["angle"], v, fvq, case["desc"], case["keys"]["angle"], None, fvt, 0.7, True, True)
            return m.copy(), int(n)
        entries = case["entries"].copy()
        seen = {}
        for _ in range(case["nk"]):
            valid, _ = rc.ref_validity(case, entries=entries)
            m, n = search(valid)
            seen.setdefault(n, (m, entries.copy()))
            if n <= 14:
                break
            entries[m[m >= 0][0]] = -1
        if 14 in seen and 15 in seen:
            break
    assert 14 in seen and 15 in seen, sorted(seen)
    for n, status in ((15, rc.TRACKED), (14, rc.TOO_FEW)):
        m, ent = seen[n]
        rrc, out, ids_out, outl, br = rc.ref_run(case, m, entries=ent)
        mod = rc.model_run(case, m, entries=ent)
        assert rrc == 0 and out["n_bow"][0] == n and out["status"][0] == status == mod["status"] and br["gateTaken"] == (n == 14)
        assert np.array_equal(ids_out, mod["ids_out"]) and np.array_equal(outl, mod["outlier_out"])
        assert (out["track"]["opt"]["rounds"][0] > 0) == (n == 15)


def test_the_verdict_at_9_and_10_observed_inliers(oracle):
    """OBSERVED cleared on all but 10, then all but 9, of the inliers: the flags do not enter the solve, so the inlier set stands"""
    case = rc.family_case("all_valid")
    match, nb, (rrc, out, ids_out, outl, br), valid = rc.ref_whole(oracle, case)
    inl = ids_out[ids_out >= 0]
    assert len(inl) == out["track"]["n_matches"][0] > 30
    L = rc.ref_lib()
    for keep, verdict in ((10, 1), (9, 0)):
        pool = case["pool"].copy()
        pool["flags"][inl[keep:]] &= ~np.uint8(rc.FLAG_OBSERVED)
        r2 = rc.ref_run(case, match, pool=pool)
        assert r2[1]["track"]["opt"].tobytes() == out["track"]["opt"].tobytes() and np.array_equal(r2[2], ids_out)
        assert r2[1]["track"]["n_matches_map"][0] == keep and r2[1]["track"]["n_matches"][0] == len(inl)
        assert L.trackrefref_verdict(int(r2[1]["status"][0]), keep) == verdict
        assert rc.model_run(case, match, pool=pool)["n_matches_map"] == keep
    assert L.trackrefref_verdict(rc.TOO_FEW, 50) == 0


def test_what_the_restatement_refuses():
    case = rc.family_case("all_valid")
    m = np.full(case["n"], -1, np.int32)
    m[:20] = case["src"][:20]
    assert rc.ref_run(case, m)[0] == 0
    assert rc.ref_run(case, m, nlevels=1)[0] == -1                       # an edge's octave outside [0, nlevels)
    bad = m.copy()
    bad[0] = case["nk"]                                                  # a match that names no keyframe feature
    assert rc.ref_run(case, bad)[0] == -1
    ent = case["entries"].copy()
    ent[m[0]] = -1                                                       # a matched feature without a point
    assert rc.ref_run(case, m, entries=ent)[0] == -1


# ------------------------------------------------------------------ the built library
def one_job(**kw):
    j = dict(fs=0x1000, kf_slot=0, slot=1, kf=0, n=5, solve=1, Tcw=np.eye(4), K=[500, 500, 320, 240])
    j.update(kw)
    return pack_ref_jobs([j])


def refuse(code, jobs, sig=tc.sigma2(), min_matches=15, h=None, **kw):
    rc_, out, ids, flags, match = track_reference_raw(h, h, h, jobs, 0.7, 1, min_matches, sig, fill=7, **kw)
    assert rc_ == code, (rc_, _lib.lib().orbx_last_error())
    assert out.tobytes() == bytes(out.nbytes)
    assert all((a == 7).all() for a in ids) and all((a == 7).all() for a in flags) and all((a == 7).all() for a in match)


def test_the_library_declares_the_entry_and_its_records():
    assert _lib.declarations()["orbq_track_reference"].header == "orbslamm_trackpose.h" and hasattr(_lib.lib(), "orbq_track_reference")
    assert REF_JOB_DTYPE.itemsize == 112 and REF_RESULT_DTYPE.itemsize == 192 and rc.REF_RESULT.itemsize == 192
    assert [REF_JOB_DTYPE.fields[f][1] for f in ("fs", "kf_slot", "slot", "kf", "n", "solve", "frame")] == [0, 8, 12, 16, 20, 24, 28]
    assert [REF_RESULT_DTYPE.fields[f][1] for f in ("track", "n_bow", "status")] == [0, 184, 188]
    assert (REF_TRACKED, REF_TOO_FEW, REF_SEARCH_ONLY) == (rc.TRACKED, rc.TOO_FEW, rc.SEARCH_ONLY) == (0, 1, 2)
    # the entry stays out of orbslamm_hip.h's own text
    assert _lib.declarations()["orbq_track_reference"].header != "orbslamm_hip.h"


def test_refusals_that_need_no_gpu():
    E_INVALID, E_UNSUPPORTED = _lib.ORBX_E_INVALID, _lib.ORBX_E_UNSUPPORTED
    # zero jobs: ORBX_OK at once, whatever else is passed
    assert track_reference_raw(None, None, None, None, 0.7, 1, 15, None)[0] == 0
    rec = one_job()
    assert track_reference_raw(None, None, None, rec, 0.7, 1, 15, None, n_jobs=0)[0] == 0
    refuse(E_INVALID, rec, n_jobs=-1)
    refuse(E_UNSUPPORTED, rec, n_jobs=4097)                              # above ORBO_MAX_FRAMES (refused before any record is read)
    refuse(E_INVALID, None, n_jobs=1)                                    # null jobs
    refuse(E_INVALID, rec, sig=None)                                     # null sigma table
    for nl in (0, 17, -1):
        refuse(E_INVALID, rec, nlevels=nl)
    refuse(E_INVALID, rec, min_matches=-1)
    refuse(E_INVALID, one_job(fs=0))                                     # null frame set
    refuse(E_INVALID, one_job(n=-1))
    refuse(E_UNSUPPORTED, one_job(n=65536))                              # above ORBO_MAX_EDGES
    for solve in (-1, 2):
        refuse(E_INVALID, one_job(solve=solve))
    for k in ("kf_slot", "slot", "kf"):
        refuse(E_INVALID, one_job(**{k: -1}))
    refuse(E_UNSUPPORTED, np.concatenate([one_job(n=65535)] * 65))       # more than ORBO_MAX_CALL_EDGES features in one call
    # the argument checks pass: null handles are refused without a GPU
    refuse(E_INVALID, rec)
    assert b"null handle" in _lib.lib().orbx_last_error()
    L = _lib.lib()
    out = np.zeros(1, REF_RESULT_DTYPE)
    arr = (C.c_void_p * 1)(0)
    ok = (C.c_void_p * 1)(out.ctypes.data)
    for args in ((None, ok, ok), (out.ctypes.data, None, ok), (out.ctypes.data, ok, None), (out.ctypes.data, arr, ok), (out.ctypes.data, ok, arr)):
        rc_ = L.orbq_track_reference(None, None, None, rec.ctypes.data, 1, 0.7, 1, 15, tc.sigma2().ctypes.data, 8, *args, None)
        assert rc_ == E_INVALID, args
