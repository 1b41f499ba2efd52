"""orbq_track_pose without a GPU: tools/trackpose_ref.hpp, the restatement the device is held to, against an
independent numpy model of the merge, the edge order and both loops (the solve is poseopt_cases.ref_run on the model's own edge
list) -- pose, counts and flags by equality over every scene family, each asserted to force the branch it is named after; the
two verdicts at their thresholds; and every refusal of the built library that needs no GPU."""
import numpy as np
import pytest

import trackpose_cases as tc
from orbslamm_amd import _lib
from orbslamm_amd.track_pose import JOB_DTYPE, TRACK_RESULT_DTYPE, pack_jobs, track_pose_raw


def assert_ref_equals_model(case, discard, tag, **kw):
    rc, out, ids_out, outl, br = tc.ref_run(case, discard, **kw)
    assert rc == 0, tag
    m = tc.model_run(case, discard, **{k: v for k, v in kw.items() if k in ("assign", "n")})
    assert out["opt"][0].tobytes() == m["opt"].tobytes(), (tag, "OrboResult", out["opt"][0], m["opt"])
    assert np.array_equal(ids_out, m["ids_out"]), (tag, "ids", np.flatnonzero(ids_out != m["ids_out"])[:8])
    assert np.array_equal(outl, m["outlier_out"]), (tag, "outlier")
    assert (int(out["n_matches"][0]), int(out["n_matches_map"][0])) == (m["n_matches"], m["n_matches_map"]), (tag, "counts")
    return out[0], ids_out, outl, br


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_restatement_equals_the_model_and_the_family_forces_its_branch(family):
    for case in tc.family_cases(family):
        tag = (family, case["seed"])
        r0, ids0, o0, b0 = assert_ref_equals_model(case, 0, tag + (0,))
        r1, ids1, o1, b1 = assert_ref_equals_model(case, 1, tag + (1,))
        assert tc.BRANCH[family](b0, b1, r0, r1), (tag, b0, b1)
        # the pose, the flags and the counts do not depend on the loop; the ids do exactly where a flag is set
        assert r0.tobytes() == r1.tobytes() and np.array_equal(o0, o1)
        assert np.array_equal(ids1, np.where(o0 != 0, -1, ids0))
        if family == "gross_outliers":
            assert not np.array_equal(ids0, ids1) and 40 <= r0["n_matches"] <= 62
        if family in ("base_only", "search_only", "search_overwrites_base"):
            assert r0["opt"]["rounds"] == 4 and r0["n_matches"] >= 55, (tag, r0)


def test_the_edge_list_ascends_by_feature_whatever_the_query_order():
    """the same matches listed in another query order: the same merged ids, so the same bytes"""
    case = dict(tc.family_cases("search_overwrites_base")[0])
    want = tc.ref_run(case, 0)
    perm = np.random.default_rng(3).permutation(len(case["ids"]))
    inv = np.argsort(perm)
    ids2 = case["ids"][perm]
    assign2 = np.where(case["assign"] >= 0, inv[np.maximum(case["assign"], 0)], -1).astype(np.int32)
    got = tc.ref_run(case, 0, assign=assign2, ids=ids2)
    assert got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_prefixes_of_a_frame():
    """n below the frame's feature count: the features behind n take no part"""
    case = tc.family_cases("search_overwrites_base")[0]
    for n in (0, 1, 63, 64, 65, case["n"]):
        assert_ref_equals_model(case, 1, ("prefix", n), n=n)


def test_what_the_restatement_refuses():
    case = tc.family_cases("search_only")[0]
    assert tc.ref_run(case, 0, nlevels=1)[0] == -1                       # an edge's octave outside [0, nlevels)
    bad = case["assign"].copy()
    bad[np.flatnonzero(bad >= 0)[0]] = len(case["ids"])                  # a match that names no query
    assert tc.ref_run(case, 0, assign=bad)[0] == -1
    ids = case["ids"].copy()
    ids[0] = -1                                                          # a matched query without a point
    assert tc.ref_run(case, 0, ids=ids)[0] == -1


def test_verdicts_at_their_thresholds():
    L = tc.ref_lib()
    for nm in (9, 10, 19, 20, 21, 49, 50):
        # TrackWithMotionModel: nmatchesMap >= 10; under mbOnlyTracking nmatches > 20 and mbVO = nmatchesMap < 10
        assert L.trackposeref_motion_model_verdict(100, nm, 0, None) == int(nm >= 10)
        vo = np.zeros(1, np.int32)
        assert L.trackposeref_motion_model_verdict(nm, 5 if nm % 2 else 15, 1, vo.ctypes.data) == int(nm > 20) and vo[0] == nm % 2
        # TrackLocalMap: 50 within mMaxFrames of a relocalisation, else 20; mnMatchesInliers is n_matches under mbOnlyTracking
        assert L.trackposeref_local_map_verdict(100, nm, 0, 100, 90, 30) == int(nm >= 50)
        assert L.trackposeref_local_map_verdict(100, nm, 0, 120, 90, 30) == int(nm >= 20)
        assert L.trackposeref_local_map_verdict(nm, 0, 1, 120, 90, 30) == int(nm >= 20)


# ------------------------------------------------------------------ the built library's refusals that need no GPU
def one_job(**kw):
    j = dict(fs=0x1000, slot=0, back=0, base_ids=None, n=5, discard=0, Tcw=np.eye(4), K=[500, 500, 320, 240])
    j.update(kw)
    return pack_jobs([j])


def refuse(code, jobs, sig=tc.sigma2(), **kw):
    rc, out, ids, flags = track_pose_raw(None, None, jobs, sig, fill=7, **kw)
    assert rc == code, (rc, _lib.lib().orbx_last_error())
    assert out.tobytes() == bytes(out.nbytes)
    assert all((a == 7).all() for a in ids) and all((a == 7).all() for a in flags)


def test_the_library_declares_the_entry_and_its_records():
    assert _lib.declarations()["orbq_track_pose"].header == "orbslamm_trackpose.h" and hasattr(_lib.lib(), "orbq_track_pose")
    assert JOB_DTYPE.itemsize == 112 and TRACK_RESULT_DTYPE.itemsize == 184 and tc.REF_RESULT.itemsize == 184


def test_refusals_that_need_no_gpu():
    E_INVALID, E_UNSUPPORTED = _lib.ORBX_E_INVALID, _lib.ORBX_E_UNSUPPORTED
    # zero jobs: ORBX_OK at once, whatever else is passed
    assert track_pose_raw(None, None, None, None)[0] == 0
    rec, keep = one_job()
    assert track_pose_raw(None, None, rec, None, n_jobs=0)[0] == 0
    refuse(E_INVALID, rec, n_jobs=-1)
    refuse(E_UNSUPPORTED, rec, n_jobs=4097)                              # above ORBO_MAX_FRAMES (refused before any record is read)
    refuse(E_INVALID, None, n_jobs=1)                                    # null jobs
    refuse(E_INVALID, rec, sig=None)                                     # null sigma table
    for nl in (0, 17, -1):
        refuse(E_INVALID, rec, nlevels=nl)
    refuse(E_INVALID, one_job(fs=0)[0])                                  # null frame set
    refuse(E_INVALID, one_job(n=-1)[0])
    refuse(E_UNSUPPORTED, one_job(n=65536)[0])                           # above ORBO_MAX_EDGES
    for back in (-2, 4):
        refuse(E_INVALID, one_job(back=back)[0])
    refuse(E_INVALID, one_job(discard=2)[0])
    # more than ORBO_MAX_CALL_EDGES features in one call
    many = np.concatenate([one_job(n=65535)[0]] * 65)
    refuse(E_UNSUPPORTED, many)
    # the argument checks pass: the handle's come next, and a null handle is refused without a GPU
    refuse(E_INVALID, rec)
    assert b"handle" in _lib.lib().orbx_last_error()
    L = _lib.lib()
    import ctypes as C
    out = np.zeros(1, TRACK_RESULT_DTYPE)
    arr = (C.c_void_p * 1)(0)
    ok = (C.c_void_p * 1)(out.ctypes.data)
    for args in ((None, ok, ok), (out.ctypes.data, None, ok), (out.ctypes.data, ok, None), (out.ctypes.data, arr, ok), (out.ctypes.data, ok, arr)):
        rc = L.orbq_track_pose(None, None, rec.ctypes.data, 1, tc.sigma2().ctypes.data, 8, *args)
        assert rc == E_INVALID, args
