"""orbq_track_motion_model without a GPU: tools/motionmodel_ref.hpp, the restatement the device is held to, against an
independent model of rules 1 to 6 (the pose product in numpy float32 scalars summed left to right, tools/frustum_ref.hpp's frame/frame
gates, the oracle's mode-4 search, tools/trackpose_ref.hpp for the solve and the loop) -- by equality of bytes over every family,
seeds 1..5, each seed asserted to reach the exit and to force the counter the family is named after; the verdicts; the records'
layouts against the header and the mirror; every refusal of the built library that needs no GPU, with the outputs untouched."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import dropin
import localmap_cases as lc
import motionmodel_cases as mc
import ref_shim
import trackpose_cases as tc

tp = importlib.import_module("orbslamm_amd.track_pose")   # (the package exports a function of the module's name)

E_INVALID, E_UNSUPPORTED = -1, -5


def assert_ref_equals_model(oracle, case, tag, **kw):
    r = mc.ref_run(case, **kw)
    m = mc.model_run(oracle, case, **kw)
    o = r[1][0]
    assert r[0] == 0, tag
    assert (int(o["status"]), int(o["wide"]), list(o["n_search"])) == (m["status"], m["wide"], m["n_search"]), (tag, o["status"], o["wide"], o["n_search"], m["n_search"])
    assert o["Tcw_pred"].tobytes() == m["Tcw_pred"].tobytes(), (tag, "Tcw_pred")
    assert r[5].tobytes() == m["search_status"].tobytes(), (tag, "status", np.argwhere(r[5] != m["search_status"])[:8])
    assert r[4].tobytes() == m["assign"].tobytes(), (tag, "assign", np.flatnonzero(r[4] != m["assign"])[:8])
    assert r[2].tobytes() == m["ids_out"].tobytes(), (tag, "ids", np.flatnonzero(r[2] != m["ids_out"])[:8])
    assert r[3].tobytes() == m["outlier_out"].tobytes(), (tag, "outlier", np.flatnonzero(r[3] != m["outlier_out"])[:8])
    assert o["track"].tobytes() == m["track"].tobytes(), (tag, "track", o["track"], m["track"])
    return r


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_restatement_equals_the_model_and_the_family_forces_its_branch(oracle, family):
    L = tc.ref_lib()
    for seed in mc.SEEDS:
        case = mc.make_case(family, seed)
        code, out, ids_out, outl, assign, status, br = assert_ref_equals_model(oracle, case, (family, seed))
        r = out[0]
        assert mc.BRANCH[family](br, r), (family, seed, br, r["status"], r["n_search"], r["track"]["n_matches"], r["track"]["n_matches_map"])
        # what holds at every exit
        assert (status[1] == mc.ST_NOT_RUN).all() == (r["wide"] == 0) and not (status[0] == mc.ST_NOT_RUN).any()
        assert np.array_equal(assign >= 0, (ids_out >= 0) | (outl == 1)), "a feature holds a point, or lost it as an outlier, exactly where the table matched it"
        stands = r["n_search"][r["wide"]]
        assert stands >= (assign >= 0).sum(), "nmatches counts a feature once per point that took it"
        if r["status"] == mc.TOO_FEW:
            assert stands < mc.MIN_MATCHES and r["track"]["opt"]["rounds"] == 0 and r["track"]["opt"]["n_initial"] == 0 and not outl.any()
            assert r["track"]["opt"]["Tcw"].tobytes() == r["Tcw_pred"].tobytes() and r["track"]["n_matches_map"] == 0
            assert np.array_equal(ids_out, np.where(assign >= 0, case["last_ids"][np.maximum(assign, 0)], -1))
        else:
            assert stands >= mc.MIN_MATCHES and r["track"]["opt"]["n_initial"] == (assign >= 0).sum()
            assert not (outl[ids_out >= 0] == 1).any(), "behind the discard no feature with a point is an outlier"
        if family in ("map_9", "map_10"):
            # Tracking.cc:971-977 under both modes: the observed bits decide the mapping verdict and mbVO, never the only-tracking one
            want = family == "map_10"
            vo = C.c_int(-1)
            assert L.trackposeref_motion_model_verdict(int(r["track"]["n_matches"]), int(r["track"]["n_matches_map"]), 0, C.byref(vo)) == int(want)
            assert L.trackposeref_motion_model_verdict(int(r["track"]["n_matches"]), int(r["track"]["n_matches_map"]), 1, C.byref(vo)) == 1 and vo.value == int(not want)
        if family == "fewer_device_keys":
            gone = np.flatnonzero(case["src"] >= case["n_dev"])
            gone = gone[case["last_ids"][gone] >= 0]
            assert len(gone) >= 2 and (status[0][gone] == lc.ST_IN_VIEW).all() and not np.isin(gone, assign).any()
            assert (ids_out[case["n_dev"]:] == -1).all() and (assign[case["n_dev"]:] == -1).all()
            full = mc.ref_run(dict(case, n_dev=case["n"]))
            assert np.isin(gone, full[4]).all(), "with the whole frame on the device each of them is matched"
        if family == "first_enough":
            hit = np.flatnonzero(ids_out >= 0)
            assert (ids_out[hit] == case["own"][hit]).all(), "every match is the feature's own point"


def test_check_ori(oracle):
    case = mc.make_case("rotation_pruned", 1)
    on, off = assert_ref_equals_model(oracle, case, "ori on", check_ori=True), assert_ref_equals_model(oracle, case, "ori off", check_ori=False)
    assert on[6]["nRotPruned"] >= 3 and off[6]["nRotPruned"] == 0 and off[1]["n_search"][0][0] > on[1]["n_search"][0][0]


def test_the_product_rounds_as_a_float_sum_left_to_right():
    """a velocity with a real rotation: the float product differs from the double product narrowed, so the rounding is seen"""
    case = mc.make_case("velocity_rotation", 1)
    got = np.zeros(16, np.float32)
    mc.ref_lib().motionref_pose_product(mc.p(np.ascontiguousarray(case["velocity"])), mc.p(np.ascontiguousarray(case["last_Tcw"])), mc.p(got))
    assert got.tobytes() == mc.model_pose_product(case["velocity"], case["last_Tcw"]).tobytes()
    exact = (case["velocity"].astype(np.float64) @ case["last_Tcw"].astype(np.float64)).astype(np.float32).reshape(16)
    assert got.tobytes() != exact.tobytes() and np.abs(got - exact).max() < 1e-5
    assert mc.ref_run(case)[1]["Tcw_pred"][0].tobytes() == got.tobytes()


def test_other_thresholds(oracle):
    """th and min_matches are the call's: a min_matches of 0 never retries, one above the first count does"""
    case = mc.make_case("first_20", 2)
    r = assert_ref_equals_model(oracle, case, "min 0", min_matches=0)
    assert r[1]["wide"][0] == 0 and r[1]["status"][0] == mc.TRACKED
    r = assert_ref_equals_model(oracle, case, "min 21", min_matches=21)
    assert r[1]["wide"][0] == 1 and r[1]["n_search"][0][0] == 20
    r = assert_ref_equals_model(oracle, case, "th 7", th=7.0)
    assert r[0] == 0


def test_the_restatement_stands_alone():
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ref_shim.ROOT, "tools", "motionmodel_ref.hpp"))


def test_layouts():
    text = open(os.path.join(ref_shim.ROOT, "include", "orbslamm_motion.h")).read()
    job = re.search(r"typedef struct \{(.*?)\} OrbqMotionJob;", text, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", job, flags=re.S))
    assert names == ["fs", "cur_slot", "last_slot", "n", "nq", "last_ids", "velocity", "last_Tcw", "K"] == list(tp.MOTION_JOB_DTYPE.names)
    res = re.search(r"typedef struct \{([^{}]*)\} OrbqMotionResult;", text).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", res) == ["track", "Tcw_pred", "n_search", "wide", "status"] == list(tp.MOTION_RESULT_DTYPE.names)
    assert [tp.MOTION_JOB_DTYPE.fields[k][1] for k in tp.MOTION_JOB_DTYPE.names] == [0, 8, 12, 16, 20, 24, 32, 96, 160] and tp.MOTION_JOB_DTYPE.itemsize == 176
    assert tp.MOTION_RESULT_DTYPE.itemsize == mc.REF_RESULT.itemsize == 264
    for name in ("track", "Tcw_pred", "n_search", "wide", "status"):
        assert tp.MOTION_RESULT_DTYPE.fields[name][1] == mc.REF_RESULT.fields[name][1], name
    for name, value in (("ORBQ_MM_TRACKED", tp.MM_TRACKED), ("ORBQ_MM_TOO_FEW", tp.MM_TOO_FEW), ("ORBQ_MM_ST_NOT_RUN", tp.MM_ST_NOT_RUN)):
        assert int(re.search(r"#define %s (\w+)" % name, text).group(1), 0) == value, name
    assert (tp.MM_TRACKED, tp.MM_TOO_FEW, tp.MM_ST_NOT_RUN) == (mc.TRACKED, mc.TOO_FEW, mc.ST_NOT_RUN)
    assert ref_shim.declared("orbslamm_motion.h") == ["orbq_debug_motion_arena", "orbq_track_motion_model"]
    rec, keep = tp.pack_motion_jobs([dict(fs=C.c_void_p(0x1000), cur_slot=1, last_slot=2, n=4, last_ids=np.arange(5), velocity=np.eye(4), last_Tcw=2 * np.eye(4), K=lc.K_A)])
    assert rec["fs"][0] == 0x1000 and (rec["cur_slot"][0], rec["last_slot"][0], rec["n"][0], rec["nq"][0]) == (1, 2, 4, 5) and rec["last_ids"][0] == keep[0].ctypes.data
    assert rec["velocity"][0][5] == 1 and rec["last_Tcw"][0][5] == 2 and rec["K"][0][0] == lc.K_A[0]


def test_refusals_that_need_no_gpu():
    """the argument checks come before the handles': the handle values below are never followed"""
    H_ = 0x10
    sig, sf = mc.sigma2(), lc.SF

    def jobs(n=4, nq=4, **kw):
        j = dict(fs=C.c_void_p(0x1000), cur_slot=1, last_slot=0, n=max(n, 0), last_ids=np.full(max(nq, 1), -1, np.int32), velocity=np.eye(4), last_Tcw=np.eye(4), K=lc.K_A)
        j.update(kw)
        rec, keep = tp.pack_motion_jobs([j])
        rec["n"][0], rec["nq"][0] = n, nq
        return rec, keep

    def refused(code, what, rec, h=H_, pool=H_, th=15.0, min_matches=20, check_ori=1, sig=sig, sf=sf, **kw):
        got = tp.track_motion_model_raw(h, pool, rec, th, min_matches, check_ori, sig, sf, fill=9, **kw)
        assert got[0] == code, (what, got[0])
        assert got[1].tobytes() == bytes(got[1].nbytes) and all((a == 9).all() for k in (2, 3, 4, 5) for a in got[k] if a.size), what
    rec, keep = jobs()
    assert tp.track_motion_model_raw(None, None, None, 15.0, 20, 1, None, None, n_jobs=0)[0] == 0, "zero jobs: ORBX_OK at once, nothing read"
    refused(E_INVALID, "negative job count", rec, n_jobs=-1)
    refused(E_UNSUPPORTED, "too many jobs", rec, n_jobs=4097)
    refused(E_INVALID, "null jobs", None, n_jobs=1)
    refused(E_INVALID, "check_ori 2", rec, check_ori=2)
    refused(E_INVALID, "check_ori -1", rec, check_ori=-1)
    refused(E_INVALID, "negative min_matches", rec, min_matches=-1)
    for th in (0.0, -1.0, float("inf"), float("nan")):
        refused(E_INVALID, "th %r" % th, rec, th=th)
    refused(E_INVALID, "nlevels 0", rec, nlevels=0)
    refused(E_INVALID, "nlevels 17", rec, nlevels=17)
    refused(E_INVALID, "no sigma table", rec, sig=None, nlevels=8)
    refused(E_INVALID, "no scale table", rec, sf=None)
    refused(E_INVALID, "null frame set", jobs(fs=C.c_void_p(0))[0])
    refused(E_INVALID, "negative n", jobs(n=-1)[0])
    refused(E_INVALID, "negative nq", jobs(nq=-1)[0])
    refused(E_UNSUPPORTED, "n above ORBO_MAX_EDGES", jobs(n=65536)[0])
    many = np.concatenate([jobs(n=65535)[0]] * 65)
    refused(E_UNSUPPORTED, "more than ORBO_MAX_CALL_EDGES features in a call", many)
    refused(E_INVALID, "negative cur_slot", jobs(cur_slot=-1)[0])
    refused(E_INVALID, "negative last_slot", jobs(last_slot=-1)[0])
    refused(E_INVALID, "null last_ids", jobs(last_ids=None)[0])
    refused(E_INVALID, "null handle", rec, h=None)
    refused(E_INVALID, "null pool", rec, pool=None)
    L = tp.lib()
    assert L.orbq_debug_motion_arena(H_, -2, None) == E_INVALID and L.orbq_debug_motion_arena(H_, (1 << 24) + 1, None) == E_INVALID


def test_the_dropin_instantiates_on_its_mocks():
    """include/Tracking_hip.hpp's TrackWithMotionModelT::Run on the mock types, warnings as errors (it runs in tests/test_gpu_motionmodel.py)"""
    dropin.syntax_only("motionmodel_dropin_gpu")
