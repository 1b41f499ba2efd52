"""orby_compute_sim3 without a GPU: tools/computesim3_ref.hpp, the restatement the device is held to, against an
independent numpy model of the marks, the gates, the agreement, the walk and the epilogue -- by equality over every scene family,
each asserted to force the branch it is named after; the two searches of the model are the oracle's window_best, its solve
sim3opt_ref.hpp on the model's own correspondence list; the conditions that keep the families honest; the verdict at 19 and 20
inliers; the records' sizes; and every refusal of the built library that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import computesim3_cases as cc
import localmap_cases as lc
from orbslamm_amd import _lib
from orbslamm_amd.compute_sim3 import JOB_DTYPE, RESULT_DTYPE, compute_sim3_raw, pack_jobs


def assert_ref_equals_model(oracle, case, ref, tag):
    m = cc.model_run(oracle, case)
    r = ref["res"][0]
    assert np.array_equal(ref["vn"], m["vn"]), (tag, "vnMatch", np.flatnonzero(ref["vn"] != m["vn"])[:8])
    assert np.array_equal(ref["status"], m["status"]), (tag, "status", np.flatnonzero(ref["status"] != m["status"])[:8])
    assert (int(r["n_found"]), int(r["n_corr"])) == (m["n_found"], m["n_corr"]), (tag, r["n_found"], r["n_corr"], m["n_found"], m["n_corr"])
    assert r["opt"].tobytes() == m["res"].tobytes(), (tag, "the solve on the model's list", r["opt"], m["res"])
    assert np.array_equal(ref["removed"], m["removed"]), (tag, "removed")
    assert np.array_equal(ref["match"], m["match"]), (tag, "match_out", np.flatnonzero(ref["match"] != m["match"])[:8])
    assert np.array_equal(ref["ids"], m["ids"]), (tag, "ids_out", np.flatnonzero(ref["ids"] != m["ids"])[:8])
    return m


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_restatement_equals_the_model_and_the_family_forces_its_branch(oracle, family):
    case, ref = cc.family_case(family), cc.family_ref(family)
    m = assert_ref_equals_model(oracle, case, ref, family)
    r, b = ref["res"][0], ref["br"]
    assert cc.BRANCH[family](b, r), (family, b, r)
    if family not in cc.DEGENERATE:
        assert r["n_found"] >= 50 and r["opt"]["n_in"] >= 20 and r["opt"]["written"] == 1, (family, r["n_found"], r["opt"]["n_in"])
        assert cc.ref_lib().computesim3ref_verdict(int(r["opt"]["n_in"])) == 1
    if not family.startswith("distance_range"):
        new = np.flatnonzero(m["new"])
        assert (ref["vn"][:case["n1"]][new] == case["true2"][new]).all(), "every new match is the true correspondence"
    if family == "no_vote":
        # a new match whose entry carries bit 30: it stays in the table and gets no edge
        nv = np.flatnonzero(m["new"] & (m["i2"] < 0))
        assert len(nv) >= 20 and (ref["match"][nv] >= 0).all() and (ref["ids"][nv] < cc.NO_VOTE).all() and not np.isin(nv, m["feat"]).any()
    if family == "bad_points":
        assert not (case["pool"]["flags"][ref["ids"][m["new"]]] & cc.FLAG_BAD).any()
    if family == "gross_outliers":
        wrong = np.flatnonzero((case["m12_idx2"] >= 0) & (case["m12_idx2"] != case["true2"]))
        assert len(wrong) == 25 and (ref["match"][wrong] == -1).sum() >= 15


def test_verdict_boundary():
    L = cc.ref_lib()
    assert L.computesim3ref_verdict(19) == 0 and L.computesim3ref_verdict(20) == 1


# ------------------------------------------------------------------ the built library
def one_job(**kw):
    j = dict(fs=0x1000, slot1=0, slot2=1, kf1=0, kf2=1, n1=5, n2=5, R12=np.eye(3), t12=np.zeros(3), s12=1.0, R1w=np.eye(3), t1w=np.zeros(3),
             R2w=np.eye(3), t2w=np.zeros(3), K1=[500, 500, 320, 240], bounds1=lc.BOUNDS, S12=(np.array([0, 0, 0, 1.0]), np.zeros(3), 1.0))
    j.update(kw)
    return pack_jobs([j])


def refuse(code, rec_keep, n_jobs=None, nlevels=None, **tables):
    rec = rec_keep[0] if isinstance(rec_keep, tuple) else rec_keep
    t = dict(sf1=lc.SF, sf2=lc.SF, breaks1=cc.breaks(), breaks2=cc.breaks(), sigma1=cc.sigma2(), sigma2=cc.sigma2())
    t.update(tables)
    got = compute_sim3_raw(None, None, None, rec, t["sf1"], t["sf2"], t["breaks1"], t["breaks2"], t["sigma1"], t["sigma2"], nlevels=nlevels, n_jobs=n_jobs, fill=7)
    assert got[0] == code, (got[0], _lib.lib().orbx_last_error())
    assert got[1].tobytes() == bytes(got[1].nbytes)
    assert all((a == 7).all() for k in (2, 3, 4, 5, 6) for a in got[k])


def test_the_library_declares_the_entry_and_its_records():
    assert _lib.declarations()["orby_compute_sim3"].header == "orbslamm_computesim3.h" and hasattr(_lib.lib(), "orby_compute_sim3")
    assert JOB_DTYPE.itemsize == 336 and RESULT_DTYPE.itemsize == 136 and cc.REF_RESULT.itemsize == 136
    assert [JOB_DTYPE.fields[f][1] for f in ("fs", "slot1", "slot2", "kf1", "kf2", "n1", "n2", "prob", "R12", "t12", "s12", "bounds1", "bounds2", "th", "m12_id", "m12_idx2")] == \
        [0, 8, 12, 16, 20, 24, 28, 32, 232, 268, 280, 284, 300, 316, 320, 328]
    assert [RESULT_DTYPE.fields[f][1] for f in ("opt", "n_found", "n_corr")] == [0, 128, 132]
    assert _lib.declarations()["orby_compute_sim3"].header != "orbslamm_hip.h"


def test_refusals_that_need_no_gpu():
    E_INVALID, E_UNSUPPORTED = _lib.ORBX_E_INVALID, _lib.ORBX_E_UNSUPPORTED
    # zero jobs: ORBX_OK at once, whatever else is passed
    assert compute_sim3_raw(None, None, None, None, None, None, None, None, None, None)[0] == 0
    rec = one_job()
    assert compute_sim3_raw(None, None, None, rec[0], None, None, None, None, None, None, n_jobs=0)[0] == 0
    refuse(E_INVALID, rec, n_jobs=-1)
    refuse(E_UNSUPPORTED, rec, n_jobs=4097)                              # above ORBZ_MAX_PROBLEMS (refused before any record is read)
    refuse(E_INVALID, None, n_jobs=1)                                    # null jobs
    for k in ("sf1", "sf2", "breaks1", "breaks2", "sigma1", "sigma2"):
        refuse(E_INVALID, rec, nlevels=8, **{k: None})                   # a null level table
    for nl in (0, 17, -1):
        refuse(E_INVALID, rec, nlevels=nl)
    flat = cc.breaks().copy()
    flat[3] = flat[2]
    refuse(E_INVALID, rec, breaks2=flat)                                 # a break table that does not ascend
    refuse(E_INVALID, one_job(fs=0))                                     # null frame set
    for k in ("n1", "n2"):
        refuse(E_INVALID, one_job(**{k: -1}))
        refuse(E_UNSUPPORTED, one_job(**{k: 32768}))                     # above ORBZ_MAX_CORR
    for k in ("slot1", "slot2", "kf1", "kf2"):
        refuse(E_INVALID, one_job(**{k: -1}))
    for v in (0.0, -1.0, np.inf, np.nan):
        refuse(E_INVALID, one_job(th2=v))
        refuse(E_INVALID, one_job(th=v))
        refuse(E_INVALID, one_job(s12=v))
    ids, idx = np.zeros(5, np.int32), np.zeros(5, np.int32)
    refuse(E_INVALID, one_job(m12_id=ids))                               # one of the two entering arrays alone
    for bad in (5, -2):
        idx2 = idx.copy()
        idx2[3] = bad
        refuse(E_INVALID, one_job(m12_id=ids, m12_idx2=idx2))            # an m12_idx2 >= n2, or below -1
    refuse(E_UNSUPPORTED, np.concatenate([one_job(n1=32767, n2=32767)[0]] * 33))   # more than ORBZ_MAX_CALL_CORR features in one call
    # the argument checks pass: null handles are refused without a GPU
    refuse(E_INVALID, rec)
    assert b"null handle" in _lib.lib().orbx_last_error()
    # null output arguments
    L = _lib.lib()
    out = np.zeros(1, RESULT_DTYPE)
    buf = np.zeros(8, np.int32)
    arr, ok = (C.c_void_p * 1)(0), (C.c_void_p * 1)(buf.ctypes.data)
    keep = [lc.SF, cc.breaks(), cc.sigma2()]
    tb = [keep[0].ctypes.data, keep[0].ctypes.data, keep[1].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[2].ctypes.data]
    for args in ((None, ok, ok), (out.ctypes.data, None, ok), (out.ctypes.data, ok, None), (out.ctypes.data, arr, ok), (out.ctypes.data, ok, arr)):
        rc_ = L.orby_compute_sim3(None, None, None, rec[0].ctypes.data, 1, *tb, 8, *args, None, None, None)
        assert rc_ == E_INVALID, args
