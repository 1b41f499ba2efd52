"""orbq_relocalize without a GPU: tools/reloc_ref.hpp, the restatement the device is held to, against an independent
Python model of rules 1 to 7 (numpy float32 scalars and Python floats for the gates, the DEFINED solve of poseopt_cases on the model's
own edge list, the oracle's mode-5 search) -- by equality of bytes over every family, seeds 1..10, each seed asserted to reach the
exit and to force the counter the family is named after; the verdict; the records' layouts against the mirror; every refusal of the
built library that needs no GPU, with the outputs untouched."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import localmap_cases as lc
import ref_shim
import reloc_cases as rc

tp = importlib.import_module("orbslamm_amd.track_pose")   # (the package exports a function of the module's name)

E_INVALID, E_UNSUPPORTED = -1, -5


def assert_ref_equals_model(oracle, case, tag, **kw):
    r = rc.ref_run(case, **kw)
    m = rc.model_run(oracle, case, **kw)
    o = r[1][0]
    assert r[0] == 0, tag
    assert (int(o["exit"]), list(o["n_good"]), list(o["n_additional"])) == (m["exit"], m["n_good"], m["n_additional"]), (tag, o["exit"], o["n_good"], o["n_additional"], m)
    assert r[4].tobytes() == m["status"].tobytes(), (tag, "status", np.argwhere(r[4] != m["status"])[:8])
    assert r[2].tobytes() == m["ids_out"].tobytes(), (tag, "ids", np.flatnonzero(r[2] != m["ids_out"])[:8])
    assert r[3].tobytes() == m["outlier_out"].tobytes(), (tag, "outlier", np.flatnonzero(r[3] != m["outlier_out"])[:8])
    assert o["Tcw"].tobytes() == m["Tcw"].tobytes(), (tag, "Tcw")
    for k in range(3):
        want = m["opt"][k].tobytes() if k < len(m["opt"]) else bytes(o["opt"][k].nbytes)
        assert o["opt"][k].tobytes() == want, (tag, "opt", k)
    return r


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_restatement_equals_the_model_and_the_family_forces_its_branch(oracle, family):
    for seed in rc.SEEDS:
        case = rc.make_case(family, seed)
        rcode, out, ids_out, outl, status, br = assert_ref_equals_model(oracle, case, (family, seed))
        r = out[0]
        assert rc.BRANCH[family](br, r), (family, seed, br, r["exit"], r["n_good"], r["n_additional"])
        if family in rc.EXIT_OF:
            assert r["exit"] == rc.EXIT_OF[family], (family, seed, r["exit"])
        # what holds at every exit: a feature without a point never kept a fresh outlier flag's point, stages not reached are zero
        reached = {rc.REJECTED: 1, rc.FIRST: 1, rc.WIDE_SHORT: 1, rc.SECOND: 2, rc.NARROW_SHORT: 2, rc.THIRD: 3}[int(r["exit"])]
        assert all(r["opt"][k].tobytes() == bytes(r["opt"][k].nbytes) and r["n_good"][k] == 0 for k in range(reached, 3))
        assert (status[1] == rc.ST_NOT_RUN).all() == (r["exit"] not in (rc.NARROW_SHORT, rc.THIRD))
        assert (status[0] == rc.ST_NOT_RUN).all() == (r["exit"] in (rc.REJECTED, rc.FIRST))
        if r["exit"] in (rc.FIRST, rc.THIRD):
            assert not (outl[ids_out >= 0] == 1).any(), "behind a discard no feature with a point is an outlier"
        if r["exit"] not in (rc.WIDE_SHORT, rc.NARROW_SHORT):
            assert ((outl == rc.KEEP) <= (ids_out < 0)).all(), "behind a solve a feature that was never an edge holds no point"
        assert rc.ref_n_good(r) == tp.reloc_n_good(r)
        if family == "fewer_device_keys":
            # the points whose own feature lies behind the device count are projected into view and find nobody: it is not there
            gq = case["gone_q"]
            assert len(gq) >= 2 and (case["src"][gq] >= case["n_dev"]).all() and (status[0][gq] == rc.ST_IN_VIEW).all()
            assert not np.isin(case["entries"][gq], ids_out).any() and (ids_out[case["n_dev"]:] == -1).all() and (outl[case["n_dev"]:] == rc.KEEP).all()
            full = rc.ref_run(dict(case, n_dev=case["n"]))
            assert np.isin(case["entries"][gq], full[2]).all(), "with the whole frame on the device each of them is matched"
        hit = np.flatnonzero((ids_out >= 0) & (case["ids"] < 0))
        if family in ("first", "second_high", "third_succeeds", "no_vote"):
            assert (ids_out[hit] == case["own"][hit]).all() and (ids_out < rc.NO_VOTE).all(), "every added match is the feature's own point"


def test_check_ori_and_the_verdict(oracle):
    case = rc.make_case("rotation_pruned", 1)
    on, off = assert_ref_equals_model(oracle, case, "ori on", check_ori=True), assert_ref_equals_model(oracle, case, "ori off", check_ori=False)
    assert on[5]["nRotPruned"] >= 3 and off[5]["nRotPruned"] == 0 and off[1]["n_additional"][0][0] > on[1]["n_additional"][0][0]
    L = rc.ref_lib()
    for fam, want in (("rejected", 0), ("first", 1), ("wide_short", 0), ("second_high", 1), ("second_low", 0), ("narrow_short", 0), ("third_succeeds", 1), ("third_fails", 0)):
        r = rc.ref_run(rc.family_case(fam))[1]
        assert L.relocref_verdict(rc.p(r)) == want, fam
        assert (tp.reloc_n_good(r[0]) >= 50 and r["exit"][0] != rc.REJECTED) == bool(want), fam


def test_the_restatement_stands_alone():
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ref_shim.ROOT, "tools", "reloc_ref.hpp"))


def test_layouts():
    assert tp.RELOC_RESULT_DTYPE.itemsize == rc.REF_RESULT.itemsize == 616 and tp.RELOC_JOB_DTYPE.itemsize == 112
    for name in ("opt", "Tcw", "exit", "n_good", "n_additional"):
        assert tp.RELOC_RESULT_DTYPE.fields[name][1] == rc.REF_RESULT.fields[name][1], name
    assert [tp.RELOC_JOB_DTYPE.fields[k][1] for k in ("fs", "slot", "kf_slot", "kf", "n", "ids", "frame")] == [0, 8, 12, 16, 20, 24, 32]
    assert (tp.RELOC_REJECTED, tp.RELOC_FIRST, tp.RELOC_WIDE_SHORT, tp.RELOC_SECOND, tp.RELOC_NARROW_SHORT, tp.RELOC_THIRD) == \
        (rc.REJECTED, rc.FIRST, rc.WIDE_SHORT, rc.SECOND, rc.NARROW_SHORT, rc.THIRD)
    assert tp.RELOC_KEEP == rc.KEEP and tp.RELOC_ST_IN_VIEW == rc.ST_IN_VIEW and tp.RELOC_ST_NOT_RUN == rc.ST_NOT_RUN
    rec, keep = tp.pack_reloc_jobs([dict(fs=C.c_void_p(0x1000), slot=1, kf_slot=2, kf=3, n=4, ids=np.arange(4), Tcw=np.eye(4), K=lc.K_A)])
    assert rec["fs"][0] == 0x1000 and (rec["slot"][0], rec["kf_slot"][0], rec["kf"][0], rec["n"][0]) == (1, 2, 3, 4) and rec["ids"][0] == keep[0].ctypes.data
    assert rec["frame"]["Tcw"][0][5] == 1 and rec["frame"]["K"][0][0] == lc.K_A[0]


def test_refusals_that_need_no_gpu():
    """the argument checks come before the handles': the handle values below are never followed"""
    H_ = 0x10
    sig, sf, brk = rc.sigma2(), lc.SF, rc.breaks()

    def jobs(n=4, **kw):
        j = dict(fs=C.c_void_p(0x1000), slot=1, kf_slot=0, kf=0, n=max(n, 0), ids=np.full(max(n, 1), -1, np.int32), Tcw=np.eye(4), K=lc.K_A)
        j.update(kw)
        rec, keep = tp.pack_reloc_jobs([j])
        rec["n"][0] = n
        return rec, keep

    def refused(code, what, rec, h=H_, pool=H_, store=H_, check_ori=1, sig=sig, sf=sf, brk=brk, **kw):
        got = tp.relocalize_raw(h, pool, store, rec, check_ori, sig, sf, brk, 8, fill=9, **kw)
        assert got[0] == code, (what, got[0])
        assert got[1].tobytes() == bytes(got[1].nbytes) and all((a == 9).all() for k in (2, 3, 4) for a in got[k]), what
    rec, keep = jobs()
    assert tp.relocalize_raw(None, None, None, None, 1, None, None, None, 8, n_jobs=0)[0] == 0, "zero jobs: ORBX_OK at once, nothing read"
    refused(E_INVALID, "negative job count", rec, n_jobs=-1)
    refused(E_UNSUPPORTED, "too many jobs", rec, n_jobs=4097)
    refused(E_INVALID, "null jobs", None, n_jobs=1)
    refused(E_INVALID, "check_ori 2", rec, check_ori=2)
    refused(E_INVALID, "nlevels 0", rec, nlevels=0)
    refused(E_INVALID, "nlevels 17", rec, nlevels=17)
    refused(E_INVALID, "no sigma table", rec, sig=None, nlevels=8)
    refused(E_INVALID, "no scale table", rec, sf=None)
    refused(E_INVALID, "no break table", rec, brk=None)
    flat = brk.copy()
    flat[3] = flat[2]
    refused(E_INVALID, "a break table that does not ascend strictly", rec, brk=flat)
    refused(E_INVALID, "null frame set", jobs(fs=C.c_void_p(0))[0])
    refused(E_INVALID, "negative n", jobs(n=-1)[0])
    refused(E_UNSUPPORTED, "n above ORBO_MAX_EDGES", jobs(n=65536)[0])
    refused(E_INVALID, "negative slot", jobs(slot=-1)[0])
    refused(E_INVALID, "negative kf_slot", jobs(kf_slot=-1)[0])
    refused(E_INVALID, "negative kf", jobs(kf=-1)[0])
    refused(E_INVALID, "null ids", jobs(ids=None)[0])
    refused(E_INVALID, "null handle", rec, h=None)
    refused(E_INVALID, "null pool", rec, pool=None)
    refused(E_INVALID, "null store", rec, store=None)
    L = tp.lib()
    assert L.orbq_debug_reloc_arena(H_, -2, None) == E_INVALID and L.orbq_debug_reloc_arena(H_, (1 << 24) + 1, None) == E_INVALID
