"""ctypes mirror of orbq_track_pose, orbq_track_reference (include/orbslamm_trackpose.h), orbq_relocalize
(include/orbslamm_reloc.h, §8y) and orbq_track_motion_model (include/orbslamm_motion.h, §8z): Optimizer::PoseOptimization as Tracking calls
it right behind a pool search, with the loop that follows it, for any number of frames in one launch.

    pool.track_local_map(fs, slot, view, ids, 1.0, sf, breaks); fs.results()          # or store.track_local_map / track_frame_pose
    r, = track_pose(matcher, pool, [dict(fs=fs, slot=slot, back=0, base_ids=frame_ids, n=N, discard=0, Tcw=Tcw, K=K)], inv_level_sigma2)

back: which of the set's last searches to merge, as fs.results(back) counts them, or -1 for none; base_ids: the pool id of
mvpMapPoints[t] before that search (-1 = NULL; None = all NULL); discard: 1 for TrackWithMotionModel's loop, 0 for TrackLocalMap's.
Each result is a dict: Tcw (what SetPose gets), ids (mvpMapPoints as pool ids after the loop), outlier (mvbOutlier as
PoseOptimization left it), n_matches, n_matches_map, n_good, n_initial, rounds, iterations, trials, lambda_, chi2."""
import collections
import ctypes as C

import numpy as np

from ._lib import K4, check, handle_value, lib, ptr, table
from .optimizer import FRAME_DTYPE, RESULT_DTYPE

JOB_DTYPE = np.dtype([("fs", "<u8"), ("slot", "<i4"), ("back", "<i4"), ("base_ids", "<u8"), ("n", "<i4"), ("discard", "<i4"), ("frame", FRAME_DTYPE)])
TRACK_RESULT_DTYPE = np.dtype([("opt", RESULT_DTYPE), ("n_matches", "<i4"), ("n_matches_map", "<i4")])
assert JOB_DTYPE.itemsize == 112 and TRACK_RESULT_DTYPE.itemsize == 184


def pack_jobs(jobs):
    """(JOB_DTYPE array, the arrays it points into) from job dicts: fs (a FrameSet, or a raw handle value), slot, back, base_ids, n,
    discard, Tcw, K"""
    rec = np.zeros(len(jobs), dtype=JOB_DTYPE)
    keep = []
    for i, j in enumerate(jobs):
        rec["fs"][i] = handle_value(j["fs"])
        rec["slot"][i], rec["back"][i], rec["n"][i], rec["discard"][i] = j["slot"], j.get("back", 0), j["n"], j.get("discard", 0)
        base = j.get("base_ids")
        if base is not None:
            base = np.ascontiguousarray(base, dtype=np.int32).reshape(-1)
            assert base.shape[0] >= j["n"]
            keep.append(base)
            rec["base_ids"][i] = base.ctypes.data
        rec["frame"]["Tcw"][i] = np.asarray(j["Tcw"], dtype=np.float32).reshape(16)
        rec["frame"]["K"][i] = K4(j["K"])
    return rec, keep


def _cut(arrays, ns):
    return [None if a is None else a[:n] for a, n in zip(arrays, ns)]


_Raw = collections.namedtuple("_Raw", "n_jobs nlevels sigma out ns ids flags")


def _raw_arrays(jobs, inv_level_sigma2, nlevels, n_jobs, fill, result_dtype):
    """what both *_raw calls build alike: n_jobs and nlevels as the C entry gets them, the sigma table, one result record per job the
    array holds (`out`), its n per job (`ns`) and the per-job output arrays `ids` and `flags`, which hold `fill` (ids: -2, outlier: 0
    without one) and at least one element"""
    real = 0 if jobs is None else jobs.shape[0]
    sig = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, dtype=np.float32)
    ns = [max(int(jobs["n"][i]), 0) for i in range(real)]
    return _Raw(n_jobs=real if n_jobs is None else int(n_jobs), nlevels=(0 if sig is None else sig.shape[0]) if nlevels is None else int(nlevels),
                sigma=sig, out=np.zeros(max(real, 1), dtype=result_dtype), ns=ns,
                ids=[np.full(max(n, 1), -2 if fill is None else fill, np.int32) for n in ns],
                flags=[np.full(max(n, 1), 0 if fill is None else fill, np.uint8) for n in ns])


def _track_fields(t, ids, flags, i):
    """the fields of a result dict that both entries fill from a TRACK_RESULT_DTYPE record"""
    o = t["opt"]
    return dict(Tcw=o["Tcw"][i].reshape(4, 4).copy(), ids=ids[i], outlier=flags[i].astype(bool), n_matches=int(t["n_matches"][i]),
                n_matches_map=int(t["n_matches_map"][i]), n_good=int(o["n_good"][i]), n_initial=int(o["n_initial"][i]), rounds=int(o["rounds"][i]),
                iterations=o["iterations"][i].copy(), trials=o["trials"][i].copy(), lambda_=o["lambda_"][i].copy(), chi2=o["chi2"][i].copy())


def track_pose_raw(handle, pool_handle, jobs, inv_level_sigma2, nlevels=None, n_jobs=None, fill=None):
    """the C entry as it is: jobs a JOB_DTYPE array (or None).  Returns (rc, results, [ids per job], [outlier per job]); no exception
    on a refusal.  fill: the byte the output arrays hold before the call (to see that a refusal leaves them alone)"""
    L = lib()
    a = _raw_arrays(jobs, inv_level_sigma2, nlevels, n_jobs, fill, TRACK_RESULT_DTYPE)
    rc = L.orbq_track_pose(handle, pool_handle, ptr(jobs), a.n_jobs, ptr(a.sigma), a.nlevels, ptr(a.out), table(a.ids), table(a.flags))
    return rc, a.out[:len(a.ns)], _cut(a.ids, a.ns), _cut(a.flags, a.ns)


def track_pose(matcher, pool, jobs, inv_level_sigma2):
    """orbq_track_pose over job dicts (see the module's head); one result dict per job"""
    rec, keep = pack_jobs(jobs)
    rc, out, ids, flags = track_pose_raw(matcher._h, pool._h, rec, inv_level_sigma2)
    check(rc)
    return [_track_fields(out, ids, flags, i) for i in range(len(jobs))]


# ------------------------------------------------------------------ orbq_track_reference
REF_JOB_DTYPE = np.dtype([("fs", "<u8"), ("kf_slot", "<i4"), ("slot", "<i4"), ("kf", "<i4"), ("n", "<i4"), ("solve", "<i4"), ("frame", FRAME_DTYPE)], align=True)
REF_RESULT_DTYPE = np.dtype([("track", TRACK_RESULT_DTYPE), ("n_bow", "<i4"), ("status", "<i4")])
assert REF_JOB_DTYPE.itemsize == 112 and REF_RESULT_DTYPE.itemsize == 192
REF_TRACKED, REF_TOO_FEW, REF_SEARCH_ONLY = 0, 1, 2


def pack_ref_jobs(jobs):
    """REF_JOB_DTYPE array from job dicts: fs (a FrameSet, or a raw handle value), kf_slot, slot, kf, n, solve (default 1), Tcw, K"""
    rec = np.zeros(len(jobs), dtype=REF_JOB_DTYPE)
    for i, j in enumerate(jobs):
        rec["fs"][i] = handle_value(j["fs"])
        rec["kf_slot"][i], rec["slot"][i], rec["kf"][i], rec["n"][i], rec["solve"][i] = j["kf_slot"], j["slot"], j["kf"], j["n"], j.get("solve", 1)
        rec["frame"]["Tcw"][i] = np.asarray(j.get("Tcw", np.eye(4)), dtype=np.float32).reshape(16)
        rec["frame"]["K"][i] = K4(j.get("K", [1, 1, 0, 0]))
    return rec


def track_reference_raw(handle, pool_handle, store_handle, jobs, nnratio, check_ori, min_matches, inv_level_sigma2, nlevels=None, n_jobs=None,
                        fill=None, want_match=True):
    """the C entry as it is: jobs a REF_JOB_DTYPE array (or None).  Returns (rc, results, [ids per job], [outlier per job], [match table
    per job, or None]); no exception on a refusal.  fill: the byte the output arrays hold before the call.  want_match: True, False (a
    null match_out) or one bool per job (nulls inside it)"""
    L = lib()
    a = _raw_arrays(jobs, inv_level_sigma2, nlevels, n_jobs, fill, REF_RESULT_DTYPE)
    per = [bool(want_match)] * len(a.ns) if isinstance(want_match, bool) else [bool(w) for w in want_match]
    match = [np.full(max(n, 1), -2 if fill is None else fill, np.int32) if per[i] else None for i, n in enumerate(a.ns)]
    pm = table(match) if any(per) or not isinstance(want_match, bool) else None
    rc = L.orbq_track_reference(handle, pool_handle, store_handle, ptr(jobs), a.n_jobs, float(nnratio), int(bool(check_ori)), int(min_matches),
                                ptr(a.sigma), a.nlevels, ptr(a.out), table(a.ids), table(a.flags), pm)
    return rc, a.out[:len(a.ns)], _cut(a.ids, a.ns), _cut(a.flags, a.ns), _cut(match, a.ns)


def track_reference(matcher, pool, store, jobs, inv_level_sigma2, nnratio=0.7, check_ori=True, min_matches=15, want_match=True):
    """orbq_track_reference over job dicts (fs, kf_slot, slot, kf, n, solve, Tcw, K): Tracking::TrackReferenceKeyFrame from SearchByBoW to
    the loop behind PoseOptimization (solve = 0: Relocalization's first loop).  One result dict per job: status (REF_TRACKED, REF_TOO_FEW,
    REF_SEARCH_ONLY), n_bow, match (the keyframe feature per frame feature, or None), and track_pose's fields; the verdict
    n_matches_map >= 10 is the caller's"""
    rec = pack_ref_jobs(jobs)
    rc, out, ids, flags, match = track_reference_raw(matcher._h, pool._h, store._h, rec, nnratio, check_ori, min_matches, inv_level_sigma2, want_match=want_match)
    check(rc)
    return [dict(_track_fields(out["track"], ids, flags, i), status=int(out["status"][i]), n_bow=int(out["n_bow"][i]), match=match[i]) for i in range(len(jobs))]


# ------------------------------------------------------------------ orbq_relocalize
RELOC_JOB_DTYPE = np.dtype([("fs", "<u8"), ("slot", "<i4"), ("kf_slot", "<i4"), ("kf", "<i4"), ("n", "<i4"), ("ids", "<u8"), ("frame", FRAME_DTYPE)])
RELOC_RESULT_DTYPE = np.dtype([("opt", RESULT_DTYPE, (3,)), ("Tcw", "<f4", (16,)), ("exit", "<i4"), ("n_good", "<i4", (3,)), ("n_additional", "<i4", (2,))])
assert RELOC_JOB_DTYPE.itemsize == 112 and RELOC_RESULT_DTYPE.itemsize == 616
RELOC_REJECTED, RELOC_FIRST, RELOC_WIDE_SHORT, RELOC_SECOND, RELOC_NARROW_SHORT, RELOC_THIRD = range(6)
RELOC_KEEP = 0xff
RELOC_ST_NOT_RUN, RELOC_ST_NO_POINT, RELOC_ST_BAD, RELOC_ST_FOUND, RELOC_ST_OUT_OF_IMAGE, RELOC_ST_DISTANCE, RELOC_ST_LEVEL_RANGE, RELOC_ST_IN_VIEW = range(8)


def pack_reloc_jobs(jobs):
    """(RELOC_JOB_DTYPE array, the id arrays it points into) from job dicts: fs (a FrameSet, or a raw handle value), slot, kf_slot, kf,
    n, ids (the pool id of vvpMapPointMatches[i][t] where vbInliers[t], else -1; None: a null pointer), Tcw (PnP's pose), K"""
    rec = np.zeros(len(jobs), dtype=RELOC_JOB_DTYPE)
    keep = []
    for i, j in enumerate(jobs):
        rec["fs"][i] = handle_value(j["fs"])
        rec["slot"][i], rec["kf_slot"][i], rec["kf"][i], rec["n"][i] = j["slot"], j["kf_slot"], j["kf"], j["n"]
        ids = j.get("ids")
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
            assert ids.shape[0] >= j["n"]
            keep.append(ids)
            rec["ids"][i] = ids.ctypes.data
        rec["frame"]["Tcw"][i] = np.asarray(j.get("Tcw", np.eye(4)), dtype=np.float32).reshape(16)
        rec["frame"]["K"][i] = K4(j.get("K", [1, 1, 0, 0]))
    return rec, keep


def relocalize_raw(handle, pool_handle, store_handle, jobs, check_ori, inv_level_sigma2, scale_factors, level_breaks, stride, nlevels=None,
                   n_jobs=None, fill=None, want_status=True):
    """the C entry as it is: jobs a RELOC_JOB_DTYPE array (or None); stride: the store's (it sizes the status arrays).  Returns (rc,
    results, [ids per job], [outlier per job], [status (2, stride) per job, or None]); no exception on a refusal.  fill: the byte the
    output arrays hold before the call.  want_status: True, False (a null status_out) or one bool per job (nulls inside it)"""
    L = lib()
    a = _raw_arrays(jobs, inv_level_sigma2, nlevels, n_jobs, fill, RELOC_RESULT_DTYPE)
    sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, dtype=np.float32)
    br = None if level_breaks is None else np.ascontiguousarray(level_breaks, dtype=np.float32)
    per = [bool(want_status)] * len(a.ns) if isinstance(want_status, bool) else [bool(w) for w in want_status]
    status = [np.full((2, max(int(stride), 1)), 0 if fill is None else fill, np.uint8) if per[i] else None for i in range(len(a.ns))]
    ps = table(status) if any(per) or not isinstance(want_status, bool) else None
    rc = L.orbq_relocalize(handle, pool_handle, store_handle, ptr(jobs), a.n_jobs, int(check_ori), ptr(a.sigma), ptr(sf), ptr(br), a.nlevels,
                           ptr(a.out), table(a.ids), table(a.flags), ps)
    return rc, a.out[:len(a.ns)], _cut(a.ids, a.ns), _cut(a.flags, a.ns), [None if s is None else s[:, :int(stride)] for s in status]


def reloc_n_good(rec):
    """the nGood that Tracking.cc:1546 reads at the exit of a RELOC_RESULT_DTYPE record (orbq_reloc_n_good)"""
    e = int(rec["exit"])
    return int(rec["n_good"][2 if e == RELOC_THIRD else 1 if e in (RELOC_SECOND, RELOC_NARROW_SHORT) else 0])


def relocalize(matcher, pool, store, jobs, inv_level_sigma2, scale_factors, level_breaks, check_ori=True, want_status=False):
    """orbq_relocalize over job dicts (fs, slot, kf_slot, kf, n, ids, Tcw, K): the body of Tracking::Relocalization behind
    PnPsolver::iterate, per candidate.  One result dict per job: exit (RELOC_*), n_good (3), n_additional (2), opt (the three solves'
    records), Tcw (what mCurrentFrame.mTcw is left as), ids (mvpMapPoints as pool ids at the exit), outlier (bytes: 0, 1, or RELOC_KEEP
    where no solve of the job had the feature as an edge), status ((2, stride) bytes or None), n_good_at_exit and ok, the verdict of
    :1546 for a job on its own"""
    rec, keep = pack_reloc_jobs(jobs)
    rc, out, ids, flags, status = relocalize_raw(matcher._h, pool._h, store._h, rec, check_ori, inv_level_sigma2, scale_factors, level_breaks, store.stride,
                                                 want_status=want_status)
    check(rc)
    res = []
    for i in range(len(jobs)):
        ng = reloc_n_good(out[i])
        res.append(dict(exit=int(out["exit"][i]), n_good=out["n_good"][i].copy(), n_additional=out["n_additional"][i].copy(), opt=out["opt"][i].copy(),
                        Tcw=out["Tcw"][i].reshape(4, 4).copy(), ids=ids[i], outlier=flags[i], status=status[i], n_good_at_exit=ng,
                        ok=int(out["exit"][i]) != RELOC_REJECTED and ng >= 50))
    return res


def debug_reloc_arena(matcher, entries_per_job=-1):
    """orbq_debug_reloc_arena, for the overflow tests: sets the starting size of a job's share of the candidate arena (0: the default;
    -1: leaves it) and returns how many times the last relocalize on the matcher ran its chain"""
    L = lib()
    runs = C.c_int(0)
    check(L.orbq_debug_reloc_arena(matcher._h, int(entries_per_job), C.byref(runs)))
    return runs.value


# ------------------------------------------------------------------ orbq_track_motion_model
MOTION_JOB_DTYPE = np.dtype([("fs", "<u8"), ("cur_slot", "<i4"), ("last_slot", "<i4"), ("n", "<i4"), ("nq", "<i4"), ("last_ids", "<u8"),
                             ("velocity", "<f4", (16,)), ("last_Tcw", "<f4", (16,)), ("K", "<f4", (4,))])
MOTION_RESULT_DTYPE = np.dtype([("track", TRACK_RESULT_DTYPE), ("Tcw_pred", "<f4", (16,)), ("n_search", "<i4", (2,)), ("wide", "<i4"), ("status", "<i4")])
assert MOTION_JOB_DTYPE.itemsize == 176 and MOTION_RESULT_DTYPE.itemsize == 264
MM_TRACKED, MM_TOO_FEW = 0, 1
MM_ST_NOT_RUN = 0xff


def pack_motion_jobs(jobs):
    """(MOTION_JOB_DTYPE array, the id arrays it points into) from job dicts: fs (a FrameSet, or a raw handle value), cur_slot, last_slot,
    n, last_ids (the pool id of mLastFrame.mvpMapPoints[i], -1 where NULL or an outlier; None: a null pointer), nq (default: len(last_ids)),
    velocity (mVelocity), last_Tcw (mLastFrame.mTcw), K"""
    rec = np.zeros(len(jobs), dtype=MOTION_JOB_DTYPE)
    keep = []
    for i, j in enumerate(jobs):
        rec["fs"][i] = handle_value(j["fs"])
        rec["cur_slot"][i], rec["last_slot"][i], rec["n"][i] = j["cur_slot"], j["last_slot"], j["n"]
        ids = j.get("last_ids")
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
            keep.append(ids)
            rec["last_ids"][i] = ids.ctypes.data
        rec["nq"][i] = j["nq"] if "nq" in j else 0 if ids is None else ids.shape[0]
        assert ids is None or ids.shape[0] >= rec["nq"][i]
        rec["velocity"][i] = np.asarray(j.get("velocity", np.eye(4)), dtype=np.float32).reshape(16)
        rec["last_Tcw"][i] = np.asarray(j.get("last_Tcw", np.eye(4)), dtype=np.float32).reshape(16)
        rec["K"][i] = K4(j.get("K", [1, 1, 0, 0]))
    return rec, keep


def track_motion_model_raw(handle, pool_handle, jobs, th, min_matches, check_ori, inv_level_sigma2, scale_factors, nlevels=None, n_jobs=None,
                           fill=None, want_tables=True):
    """the C entry as it is: jobs a MOTION_JOB_DTYPE array (or None).  Returns (rc, results, [ids per job], [outlier per job], [assign
    table per job, or None], [status (2, nq) per job, or None]); no exception on a refusal.  fill: the byte the output arrays hold before
    the call.  want_tables: True, False (null assign_out and status_out) or one bool per job (nulls inside them)"""
    L = lib()
    a = _raw_arrays(jobs, inv_level_sigma2, nlevels, n_jobs, fill, MOTION_RESULT_DTYPE)
    sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, dtype=np.float32)
    per = [bool(want_tables)] * len(a.ns) if isinstance(want_tables, bool) else [bool(w) for w in want_tables]
    nqs = [max(int(jobs["nq"][i]), 0) for i in range(len(a.ns))]
    assign = [np.full(max(n, 1), -2 if fill is None else fill, np.int32) if per[i] else None for i, n in enumerate(a.ns)]
    status = [np.full((2, max(nq, 1)), 0 if fill is None else fill, np.uint8) if per[i] else None for i, nq in enumerate(nqs)]
    some = any(per) or not isinstance(want_tables, bool)
    rc = L.orbq_track_motion_model(handle, pool_handle, ptr(jobs), a.n_jobs, float(th), int(min_matches), int(check_ori), ptr(a.sigma), ptr(sf),
                                   a.nlevels, ptr(a.out), table(a.ids), table(a.flags), table(assign) if some else None, table(status) if some else None)
    # (the C side writes 2 * nq contiguous bytes: search 1's and then search 2's)
    status = [None if s is None else s.reshape(-1)[:2 * nq].reshape(2, nq) for s, nq in zip(status, nqs)]
    return rc, a.out[:len(a.ns)], _cut(a.ids, a.ns), _cut(a.flags, a.ns), _cut(assign, a.ns), status


def track_motion_model(matcher, pool, jobs, inv_level_sigma2, scale_factors, th=15.0, min_matches=20, check_ori=True, want_tables=False):
    """orbq_track_motion_model over job dicts (fs, cur_slot, last_slot, n, last_ids, velocity, last_Tcw, K): Tracking::TrackWithMotionModel
    from the pose product to the loop behind PoseOptimization, the retry with 2 * th included.  One result dict per job: status (MM_TRACKED,
    MM_TOO_FEW), Tcw_pred, n_search (2; -1 where the retry did not run), wide, assign and search_status (or None), and track_pose's fields;
    the verdicts of Tracking.cc:971-977 are the caller's"""
    rec, keep = pack_motion_jobs(jobs)
    rc, out, ids, flags, assign, status = track_motion_model_raw(matcher._h, pool._h, rec, th, min_matches, check_ori, inv_level_sigma2, scale_factors,
                                                                 want_tables=want_tables)
    check(rc)
    return [dict(_track_fields(out["track"], ids, flags, i), status=int(out["status"][i]), Tcw_pred=out["Tcw_pred"][i].reshape(4, 4).copy(),
                 n_search=out["n_search"][i].copy(), wide=int(out["wide"][i]), assign=assign[i], search_status=status[i]) for i in range(len(jobs))]


def debug_motion_arena(matcher, entries_per_job=-1):
    """orbq_debug_motion_arena, for the overflow tests: sets the starting size of a job's share of the candidate arena (0: the default;
    -1: leaves it) and returns how many times the last track_motion_model on the matcher ran its chain"""
    L = lib()
    runs = C.c_int(0)
    check(L.orbq_debug_motion_arena(matcher._h, int(entries_per_job), C.byref(runs)))
    return runs.value
