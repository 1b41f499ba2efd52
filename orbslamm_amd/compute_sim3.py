"""ctypes mirror of orby_compute_sim3 (include/orbslamm_computesim3.h): what LoopClosing::ComputeSim3 and
MultiMapper::Run do per candidate behind Sim3Solver::iterate -- SearchBySim3(pKF1, pKF2, vpMatches12, s, R, t, 7.5), then
OptimizeSim3(pKF1, pKF2, vpMatches12, gScm, 10, mbFixScale) -- for any number of candidates in one device call.

    r, = compute_sim3(matcher, pool, store, [dict(fs=fs, slot1=0, slot2=1, kf1=kf1, kf2=kf2, n1=N1, n2=N2, R12=R, t12=t, s12=s,
                                                  R1w=..., t1w=..., K1=..., R2w=..., t2w=..., K2=..., bounds1=..., bounds2=...,
                                                  m12_id=ids, m12_idx2=idx2, fix_scale=False)],
                      scale_factors, level_breaks(log_sf, 8), inv_level_sigma2)
    rs = compute_sim3_batch(matcher, pool, store, jobs, sf1, sf2, breaks1, breaks2, sigma1, sigma2)

The two keyframes are slots of one resident frame set (fs) and slots of the keyframe store (kf1, kf2); m12_id[i] is the pool id of
vpMatches12[i] as it enters (the solver's inliers) or -1, m12_idx2[i] its GetIndexInKeyFrame(pKF2) or -1 (both None: none).  S12
defaults to sim3_from_rts(R12, t12, s12), th to 7.5, th2 to 10.  Each result is a dict: n_found (SearchBySim3's return value), n_in
(OptimizeSim3's), S12 (the input's when written is False: the early return of Optimizer.cc:1514), written, match (the pKF2 feature of
vpMatches12[i] as OptimizeSim3 leaves it, or -1), ids (its pool id, or -1), removed (per correspondence), n_corr, n_bad, iterations,
trials, lambda_, chi2.  The verdict n_in >= 20 is the caller's."""
import numpy as np

from ._lib import K4, check, handle_value, lib, ptr, table
from .optimizer import SIM3_PROBLEM_DTYPE, SIM3_RESULT_DTYPE, sim3_from_rts

JOB_DTYPE = np.dtype([("fs", "<u8"), ("slot1", "<i4"), ("slot2", "<i4"), ("kf1", "<i4"), ("kf2", "<i4"), ("n1", "<i4"), ("n2", "<i4"),
                      ("prob", SIM3_PROBLEM_DTYPE), ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("bounds1", "<f4", (4,)),
                      ("bounds2", "<f4", (4,)), ("th", "<f4"), ("m12_id", "<u8"), ("m12_idx2", "<u8")])
RESULT_DTYPE = np.dtype([("opt", SIM3_RESULT_DTYPE), ("n_found", "<i4"), ("n_corr", "<i4")])
assert JOB_DTYPE.itemsize == 336 and RESULT_DTYPE.itemsize == 136
(ST_NO_POINT, ST_MARKED, ST_BAD, ST_DEPTH, ST_OUTSIDE_IMAGE, ST_DISTANCE, ST_LEVEL_RANGE, ST_NO_CANDIDATE, ST_FOUND) = range(9)


def pack_jobs(jobs):
    """(JOB_DTYPE array, the arrays it points into) from job dicts"""
    rec = np.zeros(len(jobs), dtype=JOB_DTYPE)
    keep = []
    for i, j in enumerate(jobs):
        rec["fs"][i] = handle_value(j["fs"])
        for k in ("slot1", "slot2", "kf1", "kf2", "n1", "n2"):
            rec[k][i] = j[k]
        R12, t12, s12 = np.asarray(j["R12"], np.float32).reshape(9), np.asarray(j["t12"], np.float32).reshape(3), np.float32(j["s12"])
        rec["R12"][i], rec["t12"][i], rec["s12"][i] = R12, t12, s12
        q, t, s = j["S12"] if j.get("S12") is not None else sim3_from_rts(R12.astype(np.float64).reshape(3, 3), t12.astype(np.float64), float(s12))
        pr = rec["prob"]
        pr["q"][i], pr["t"][i], pr["s"][i] = np.asarray(q, np.float64).reshape(4), np.asarray(t, np.float64).reshape(3), float(s)
        for k in ("R1w", "R2w"):
            pr[k][i] = np.asarray(j[k], np.float32).reshape(9)
        for k in ("t1w", "t2w"):
            pr[k][i] = np.asarray(j[k], np.float32).reshape(3)
        pr["K1"][i], pr["K2"][i] = K4(j["K1"]), K4(j["K2"] if j.get("K2") is not None else j["K1"])
        pr["th2"][i], pr["fix_scale"][i] = np.float32(j.get("th2", 10.0)), int(bool(j.get("fix_scale", False)))
        rec["bounds1"][i] = np.asarray(j["bounds1"], np.float32).reshape(4)
        rec["bounds2"][i] = np.asarray(j["bounds2"] if j.get("bounds2") is not None else j["bounds1"], np.float32).reshape(4)
        rec["th"][i] = np.float32(j.get("th", 7.5))
        for k in ("m12_id", "m12_idx2"):
            a = j.get(k)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
                assert a.shape[0] >= j["n1"]
                keep.append(a)
                rec[k][i] = a.ctypes.data
    return rec, keep


def compute_sim3_raw(handle, pool_handle, store_handle, jobs, sf1, sf2, breaks1, breaks2, sigma1, sigma2, nlevels=None, n_jobs=None, fill=None,
                     debug=True):
    """the C entry as it is: jobs a JOB_DTYPE array (or None).  Returns (rc, results, [match per job], [ids per job], [removed per job],
    [status per job or None], [vnMatch1 | vnMatch2 per job or None]); no exception on a refusal.  fill: the value the output arrays hold
    before the call (to see that a refusal leaves them alone); debug: ask for the status bytes and the vnMatch tables"""
    L = lib()
    real = 0 if jobs is None else jobs.shape[0]
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    sf1, sf2, breaks1, breaks2, sigma1, sigma2 = (f(a) for a in (sf1, sf2, breaks1, breaks2, sigma1, sigma2))
    nl = (0 if sigma1 is None else sigma1.shape[0]) if nlevels is None else int(nlevels)
    n1 = [max(int(jobs["n1"][i]), 0) for i in range(real)]
    n12 = [n1[i] + max(int(jobs["n2"][i]), 0) for i in range(real)]
    out = np.zeros(max(real, 1), dtype=RESULT_DTYPE)
    mk = lambda ns, dt, dflt: [np.full(max(n, 1), dflt if fill is None else fill, dt) for n in ns]   # noqa: E731
    match, ids, removed = mk(n1, np.int32, -2), mk(n1, np.int32, -2), mk(n1, np.uint8, 0)
    status, vn = (mk(n12, np.uint8, 0), mk(n12, np.int32, -2)) if debug else (None, None)
    rc = L.orby_compute_sim3(handle, pool_handle, store_handle, ptr(jobs), real if n_jobs is None else int(n_jobs), ptr(sf1), ptr(sf2), ptr(breaks1),
                             ptr(breaks2), ptr(sigma1), ptr(sigma2), nl, ptr(out), table(match), table(ids), table(removed),
                             table(status) if debug else None, table(vn) if debug else None)
    cut = lambda arrays, ns: None if arrays is None else [a[:n] for a, n in zip(arrays, ns)]   # noqa: E731
    return rc, out[:real], cut(match, n1), cut(ids, n1), cut(removed, n1), cut(status, n12), cut(vn, n12)


def compute_sim3_batch(matcher, pool, store, jobs, scale_factors1, scale_factors2, level_breaks1, level_breaks2, inv_level_sigma2_1,
                       inv_level_sigma2_2, debug=False):
    """every job (a candidate of one ComputeSim3, or a keyframe pair of a map merge) in one device call.  The caller walks the results
    in the reference's candidate order and stops at the first with n_in >= 20: the jobs behind it have run, which the reference does
    not do -- their results are simply not read."""
    rec, keep = pack_jobs(jobs)
    rc, out, match, ids, removed, status, vn = compute_sim3_raw(matcher._h, pool._h, store._h, rec if len(jobs) else None, scale_factors1, scale_factors2,
                                                                level_breaks1, level_breaks2, inv_level_sigma2_1, inv_level_sigma2_2, debug=debug)
    check(rc)
    res = []
    for i in range(len(jobs)):
        o = out["opt"][i]
        r = dict(n_found=int(out["n_found"][i]), n_in=int(o["n_in"]), S12=(o["q"].copy(), o["t"].copy(), float(o["s"])), written=bool(o["written"]),
                 match=match[i], ids=ids[i], n_corr=int(o["n_corr"]), removed=removed[i][:int(o["n_corr"])], n_bad=int(o["n_bad"]),
                 iterations=o["iterations"].copy(), trials=o["trials"].copy(), lambda_=o["lambda_"].copy(), chi2=o["chi2"].copy())
        if debug:
            n1 = int(rec["n1"][i])
            r.update(status1=status[i][:n1], status2=status[i][n1:], vn_match1=vn[i][:n1], vn_match2=vn[i][n1:])
        res.append(r)
    return res


def compute_sim3(matcher, pool, store, jobs, scale_factors, level_breaks, inv_level_sigma2, debug=False):
    """compute_sim3_batch for two keyframes that share their level tables (one extractor)"""
    return compute_sim3_batch(matcher, pool, store, jobs, scale_factors, scale_factors, level_breaks, level_breaks, inv_level_sigma2, inv_level_sigma2,
                              debug=debug)
