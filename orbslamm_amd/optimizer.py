"""Optimizer::PoseOptimization (src/Optimizer.cc:261-473), monocular, on the device: the motion-only Levenberg that Tracking
runs after every search, batched over frames in one launch (orbo_pose_optimize*, include/orbslamm_poseopt.h).

    r = pose_optimization(matcher, Tcw, K, keys_un, feature, Xw, inv_level_sigma2)        # one frame
    rs = pose_optimization_batch(matcher, [dict(Tcw=..., K=..., keys_un=..., feature=..., Xw=...), ...], inv_level_sigma2)

feature: the indices i with mvpMapPoints[i] set (and mvuRight[i] < 0), Xw their GetWorldPos().  A frame dict may carry
frame=F (an opaque device-resident frame of the matcher's device) in place of keys_un: nothing but the edges and the poses
goes up then.  Each result is a dict: Tcw (what SetPose gets), n_good (the return value), outlier (mvbOutlier per edge),
n_initial, rounds, iterations, trials, lambda_, chi2.

Optimizer::OptimizeSim3 (src/Optimizer.cc:1348-1543), monocular: the 7-dof Levenberg of LoopClosing::ComputeSim3 and
MultiMapper::Run, batched over loop / merge candidates in one launch (orbz_optimize_sim3, include/orbslamm_sim3opt.h, §8p).

    S12 = sim3_from_rts(R12, t12, s12)                                       # Eigen's Quaterniond(R): (q xyzw, t, s)
    r = optimize_sim3(matcher, dict(S12=S12, R1w=..., t1w=..., K1=..., R2w=..., t2w=..., K2=..., idx1=..., obs1=..., oct1=...,
                                    obs2=..., oct2=..., X1w=..., X2w=..., th2=10, fix_scale=False), inv_level_sigma2)
    rs = optimize_sim3_batch(matcher, [item, ...], inv_level_sigma2_1, inv_level_sigma2_2)

The correspondences are the survivors of the reference's walk (:1401-1440) in ascending i.  Each result is a dict: S12 (the
input's when written is False: the early return of :1514), n_in (the return value), written, removed (per correspondence: 0
kept, 1 nulled by the first check, 2 by the second), n_corr, n_bad, iterations, trials, lambda_, chi2."""
import ctypes as C

import numpy as np

from ._lib import K4, KP_DTYPE, check, lib, ptr

MAX_FRAMES = 4096
MAX_EDGES = 65535
MAX_CALL_EDGES = 1 << 22

FRAME_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("K", "<f4", (4,))])
EDGE_DTYPE = np.dtype([("feature", "<i4"), ("Xw", "<f4", (3,))])
RESULT_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("n_initial", "<i4"), ("n_good", "<i4"), ("rounds", "<i4"), ("iterations", "<i4", (4,)),
                         ("trials", "<i4", (4,)), ("_pad", "<i4"), ("lambda_", "<f8", (4,)), ("chi2", "<f8", (4,))])
assert FRAME_DTYPE.itemsize == 80 and EDGE_DTYPE.itemsize == 16 and RESULT_DTYPE.itemsize == 176

SIM3_MAX_PROBLEMS = 4096
SIM3_MAX_CORR = 32767
SIM3_MAX_CALL_CORR = 1 << 21

SIM3_PROBLEM_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("R1w", "<f4", (9,)), ("t1w", "<f4", (3,)), ("K1", "<f4", (4,)),
                               ("R2w", "<f4", (9,)), ("t2w", "<f4", (3,)), ("K2", "<f4", (4,)), ("th2", "<f4"), ("fix_scale", "<i4")])
SIM3_CORR_DTYPE = np.dtype([("idx1", "<i4"), ("obs1", "<f4", (2,)), ("oct1", "<i4"), ("obs2", "<f4", (2,)), ("oct2", "<i4"), ("X1w", "<f4", (3,)),
                            ("X2w", "<f4", (3,))])
SIM3_RESULT_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("written", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"),
                              ("n_in", "<i4"), ("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("lambda_", "<f8", (2,)), ("chi2", "<f8", (2,))])
assert SIM3_PROBLEM_DTYPE.itemsize == 200 and SIM3_CORR_DTYPE.itemsize == 52 and SIM3_RESULT_DTYPE.itemsize == 128


def pack_edges(feature, Xw):
    """the edges of one frame as an EDGE_DTYPE array"""
    feature = np.asarray(feature, dtype=np.int32).reshape(-1)
    e = np.zeros(feature.shape[0], dtype=EDGE_DTYPE)
    e["feature"] = feature
    e["Xw"] = np.asarray(Xw, dtype=np.float32).reshape(-1, 3)
    return e


def pose_optimize_raw(handle, frames, keys, resident, edge_start, edges, inv_level_sigma2, nlevels=None):
    """the C entries as they are: frames a FRAME_DTYPE array, keys a list of KP_DTYPE arrays or resident a list of opaque
    frames, edge_start (n_frames + 1) and edges (EDGE_DTYPE).  Returns (rc, results, outlier); no exception on a refusal."""
    L = lib()
    frames = None if frames is None else np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    nf = 0 if frames is None else frames.shape[0]
    es = None if edge_start is None else np.ascontiguousarray(edge_start, dtype=np.int32)
    edges = None if edges is None else np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    sig = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, dtype=np.float32)
    nl = (0 if sig is None else sig.shape[0]) if nlevels is None else int(nlevels)
    out = np.zeros(max(nf, 1), dtype=RESULT_DTYPE)
    flags = np.zeros(max(1, 0 if edges is None else edges.shape[0]), dtype=np.uint8)
    if resident is not None:
        fr = (C.c_void_p * max(len(resident), 1))(*resident)
        rc = L.orbo_pose_optimize_frames(handle, ptr(frames), fr, nf, ptr(es), ptr(edges), ptr(sig), nl, ptr(out), ptr(flags))
    else:
        keys = [np.ascontiguousarray(k, dtype=KP_DTYPE) for k in (keys or [])]
        kp = (C.c_void_p * max(len(keys), 1))(*[ptr(k) for k in keys])
        nk = np.array([k.shape[0] for k in keys] + [0], dtype=np.int32)
        rc = L.orbo_pose_optimize(handle, ptr(frames), kp if keys else None, ptr(nk) if keys else None, nf, ptr(es), ptr(edges), ptr(sig), nl,
                                  ptr(out), ptr(flags))
    return rc, out[:nf], flags[:0 if edges is None else edges.shape[0]]


def pose_optimization_batch(matcher, items, inv_level_sigma2):
    """PoseOptimization of every frame in items in one device call (relocalisation's candidates, or several robots' frames).
    items: dicts with Tcw (4x4), K (fx fy cx cy or 3x3), feature, Xw and keys_un (KP_DTYPE) or frame; all with keys_un or all
    with frame.  Returns one result dict per item."""
    n = len(items)
    frames = np.zeros(n, dtype=FRAME_DTYPE)
    edges, start = [], [0]
    for i, it in enumerate(items):
        frames["Tcw"][i] = np.asarray(it["Tcw"], dtype=np.float32).reshape(16)
        frames["K"][i] = K4(it["K"])
        edges.append(pack_edges(it["feature"], it["Xw"]))
        start.append(start[-1] + edges[-1].shape[0])
    resident = [it.get("frame") for it in items]
    if any(f is not None for f in resident) and not all(f is not None for f in resident):
        raise ValueError("a batch takes resident frames or host arrays, not both")
    use_resident = n > 0 and resident[0] is not None
    all_edges = np.concatenate(edges) if edges else np.zeros(0, dtype=EDGE_DTYPE)
    rc, out, flags = pose_optimize_raw(matcher._h, frames, None if use_resident else [it["keys_un"] for it in items],
                                       resident if use_resident else None, np.array(start, dtype=np.int32), all_edges, inv_level_sigma2)
    check(rc)
    return [dict(Tcw=out["Tcw"][i].reshape(4, 4).copy(), n_good=int(out["n_good"][i]), n_initial=int(out["n_initial"][i]),
                 rounds=int(out["rounds"][i]), iterations=out["iterations"][i].copy(), trials=out["trials"][i].copy(),
                 lambda_=out["lambda_"][i].copy(), chi2=out["chi2"][i].copy(), outlier=flags[start[i]:start[i + 1]].astype(bool))
            for i in range(n)]


def pose_optimization(matcher, Tcw, K, keys_un, feature, Xw, inv_level_sigma2, frame=None):
    """PoseOptimization(pFrame) of one frame: see pose_optimization_batch"""
    it = dict(Tcw=Tcw, K=K, feature=feature, Xw=Xw)
    if frame is not None:
        it["frame"] = frame
    else:
        it["keys_un"] = keys_un
    return pose_optimization_batch(matcher, [it], inv_level_sigma2)[0]


# ------------------------------------------------------------------ OptimizeSim3
def sim3_from_rts(R, t, s):
    """g2o::Sim3(R, t, s) as (q, t, s): Eigen's Quaterniond(R) in float64, coefficients x y z w (NOT normalised, as there)"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    q = np.zeros(4, dtype=np.float64)
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0.0:
        r = np.sqrt(tr + 1.0)
        q[3] = 0.5 * r
        r = 0.5 / r
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * r, (R[0, 2] - R[2, 0]) * r, (R[1, 0] - R[0, 1]) * r
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        r = np.sqrt(((R[i, i] - R[j, j]) - R[k, k]) + 1.0)
        q[i] = 0.5 * r
        r = 0.5 / r
        q[3] = (R[k, j] - R[j, k]) * r
        q[j] = (R[j, i] + R[i, j]) * r
        q[k] = (R[k, i] + R[i, k]) * r
    return q, np.asarray(t, dtype=np.float64).reshape(3).copy(), float(s)


def pack_sim3_problem(it):
    """one problem record (SIM3_PROBLEM_DTYPE, shape (1,)) from an item dict"""
    r = np.zeros(1, dtype=SIM3_PROBLEM_DTYPE)
    q, t, s = it["S12"]
    r["q"][0], r["t"][0], r["s"][0] = np.asarray(q, np.float64).reshape(4), np.asarray(t, np.float64).reshape(3), float(s)
    for k in ("R1w", "R2w"):
        r[k][0] = np.asarray(it[k], dtype=np.float32).reshape(9)
    for k in ("t1w", "t2w"):
        r[k][0] = np.asarray(it[k], dtype=np.float32).reshape(3)
    r["K1"][0], r["K2"][0] = K4(it["K1"]), K4(it["K2"])
    r["th2"][0], r["fix_scale"][0] = np.float32(it.get("th2", 10.0)), 1 if it.get("fix_scale") else 0
    return r


def pack_sim3_corrs(it):
    """the correspondences of one problem as a SIM3_CORR_DTYPE array"""
    idx1 = np.asarray(it["idx1"], dtype=np.int32).reshape(-1)
    c = np.zeros(idx1.shape[0], dtype=SIM3_CORR_DTYPE)
    c["idx1"] = idx1
    c["obs1"], c["obs2"] = np.asarray(it["obs1"], np.float32).reshape(-1, 2), np.asarray(it["obs2"], np.float32).reshape(-1, 2)
    c["oct1"], c["oct2"] = np.asarray(it["oct1"], np.int32).reshape(-1), np.asarray(it["oct2"], np.int32).reshape(-1)
    c["X1w"], c["X2w"] = np.asarray(it["X1w"], np.float32).reshape(-1, 3), np.asarray(it["X2w"], np.float32).reshape(-1, 3)
    return c


def optimize_sim3_raw(handle, problems, corr_start, corrs, inv_level_sigma2_1, inv_level_sigma2_2, nlevels=None):
    """the C entry as it is: problems a SIM3_PROBLEM_DTYPE array, corr_start (n_problems + 1), corrs (SIM3_CORR_DTYPE), the two
    keyframes' level tables.  Returns (rc, results, removed); no exception on a refusal."""
    L = lib()
    problems = None if problems is None else np.ascontiguousarray(problems, dtype=SIM3_PROBLEM_DTYPE)
    npb = 0 if problems is None else problems.shape[0]
    cs = None if corr_start is None else np.ascontiguousarray(corr_start, dtype=np.int32)
    corrs = None if corrs is None else np.ascontiguousarray(corrs, dtype=SIM3_CORR_DTYPE)
    s1 = None if inv_level_sigma2_1 is None else np.ascontiguousarray(inv_level_sigma2_1, dtype=np.float32)
    s2 = None if inv_level_sigma2_2 is None else np.ascontiguousarray(inv_level_sigma2_2, dtype=np.float32)
    nl = (0 if s1 is None else s1.shape[0]) if nlevels is None else int(nlevels)
    out = np.zeros(max(npb, 1), dtype=SIM3_RESULT_DTYPE)
    nc = 0 if corrs is None else corrs.shape[0]
    flags = np.zeros(max(1, nc), dtype=np.uint8)
    rc = L.orbz_optimize_sim3(handle, ptr(problems), npb, ptr(cs), ptr(corrs), ptr(s1), ptr(s2), nl, ptr(out), ptr(flags))
    return rc, out[:npb], flags[:nc]


def optimize_sim3_batch(matcher, items, inv_level_sigma2_1, inv_level_sigma2_2=None):
    """OptimizeSim3 of every item in one device call: the candidates of one ComputeSim3, or every keyframe pair of a map merge.
    The caller walks the results in the reference's candidate order and stops at the first with n_in >= 20."""
    n = len(items)
    s2 = inv_level_sigma2_1 if inv_level_sigma2_2 is None else inv_level_sigma2_2
    probs = np.concatenate([pack_sim3_problem(it) for it in items]) if n else np.zeros(0, dtype=SIM3_PROBLEM_DTYPE)
    corrs = [pack_sim3_corrs(it) for it in items]
    start = np.concatenate([[0], np.cumsum([c.shape[0] for c in corrs])]).astype(np.int32)
    allc = np.concatenate(corrs) if corrs else np.zeros(0, dtype=SIM3_CORR_DTYPE)
    rc, out, flags = optimize_sim3_raw(matcher._h, probs, start, allc, inv_level_sigma2_1, s2)
    check(rc)
    return [dict(S12=(out["q"][i].copy(), out["t"][i].copy(), float(out["s"][i])), n_in=int(out["n_in"][i]), written=bool(out["written"][i]),
                 n_corr=int(out["n_corr"][i]), n_bad=int(out["n_bad"][i]), iterations=out["iterations"][i].copy(), trials=out["trials"][i].copy(),
                 lambda_=out["lambda_"][i].copy(), chi2=out["chi2"][i].copy(), removed=flags[start[i]:start[i + 1]].copy())
            for i in range(n)]


def optimize_sim3(matcher, item, inv_level_sigma2_1, inv_level_sigma2_2=None):
    """OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) of one candidate: see optimize_sim3_batch"""
    return optimize_sim3_batch(matcher, [item], inv_level_sigma2_1, inv_level_sigma2_2)[0]
