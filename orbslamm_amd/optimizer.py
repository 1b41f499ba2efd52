"""Optimizer::PoseOptimization (src/Optimizer.cc:261-473), monocular, on the device: the motion-only Levenberg that Tracking
runs after every search, batched over frames in one launch (orbo_pose_optimize*, include/orbslamm_poseopt.h).

    r = pose_optimization(matcher, Tcw, K, keys_un, feature, Xw, inv_level_sigma2)        # one frame
    rs = pose_optimization_batch(matcher, [dict(Tcw=..., K=..., keys_un=..., feature=..., Xw=...), ...], inv_level_sigma2)

feature: the indices i with mvpMapPoints[i] set (and mvuRight[i] < 0), Xw their GetWorldPos().  A frame dict may carry
frame=F (an opaque device-resident frame of the matcher's device) in place of keys_un: nothing but the edges and the poses
goes up then.  Each result is a dict: Tcw (what SetPose gets), n_good (the return value), outlier (mvbOutlier per edge),
n_initial, rounds, iterations, trials, lambda_, chi2."""
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


def _setup(L):
    if getattr(L, "_orbo_ready", False):
        return
    vp = C.c_void_p
    tail = [C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.orbo_pose_optimize.argtypes = [vp, vp, vp, vp] + tail
    L.orbo_pose_optimize_frames.argtypes = [vp, vp, vp] + tail
    L._orbo_ready = True


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
    _setup(L)
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
