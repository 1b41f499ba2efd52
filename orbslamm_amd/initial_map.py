"""Tracking::CreateInitialMapMonocular from its bundle adjustment on (src/Tracking.cc:728-758), monocular, on the device:
the two-keyframe bundle adjustment, the median depth, the verdict and the rescaling in one call, batched over maps in one
launch (orbb_initial_map*, include/orbslamm_initmap.h).

    r = initial_map(matcher, Tcw1, Tcw2, K, keys_un1, keys_un2, matches12, P3D, inv_level_sigma2, scale_factors, fixed_first=True)
    rs = initial_map_batch(matcher, [dict(Tcw1=..., Tcw2=..., K=..., keys_un1=..., keys_un2=..., matches12=..., P3D=...,
                                          fixed_first=True, iterations=20, robust=True), ...], inv_level_sigma2, scale_factors)

matches12 is mvIniMatches (-1: none), P3D mvIniP3D.  An item may carry frame1=F1, frame2=F2 (opaque device-resident frames
of the matcher's device) in place of the two key arrays.  Each result is a dict: Tcw1, Tcw2 (4x4, adjusted), Ow1, Ow2,
Tcw2_scaled (4x4), median_depth, inv_median_depth, n_points, verdict (OK, RESET_DEPTH, RESET_TRACKED, RESET_NONFINITE),
iterations, trials, stop, chi2_first, chi2_last, lambda_, and points: a POINT_DTYPE array with one record per feature of the
initial frame (matched, pos, pos_scaled, normal, min_distance, max_distance, status).  The signatures are the header's
(_lib.declarations())."""
import ctypes as C

import numpy as np

from ._lib import K4, KP_DTYPE, check, lib, ptr, table

MAX_PROBLEMS = 256
MAX_FEATURES = 65535
MAX_ITERATIONS = 20
OK, RESET_DEPTH, RESET_TRACKED, RESET_NONFINITE = 0, 1, 2, 3
STOP_ITERATIONS, STOP_TRIALS, STOP_RHO_ZERO, STOP_FLAT = 0, 1, 2, 3

PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (12,)), ("Tcw2", "<f4", (12,)), ("K", "<f4", (4,)), ("fixed_first", "<i4"), ("fixed_second", "<i4"),
                          ("iterations", "<i4"), ("robust", "<i4"), ("n1", "<i4"), ("n2", "<i4")])
RESULT_DTYPE = np.dtype([("Tcw1", "<f4", (12,)), ("Tcw2", "<f4", (12,)), ("Ow1", "<f4", (3,)), ("Ow2", "<f4", (3,)), ("Tcw2_scaled", "<f4", (12,)),
                         ("median_depth", "<f4"), ("inv_median_depth", "<f4"), ("n_points", "<i4"), ("verdict", "<i4"), ("iterations", "<i4"),
                         ("trials", "<i4"), ("stop", "<i4"), ("_pad", "<i4"), ("chi2_first", "<f8"), ("chi2_last", "<f8"), ("lambda_", "<f8")])
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("pos_scaled", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                        ("max_distance", "<f4"), ("status", "u1"), ("matched", "u1"), ("_pad", "u1", (2,))])
assert PROBLEM_DTYPE.itemsize == 136 and RESULT_DTYPE.itemsize == 224 and POINT_DTYPE.itemsize == 48


def pack_problem(it):
    """one item's OrbbProblem record; n1 and n2 from its arrays (or as given, with resident frames)"""
    p = np.zeros(1, dtype=PROBLEM_DTYPE)
    p["Tcw1"][0] = np.asarray(it["Tcw1"], dtype=np.float32).reshape(-1)[:12]
    p["Tcw2"][0] = np.asarray(it["Tcw2"], dtype=np.float32).reshape(-1)[:12]
    p["K"][0] = K4(it["K"])
    p["fixed_first"][0] = 1 if it.get("fixed_first", True) else 0
    p["fixed_second"][0] = 1 if it.get("fixed_second", False) else 0
    p["iterations"][0] = int(it.get("iterations", 20))
    p["robust"][0] = 1 if it.get("robust", True) else 0
    p["n1"][0] = int(it["n1"]) if "n1" in it else len(it["matches12"])
    p["n2"][0] = int(it["n2"]) if "n2" in it else len(it["keys_un2"])
    return p[0]


def initial_map_raw(handle, problems, keys1, keys2, resident1, resident2, matches12, P3D, inv_level_sigma2, scale_factors, nlevels=None):
    """the C entries as they are: problems a PROBLEM_DTYPE array; keys1 / keys2 lists of KP_DTYPE arrays, or resident1 /
    resident2 lists of opaque frames; matches12 and P3D lists of arrays (None: a null in the table).  Returns (rc, results,
    [points per problem]); no exception on a refusal."""
    L = lib()
    problems = None if problems is None else np.ascontiguousarray(problems, dtype=PROBLEM_DTYPE)
    n = 0 if problems is None else problems.shape[0]
    sig = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, dtype=np.float32)
    sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, dtype=np.float32)
    nl = (0 if sig is None else sig.shape[0]) if nlevels is None else int(nlevels)
    m12 = None if matches12 is None else [None if m is None else np.ascontiguousarray(m, dtype=np.int32) for m in matches12]
    p3d = None if P3D is None else [None if p is None else np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in P3D]
    out = np.zeros(max(n, 1), dtype=RESULT_DTYPE)
    points = [np.zeros(max(int(problems["n1"][i]), 1), dtype=POINT_DTYPE) for i in range(n)]
    tm, tp, tpts = (None if m12 is None else table(m12)), (None if p3d is None else table(p3d)), table(points)
    if resident1 is not None or resident2 is not None:
        f1 = None if resident1 is None else (C.c_void_p * max(len(resident1), 1))(*resident1)
        f2 = None if resident2 is None else (C.c_void_p * max(len(resident2), 1))(*resident2)
        rc = L.orbb_initial_map_frames(handle, ptr(problems), n, f1, f2, tm, tp, ptr(sig), ptr(sf), nl, ptr(out), tpts)
    else:
        k1 = None if keys1 is None else [None if k is None else np.ascontiguousarray(k, dtype=KP_DTYPE) for k in keys1]
        k2 = None if keys2 is None else [None if k is None else np.ascontiguousarray(k, dtype=KP_DTYPE) for k in keys2]
        rc = L.orbb_initial_map(handle, ptr(problems), n, None if k1 is None else table(k1), None if k2 is None else table(k2), tm, tp, ptr(sig),
                                ptr(sf), nl, ptr(out), tpts)
    return rc, out[:n], [points[i][:int(problems["n1"][i])] for i in range(n)]


def _tcw44(T12):
    T = np.eye(4, dtype=np.float32)
    T[:3, :] = T12.reshape(3, 4)
    return T


def initial_map_batch(matcher, items, inv_level_sigma2, scale_factors):
    """the initial map of every item in one device call: see the module's docstring.  All items with key arrays or all with
    resident frames."""
    n = len(items)
    resident = [it.get("frame1") is not None for it in items]
    if any(resident) and not all(resident):
        raise ValueError("a batch takes resident frames or host arrays, not both")
    use_resident = n > 0 and resident[0]
    problems = np.zeros(n, dtype=PROBLEM_DTYPE)
    for i, it in enumerate(items):
        problems[i] = pack_problem(it)
    rc, out, points = initial_map_raw(matcher._h, problems, None if use_resident else [it["keys_un1"] for it in items],
                                      None if use_resident else [it["keys_un2"] for it in items],
                                      [it["frame1"] for it in items] if use_resident else None, [it["frame2"] for it in items] if use_resident else None,
                                      [it["matches12"] for it in items], [it["P3D"] for it in items], inv_level_sigma2, scale_factors)
    check(rc)
    return [dict(Tcw1=_tcw44(out["Tcw1"][i]), Tcw2=_tcw44(out["Tcw2"][i]), Ow1=out["Ow1"][i].copy(), Ow2=out["Ow2"][i].copy(),
                 Tcw2_scaled=_tcw44(out["Tcw2_scaled"][i]), median_depth=float(out["median_depth"][i]),
                 inv_median_depth=float(out["inv_median_depth"][i]), n_points=int(out["n_points"][i]), verdict=int(out["verdict"][i]),
                 iterations=int(out["iterations"][i]), trials=int(out["trials"][i]), stop=int(out["stop"][i]),
                 chi2_first=float(out["chi2_first"][i]), chi2_last=float(out["chi2_last"][i]), lambda_=float(out["lambda_"][i]), points=points[i])
            for i in range(n)]


def initial_map(matcher, Tcw1, Tcw2, K, keys_un1, keys_un2, matches12, P3D, inv_level_sigma2, scale_factors, fixed_first=True, iterations=20,
                robust=True, frame1=None, frame2=None):
    """one initial map: see initial_map_batch"""
    it = dict(Tcw1=Tcw1, Tcw2=Tcw2, K=K, matches12=matches12, P3D=P3D, fixed_first=fixed_first, iterations=iterations, robust=robust)
    if frame1 is not None:
        it.update(frame1=frame1, frame2=frame2, n1=len(matches12), n2=int(frame2_size(frame2)))
    else:
        it.update(keys_un1=keys_un1, keys_un2=keys_un2)
    return initial_map_batch(matcher, [it], inv_level_sigma2, scale_factors)[0]


def frame2_size(frame):
    """the feature count of an opaque device-resident frame"""
    return int(lib().orbm_frame_size(frame))
