"""LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452, monocular) on the device, over the orbl_* block of
include/orbslamm_hip.h: one call searches the current keyframe against all its covisible neighbours,
triangulates every pair, applies the reference's gates and returns the new points in the reference's order.

    cur = dict(keys=mvKeysUn, desc=descriptors, fv=(node_id, start, idx), skip=has_map_point, kf=keyframe(...))
    nbs = [dict(keys=..., desc=..., fv=..., skip=..., kf=keyframe(..., median_depth=d)), ...]
    pts, status, f12 = create_new_map_points(matcher, cur, nbs, scale_factors, level_sigma2, 1.2)

With device-resident frames (ORBmatcher.frame_from_device + frame_compute_bow) a side is dict(frame=F, skip=..., kf=...).

LocalMapping::SearchInNeighbors (:454-534): fuse_batch runs the searches of ORBmatcher::Fuse for many target keyframes in
one call (orbl_fuse_batch*, include/orbslamm_fuse.h); level_breaks is the host-side table that stands in for PredictScale's log.

    tg = [fuse_target(Rcw, tcw, Ow, K, (0, 640, 0, 480), grid, keys=mvKeysUn, desc=descriptors), ...]   # or frame=F
    res = fuse_batch(matcher, tg, fuse_points(pos, normal, min_d, max_d, desc), (job_start, job_point), scale_factors,
                     inv_level_sigma2, level_breaks(np.log(np.float32(1.2)), 8))"""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, K4, OrbmFeatVec, OrbmGrid, check, lib, ptr

MAX_NEIGHBOURS = 32
(ST_NEIGHBOUR_SKIPPED, ST_FEATURE_SKIPPED, ST_NO_MATCH, ST_PARALLAX, ST_X3D_ZERO, ST_Z1, ST_Z2, ST_REPROJ1, ST_REPROJ2, ST_DIST_ZERO,
 ST_SCALE, ST_ACCEPTED) = range(12)
STATUS_NAMES = ("neighbour_skipped", "feature_skipped", "no_match", "parallax", "x3d_zero", "z1", "z2", "reproj1", "reproj2", "dist_zero",
                "scale", "accepted")

KF_DTYPE = np.dtype([("Rcw", "<f4", (3, 3)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("K", "<f4", (4,)), ("median_depth", "<f4")])
NEWPOINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)),
                           ("min_distance", "<f4"), ("max_distance", "<f4")])
assert KF_DTYPE.itemsize == 80 and NEWPOINT_DTYPE.itemsize == 44


def keyframe(Rcw, tcw, Ow, K, median_depth=0.0):
    """an OrblKeyFrame record: GetRotation, GetTranslation, GetCameraCenter as the reference's getters return them, K =
    (fx, fy, cx, cy) or the 3x3 matrix, and (for a neighbour) ComputeSceneMedianDepth(2)"""
    kf = np.zeros((), dtype=KF_DTYPE)
    kf["Rcw"] = np.asarray(Rcw, dtype=np.float32).reshape(3, 3)
    kf["tcw"] = np.asarray(tcw, dtype=np.float32).reshape(3)
    kf["Ow"] = np.asarray(Ow, dtype=np.float32).reshape(3)
    kf["K"] = K4(K)
    kf["median_depth"] = np.float32(median_depth)
    return kf


def compute_f12(kf1, kf2):
    """ComputeF12(pKF1, pKF2) and SearchForTriangulation's epipole in cv::Mat arithmetic (host; needs no GPU): F12 (3x3), (ex, ey)"""
    L = lib()
    a, b = np.ascontiguousarray(kf1, dtype=KF_DTYPE), np.ascontiguousarray(kf2, dtype=KF_DTYPE)
    F, e = np.zeros((3, 3), np.float32), np.zeros(2, np.float32)
    check(L.orbl_compute_f12(ptr(a), ptr(b), ptr(F), ptr(e)))
    return F, e


def _skip(side, n):
    s = side.get("skip")
    if s is None:
        return None
    s = np.ascontiguousarray(s, dtype=np.uint8).reshape(-1)
    if s.shape[0] != n:
        raise ValueError("skip has %d flags for %d features" % (s.shape[0], n))
    return s


def _ptr_array(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[None if a is None else a.ctypes.data for a in arrays])


def create_new_map_points(matcher, cur, neighbours, scale_factors, level_sigma2, scale_factor, check_ori=False, capacity=None,
                          want_status=True, want_f12=True):
    """CreateNewMapPoints for one keyframe.  Returns (points, status, f12): points a NEWPOINT_DTYPE array in the
    reference's order, status the (n_neighbours, n1) table of ST_* codes (None unless want_status), f12 the
    (n_neighbours, 11) F12 and epipole each processed neighbour's search used (None unless want_f12).  Raises OrbError
    (ORBX_E_CAPACITY, e.needed = the count) when capacity is given and too small."""
    L = lib()
    K = len(neighbours)
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    sg = np.ascontiguousarray(level_sigma2, dtype=np.float32).reshape(-1)
    if sf.shape[0] != sg.shape[0]:
        raise ValueError("scale_factors and level_sigma2 differ in length")
    kf1 = np.ascontiguousarray(cur["kf"], dtype=KF_DTYPE)
    kf2 = np.zeros(max(K, 1), dtype=KF_DTYPE)
    for k, nb in enumerate(neighbours):
        kf2[k] = nb["kf"]
    frames = "frame" in cur
    if any(("frame" in nb) != frames for nb in neighbours):
        raise ValueError("device-resident frames and host arrays cannot be mixed in one call")
    n1 = L.orbm_frame_size(cur["frame"]) if frames else np.ascontiguousarray(cur["keys"], dtype=KP_DTYPE).shape[0]
    cap = n1 if capacity is None else int(capacity)
    out = np.zeros(max(cap, 1), dtype=NEWPOINT_DTYPE)
    status = np.zeros((K, n1), dtype=np.uint8) if want_status else None
    f12 = np.zeros((K, 11), dtype=np.float32) if want_f12 else None
    n_new = C.c_int(0)
    s1 = _skip(cur, n1)
    if frames:
        n2 = [L.orbm_frame_size(nb["frame"]) for nb in neighbours]
        s2 = [_skip(nb, n2[k]) for k, nb in enumerate(neighbours)]
        f2 = (C.c_void_p * max(K, 1))(*[nb["frame"].value if isinstance(nb["frame"], C.c_void_p) else nb["frame"] for nb in neighbours])
        rc = L.orbl_create_new_map_points_frames(matcher._h, cur["frame"], ptr(s1), ptr(kf1), f2, _ptr_array(s2), ptr(kf2), K, ptr(sf), ptr(sg),
                                                 sf.shape[0], C.c_float(scale_factor), int(bool(check_ori)), ptr(out), cap, C.byref(n_new),
                                                 ptr(status), ptr(f12))
    else:
        def arrays(side):
            return (np.ascontiguousarray(side["keys"], dtype=KP_DTYPE), np.ascontiguousarray(side["desc"], dtype=np.uint8).reshape(-1, 32),
                    tuple(np.ascontiguousarray(a, dtype=t) for a, t in zip(side["fv"], (np.uint32, np.int32, np.int32))))
        k1, d1, v1 = arrays(cur)
        fv1 = OrbmFeatVec(v1[0].shape[0], *[a.ctypes.data for a in v1])
        sides = [arrays(nb) for nb in neighbours]
        n2a = np.array([s[0].shape[0] for s in sides] or [0], dtype=np.int32)
        s2 = [_skip(nb, int(n2a[k])) for k, nb in enumerate(neighbours)]
        fv2 = (OrbmFeatVec * max(K, 1))(*[OrbmFeatVec(s[2][0].shape[0], *[a.ctypes.data for a in s[2]]) for s in sides])
        rc = L.orbl_create_new_map_points(matcher._h, ptr(k1), ptr(d1), n1, C.byref(fv1), ptr(s1), ptr(kf1), _ptr_array([s[0] for s in sides]),
                                          _ptr_array([s[1] for s in sides]), ptr(n2a), fv2, _ptr_array(s2), ptr(kf2), K, ptr(sf), ptr(sg),
                                          sf.shape[0], C.c_float(scale_factor), int(bool(check_ori)), ptr(out), cap, C.byref(n_new),
                                          ptr(status), ptr(f12))
    if rc != 0:
        try:
            check(rc)
        except Exception as e:
            e.needed = n_new.value
            raise
    return out[:n_new.value].copy(), status, f12


# ------------------------------------------------------------------------------------------------ SearchInNeighbors
FUSE_MAX_TARGETS = 128
FUSE_MAX_JOBS = 1 << 22
(FUSE_ST_DEPTH, FUSE_ST_OUTSIDE_IMAGE, FUSE_ST_DISTANCE, FUSE_ST_VIEW_ANGLE, FUSE_ST_LEVEL_RANGE, FUSE_ST_NO_CANDIDATE,
 FUSE_ST_FOUND) = range(7)
FUSE_STATUS_NAMES = ("depth", "outside_image", "distance", "view_angle", "level_range", "no_candidate", "found")

GRID_DTYPE = np.dtype([("minX", "<f4"), ("minY", "<f4"), ("invW", "<f4"), ("invH", "<f4"), ("cols", "<i4"), ("rows", "<i4")])
FUSE_TARGET_DTYPE = np.dtype([("Rcw", "<f4", (3, 3)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("K", "<f4", (4,)),
                              ("bounds", "<f4", (4,)), ("grid", GRID_DTYPE)])
FUSE_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                             ("desc", "u1", (32,))])
FUSE_RESULT_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i4"), ("u", "<f4"), ("v", "<f4"), ("level", "i1"), ("status", "u1"),
                              ("pad", "u1", (2,))])
assert FUSE_TARGET_DTYPE.itemsize == 116 and FUSE_POINT_DTYPE.itemsize == 64 and FUSE_RESULT_DTYPE.itemsize == 20
PREDICT_FN = C.CFUNCTYPE(C.c_int, C.c_float, C.c_float)


def level_breaks(log_scale_factor, nlevels, predict=None):
    """orbl_level_breaks (host; needs no GPU): nlevels + 1 floats, entry L + 1 the largest ratio whose PredictScale level is
    <= L.  predict: the tree's own PredictScale as a Python callable (ratio, log_scale_factor) -> int; None: the float form"""
    L = lib()
    out = np.zeros(int(nlevels) + 1, np.float32)
    fn = PREDICT_FN(predict) if predict is not None else None
    check(L.orbl_level_breaks(C.c_float(log_scale_factor), int(nlevels), fn, ptr(out)))
    return out


def fuse_target(Rcw, tcw, Ow, K, bounds, grid, keys=None, desc=None, frame=None):
    """one target keyframe: the OrblFuseTarget record (bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), grid an OrbmGrid) with
    either its host arrays (mvKeysUn, descriptors) or a device-resident frame"""
    rec = np.zeros((), dtype=FUSE_TARGET_DTYPE)
    rec["Rcw"] = np.asarray(Rcw, dtype=np.float32).reshape(3, 3)
    rec["tcw"] = np.asarray(tcw, dtype=np.float32).reshape(3)
    rec["Ow"] = np.asarray(Ow, dtype=np.float32).reshape(3)
    rec["K"] = K4(K)
    rec["bounds"] = np.asarray(bounds, dtype=np.float32).reshape(4)
    if isinstance(grid, OrbmGrid):
        grid = (grid.minX, grid.minY, grid.invW, grid.invH, grid.cols, grid.rows)
    rec["grid"] = np.array(tuple(grid), dtype=GRID_DTYPE)
    t = dict(rec=rec)
    if frame is not None:
        t["frame"] = frame
    else:
        t["keys"] = np.ascontiguousarray(keys, dtype=KP_DTYPE)
        t["desc"] = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        if t["keys"].shape[0] != t["desc"].shape[0]:
            raise ValueError("keys and descriptors differ in length")
    return t


def fuse_points(pos, normal, min_distance, max_distance, desc):
    """the pool of map points: GetWorldPos, GetNormal, the RAW mfMinDistance / mfMaxDistance, GetDescriptor"""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    pts = np.zeros(pos.shape[0], dtype=FUSE_POINT_DTYPE)
    pts["pos"], pts["normal"] = pos, np.asarray(normal, dtype=np.float32).reshape(-1, 3)
    pts["min_distance"], pts["max_distance"] = min_distance, max_distance
    pts["desc"] = np.asarray(desc, dtype=np.uint8).reshape(-1, 32)
    return pts


def _fuse_levels(scale_factors, breaks, inv_level_sigma2=None):
    """the level tables of both Fuse entries as float32 rows, (sf, breaks, sigma2 or None), their lengths checked"""
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    br = np.ascontiguousarray(breaks, dtype=np.float32).reshape(-1)
    sg = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, dtype=np.float32).reshape(-1)
    if (sg is not None and sf.shape[0] != sg.shape[0]) or br.shape[0] != sf.shape[0] + 1:
        raise ValueError("%s and the break table disagree in length" % ("scale_factors" if sg is None else "scale_factors, inv_level_sigma2"))
    return sf, br, sg


class _Head(tuple):
    """the leading ctypes arguments of a Fuse entry, from the handle to the target count.  `keep` holds the arrays those
    pointers point into: they live exactly as long as the head does"""
    keep = ()


def _fuse_targets(matcher, targets):
    """what both Fuse entries take of fuse_target(...) dicts: (frames, head).  frames: the targets are device-resident frames
    (mixing them with host arrays raises); head: the leading arguments of the frames or the host-array entry (a _Head)"""
    T = len(targets)
    recs = np.zeros(max(T, 1), dtype=FUSE_TARGET_DTYPE)
    for k, t in enumerate(targets):
        recs[k] = t["rec"]
    frames = T > 0 and "frame" in targets[0]
    if any(("frame" in t) != frames for t in targets):
        raise ValueError("device-resident frames and host arrays cannot be mixed in one call")
    if frames:
        fr = (C.c_void_p * max(T, 1))(*[t["frame"].value if isinstance(t["frame"], C.c_void_p) else t["frame"] for t in targets])
        head = _Head((matcher._h, ptr(recs), fr, T))
        head.keep = (recs, fr)
    else:
        n = np.array([t["keys"].shape[0] for t in targets] or [0], dtype=np.int32)
        keys, desc = [t["keys"] for t in targets], [t["desc"] for t in targets]
        head = _Head((matcher._h, ptr(recs), _ptr_array(keys), _ptr_array(desc), ptr(n), T))
        head.keep = (recs, n, keys, desc)
    return frames, head


def fuse_batch(matcher, targets, points, jobs, scale_factors, inv_level_sigma2, breaks, th=3.0):
    """The searches of Fuse(pKF, vpMapPoints, th) for every target in one call.  targets: fuse_target(...) dicts, all with host
    arrays or all with frames; points: a FUSE_POINT_DTYPE pool; jobs: (job_start, job_point), CSR over the targets.  Returns
    a FUSE_RESULT_DTYPE array, one record per job entry in job order.  The caller applies bestDist <= TH_LOW and edits the map."""
    L = lib()
    T = len(targets)
    pts = np.ascontiguousarray(points, dtype=FUSE_POINT_DTYPE)
    js = np.ascontiguousarray(jobs[0], dtype=np.int32).reshape(-1)
    jp = np.ascontiguousarray(jobs[1], dtype=np.int32).reshape(-1)
    if js.shape[0] != T + 1:
        raise ValueError("job_start has %d entries for %d targets" % (js.shape[0], T))
    if T and jp.shape[0] < js[-1]:
        raise ValueError("job_point is shorter than job_start says")
    sf, br, sg = _fuse_levels(scale_factors, breaks, inv_level_sigma2)
    J = int(js[-1]) if T else 0
    out = np.zeros(max(J, 0), dtype=FUSE_RESULT_DTYPE)
    frames, head = _fuse_targets(matcher, targets)
    fn = L.orbl_fuse_batch_frames if frames else L.orbl_fuse_batch
    check(fn(*head, ptr(pts), pts.shape[0], ptr(js), ptr(jp), C.c_float(th), ptr(sf), ptr(sg), sf.shape[0], ptr(br), ptr(out)))
    return out
