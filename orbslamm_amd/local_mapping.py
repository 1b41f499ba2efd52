"""LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452, monocular) on the device, over the orbl_* block of
include/orbslamm_hip.h: one call searches the current keyframe against all its covisible neighbours,
triangulates every pair, applies the reference's gates and returns the new points in the reference's order.

    cur = dict(keys=mvKeysUn, desc=descriptors, fv=(node_id, start, idx), skip=has_map_point, kf=keyframe(...))
    nbs = [dict(keys=..., desc=..., fv=..., skip=..., kf=keyframe(..., median_depth=d)), ...]
    pts, status, f12 = create_new_map_points(matcher, cur, nbs, scale_factors, level_sigma2, 1.2)

With device-resident frames (ORBmatcher.frame_from_device + frame_compute_bow) a side is dict(frame=F, skip=..., kf=...)."""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, K4, OrbmFeatVec, check, lib, ptr

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


def _setup(L):
    if getattr(L, "_orbl_ready", False):
        return
    vp = C.c_void_p
    L.orbl_compute_f12.argtypes = [vp, vp, vp, vp]
    L.orbl_create_new_map_points.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float,
                                             C.c_int, vp, C.c_int, C.POINTER(C.c_int), vp, vp]
    L.orbl_create_new_map_points_frames.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int,
                                                    C.POINTER(C.c_int), vp, vp]
    L._orbl_ready = True


def compute_f12(kf1, kf2):
    """ComputeF12(pKF1, pKF2) and SearchForTriangulation's epipole in cv::Mat arithmetic (host; needs no GPU): F12 (3x3), (ex, ey)"""
    L = lib()
    _setup(L)
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
    _setup(L)
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
