"""ctypes mirror of the map-point pool (include/orbslamm_mappool.h): MapPoints resident in HBM under ids the
caller chooses, and Tracking's two projection searches run from a pose and a list of ids.

    pool = MapPool(matcher, capacity)
    pool.set(ids, map_points(pos, normal, min_d, max_d, desc, flags))     # when LocalMapping touches the points
    pool.track_local_map(fs, slot, view(Rcw, tcw, Ow, K, bounds), ids, 1.0, scale_factors, level_breaks(log_sf, 8))
    assign, nm = fs.results(); status = pool.track_status(fs)

The host replay of Tracking::SearchLocalPoints (IncreaseVisible, mnLastFrameSeen, F.mvpMapPoints) stays the caller's
(include/Tracking_hip.hpp does it in the reference's order)."""
import ctypes as C

import numpy as np

from ._lib import K4, OrbmProjParams, check, lib, ptr

MAX_CAPACITY = 1 << 22
FLAG_BAD, FLAG_OBSERVED = 1, 2
ST_BAD, ST_DEPTH, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_VIEW_ANGLE, ST_LEVEL_RANGE, ST_IN_VIEW, ST_NO_POINT = range(8)
POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("desc", "u1", 32),
                        ("flags", "u1"), ("pad", "u1", 3)])
VIEW_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("K", "<f4", 4), ("min_x", "<f4"), ("max_x", "<f4"),
                       ("min_y", "<f4"), ("max_y", "<f4"), ("viewing_cos_limit", "<f4")])
assert POINT_DTYPE.itemsize == 68 and VIEW_DTYPE.itemsize == 96


def _setup(L):
    if getattr(L, "_orbw_ready", False):
        return
    vp = C.c_void_p
    L.orbw_pool_create.argtypes = [vp, C.c_int, vp]
    L.orbw_pool_destroy.argtypes = [vp]
    L.orbw_pool_set.argtypes = [vp, vp, vp, C.c_int]
    L.orbw_pool_set_flags.argtypes = [vp, vp, vp, C.c_int]
    L.orbw_view_project.argtypes = [vp, vp, vp, vp, C.c_int, C.c_float, vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbw_view_project_frame.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, vp, vp, vp, vp]
    L.orbw_track_local_map.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, vp, vp, C.c_int, vp]
    L.orbw_track_frame_pose.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, vp, vp]
    L.orbw_track_status.argtypes = [vp, C.c_int, vp, vp]
    L._orbw_ready = True


def map_points(pos, normal, min_distance, max_distance, desc, flags):
    """n OrbwPoint records: GetWorldPos, GetNormal, the RAW mfMinDistance / mfMaxDistance, GetDescriptor, flags (FLAG_BAD |
    FLAG_OBSERVED)"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    out = np.zeros(pos.shape[0], POINT_DTYPE)
    out["pos"] = pos
    out["normal"] = np.asarray(normal, np.float32).reshape(-1, 3)
    out["min_distance"] = min_distance
    out["max_distance"] = max_distance
    out["desc"] = np.asarray(desc, np.uint8).reshape(-1, 32)
    out["flags"] = flags
    return out


def view(Rcw, tcw, Ow, K, bounds, viewing_cos_limit=0.5):
    """the OrbwView record: mRcw, mtcw, mOw as the caller's Frame holds them, K (fx, fy, cx, cy or 3x3), bounds = (mnMinX,
    mnMaxX, mnMinY, mnMaxY), isInFrustum's viewingCosLimit"""
    v = np.zeros(1, VIEW_DTYPE)
    v["Rcw"] = np.asarray(Rcw, np.float32).reshape(9)
    v["tcw"] = np.asarray(tcw, np.float32).reshape(3)
    v["Ow"] = np.asarray(Ow, np.float32).reshape(3)
    v["K"] = K4(K)
    v["min_x"], v["max_x"], v["min_y"], v["max_y"] = [np.float32(b) for b in bounds]
    v["viewing_cos_limit"] = np.float32(viewing_cos_limit)
    return v


def _ids(ids):
    return np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)


class MapPool:
    """`capacity` MapPoint slots in HBM on the matcher's device (orbw_pool_*)."""

    def __init__(self, matcher, capacity):
        self._L = lib()
        _setup(self._L)
        self._m = matcher
        self.capacity = int(capacity)
        self._h = C.c_void_p()
        check(self._L.orbw_pool_create(matcher._h, self.capacity, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbw_pool_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, ids, points):
        """orbw_pool_set: returns with the records in HBM; a repeated id takes the last record"""
        ids = _ids(ids)
        pts = np.ascontiguousarray(points, dtype=POINT_DTYPE)
        assert pts.shape[0] == ids.shape[0]
        check(self._L.orbw_pool_set(self._h, ptr(ids), ptr(pts), ids.shape[0]))

    def set_flags(self, ids, flags):
        ids = _ids(ids)
        fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        assert fl.shape[0] == ids.shape[0]
        check(self._L.orbw_pool_set_flags(self._h, ptr(ids), ptr(fl), ids.shape[0]))

    def view_project(self, view_rec, ids, th, scale_factors, breaks, last=None):
        """orbw_view_project: the projection kernel alone -> (uvr[nq, 3], lvl[nq, 2], viewcos[nq], status[nq]).
        last = (frame_set, slot): the frame/frame gate set (orbw_view_project_frame; breaks unused, viewcos zeros)"""
        ids = _ids(ids)
        nq = ids.shape[0]
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        v = np.ascontiguousarray(view_rec, dtype=VIEW_DTYPE)
        uvr, lvl = np.zeros((nq, 3), np.float32), np.zeros((nq, 2), np.int8)
        cos, st = np.zeros(nq, np.float32), np.zeros(nq, np.uint8)
        if last is not None:
            fs, slot = last
            check(self._L.orbw_view_project_frame(fs._h, int(slot), self._h, ptr(v), ptr(ids), nq, C.c_float(th), ptr(sf), ptr(uvr), ptr(lvl), ptr(st)))
        else:
            br = np.ascontiguousarray(breaks, dtype=np.float32)
            assert br.shape[0] == sf.shape[0] + 1
            check(self._L.orbw_view_project(self._m._h, self._h, ptr(v), ptr(ids), nq, C.c_float(th), ptr(sf), ptr(br), sf.shape[0],
                                            ptr(uvr), ptr(lvl), ptr(cos), ptr(st)))
        return uvr, lvl, cos, st

    @staticmethod
    def _occ(fs, t_occ):
        if t_occ is None:
            return None
        occ = np.zeros(fs.cap, np.uint8)
        occ[:len(t_occ)] = t_occ
        return occ

    def track_local_map(self, fs, slot, view_rec, ids, th, scale_factors, breaks, t_occ=None, th_dist=100, nnratio=0.8, mode=3):
        """orbw_track_local_map: SearchLocalPoints' search against the frame in `slot` of frame set fs; asynchronous, the table
        comes back through fs.results() as one pair (assign[t] = position in ids), the status bytes through track_status"""
        ids = _ids(ids)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        br = np.ascontiguousarray(breaks, dtype=np.float32)
        assert br.shape[0] == sf.shape[0] + 1
        v = np.ascontiguousarray(view_rec, dtype=VIEW_DTYPE)
        pp = OrbmProjParams(int(mode), float(nnratio), 0, int(th_dist))
        occ = self._occ(fs, t_occ)
        check(self._L.orbw_track_local_map(fs._h, int(slot), self._h, C.byref(pp), ptr(v), ptr(ids), ids.shape[0], C.c_float(th), ptr(sf), ptr(br),
                                           sf.shape[0], ptr(occ)))

    def track_frame_pose(self, fs, cur_slot, last_slot, view_rec, last_ids, th, scale_factors, t_occ=None, th_dist=100, nnratio=0.9,
                         check_ori=True, mode=4):
        """orbw_track_frame_pose: SearchByProjection(CurrentFrame, LastFrame) with CurrentFrame's pose; last_ids[i] = the pool id
        of LastFrame feature i's MapPoint or -1"""
        ids = _ids(last_ids)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        v = np.ascontiguousarray(view_rec, dtype=VIEW_DTYPE)
        pp = OrbmProjParams(int(mode), float(nnratio), int(bool(check_ori)), int(th_dist))
        occ = self._occ(fs, t_occ)
        check(self._L.orbw_track_frame_pose(fs._h, int(cur_slot), int(last_slot), self._h, C.byref(pp), ptr(v), ptr(ids), ids.shape[0],
                                            C.c_float(th), ptr(sf), ptr(occ)))

    def track_status(self, fs, back=0):
        """orbw_track_status after fs.results(back): a view of the search's status bytes in the set's pinned block"""
        st, n = C.c_void_p(), C.c_int(0)
        check(self._L.orbw_track_status(fs._h, int(back), C.byref(st), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_uint8)), shape=(n.value,))
