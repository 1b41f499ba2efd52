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
from ._solver import Handle

MAX_CAPACITY = 1 << 22
FLAG_BAD, FLAG_OBSERVED = 1, 2
ST_BAD, ST_DEPTH, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_VIEW_ANGLE, ST_LEVEL_RANGE, ST_IN_VIEW, ST_NO_POINT = range(8)
POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("desc", "u1", 32),
                        ("flags", "u1"), ("pad", "u1", 3)])
VIEW_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("K", "<f4", 4), ("min_x", "<f4"), ("max_x", "<f4"),
                       ("min_y", "<f4"), ("max_y", "<f4"), ("viewing_cos_limit", "<f4")])
assert POINT_DTYPE.itemsize == 68 and VIEW_DTYPE.itemsize == 96


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


def _track_args(fs, view_rec, scale_factors, breaks, t_occ, mode, nnratio, check_ori, th_dist):
    """what the track_* calls marshal alike: (the view record, the scale factors, the break table or None, OrbmProjParams, t_occ
    padded to the frame set's cap or None)"""
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
    br = occ = None
    if breaks is not None:
        br = np.ascontiguousarray(breaks, dtype=np.float32)
        assert br.shape[0] == sf.shape[0] + 1
    if t_occ is not None:
        occ = np.zeros(fs.cap, np.uint8)
        occ[:len(t_occ)] = t_occ
    pp = OrbmProjParams(int(mode), float(nnratio), int(bool(check_ori)), int(th_dist))
    return np.ascontiguousarray(view_rec, dtype=VIEW_DTYPE), sf, br, pp, occ


class MapPool(Handle):
    """`capacity` MapPoint slots in HBM on the matcher's device (orbw_pool_*)."""
    _destroy = "orbw_pool_destroy"

    def __init__(self, matcher, capacity):
        self._L = lib()
        self._m = matcher
        self.capacity = int(capacity)
        self._h = C.c_void_p()
        check(self._L.orbw_pool_create(matcher._h, self.capacity, C.byref(self._h)))

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

    def debug_get(self, ids):
        """orbw_debug_pool_get: the pool's records of set ids, copied down (POINT_DTYPE)"""
        ids = _ids(ids)
        out = np.zeros(ids.shape[0], POINT_DTYPE)
        check(self._L.orbw_debug_pool_get(self._h, ptr(ids), ids.shape[0], ptr(out)))
        return out

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

    def track_local_map(self, fs, slot, view_rec, ids, th, scale_factors, breaks, t_occ=None, th_dist=100, nnratio=0.8, mode=3):
        """orbw_track_local_map: SearchLocalPoints' search against the frame in `slot` of frame set fs; asynchronous, the table
        comes back through fs.results() as one pair (assign[t] = position in ids), the status bytes through track_status"""
        ids = _ids(ids)
        v, sf, br, pp, occ = _track_args(fs, view_rec, scale_factors, breaks, t_occ, mode, nnratio, 0, th_dist)
        check(self._L.orbw_track_local_map(fs._h, int(slot), self._h, C.byref(pp), ptr(v), ptr(ids), ids.shape[0], C.c_float(th), ptr(sf), ptr(br),
                                           sf.shape[0], ptr(occ)))

    def track_frame_pose(self, fs, cur_slot, last_slot, view_rec, last_ids, th, scale_factors, t_occ=None, th_dist=100, nnratio=0.9,
                         check_ori=True, mode=4):
        """orbw_track_frame_pose: SearchByProjection(CurrentFrame, LastFrame) with CurrentFrame's pose; last_ids[i] = the pool id
        of LastFrame feature i's MapPoint or -1"""
        ids = _ids(last_ids)
        v, sf, _, pp, occ = _track_args(fs, view_rec, scale_factors, None, t_occ, mode, nnratio, check_ori, th_dist)
        check(self._L.orbw_track_frame_pose(fs._h, int(cur_slot), int(last_slot), self._h, C.byref(pp), ptr(v), ptr(ids), ids.shape[0],
                                            C.c_float(th), ptr(sf), ptr(occ)))

    def track_status(self, fs, back=0):
        """orbw_track_status after fs.results(back): a view of the search's status bytes in the set's pinned block"""
        st, n = C.c_void_p(), C.c_int(0)
        check(self._L.orbw_track_status(fs._h, int(back), C.byref(st), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_uint8)), shape=(n.value,))


# ---- Tracking::UpdateLocalMap from a keyframe store beside the pool (include/orbslamm_localmap.h)
ENTRY_NO_VOTE = 1 << 30
KF_BAD, KF_SET = 1, 2
MAX_NEIGHBOURS = 10
LOCAL_OK, LOCAL_NO_VOTES = 0, 1


class OrbuKeyFrames(C.Structure):
    _fields_ = [("nkf", C.c_int32), ("slot", C.c_void_p), ("flags", C.c_void_p), ("n", C.c_void_p), ("entries", C.c_void_p), ("neigh", C.c_void_p),
                ("parent", C.c_void_p), ("nchildren", C.c_void_p), ("children", C.c_void_p)]


class OrbuResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("kf_max", C.c_int32), ("nkf", C.c_int32), ("nL", C.c_int32), ("nS", C.c_int32), ("kf", C.c_void_p),
                ("L", C.c_void_p), ("seen", C.c_void_p), ("votes", C.c_void_p)]


# ---- KeyFrame::UpdateConnections and KeyFrameCulling's counts over the store (include/orbslamm_covis.h)
COVIS_OK, COVIS_EMPTY = 0, 1
MAX_OCTAVE_VALUES = 16


class OrbnConnections(C.Structure):
    _fields_ = [("K", C.c_int32), ("status", C.c_void_p), ("kf_max", C.c_void_p), ("n_max", C.c_void_p), ("cnt_start", C.c_void_p), ("cnt_kf", C.c_void_p),
                ("cnt_w", C.c_void_p), ("ord_start", C.c_void_p), ("ord_kf", C.c_void_p), ("ord_w", C.c_void_p)]


class OrbnCulling(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_mps", C.c_void_p), ("n_redundant", C.c_void_p), ("redundant", C.c_void_p)]


# ---- MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth over the store (include/orbslamm_refresh.h)
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
REFRESH_MAX_OBS = 1024
RST_NOT_ASKED, RST_DONE, RST_BAD, RST_NO_OBSERVATION, RST_ALL_KF_BAD, RST_NO_REF, RST_LEVEL_RANGE = range(7)
REFRESH_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("desc", "u1", 32),
                          ("n_obs", "<i4"), ("n_desc", "<i4"), ("best_kf", "<i4"), ("best_idx", "<i4"), ("st_descriptor", "u1"),
                          ("st_normal_depth", "u1"), ("pad", "u1", 2)])
assert REFRESH_DTYPE.itemsize == 84

# ---- the correction of LoopClosing::CorrectLoop / MultiMapper::UpdatePosesAndAdd over the store (include/orbslamm_correct.h)
CORRECT_KF_DTYPE = np.dtype([("corrected", "<f8", 8), ("non_corrected", "<f8", 8), ("Tiw", "<f4", 12), ("Ow", "<f4", 3), ("n_points", "<i4")])
CORRECT_POINT_DTYPE = np.dtype([("id", "<i4"), ("owner_slot", "<i4"), ("owner_idx", "<i4"), ("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"),
                                ("max_distance", "<f4"), ("n_obs", "<i4"), ("status", "u1"), ("pad", "u1", 3)])
assert CORRECT_KF_DTYPE.itemsize == 192 and CORRECT_POINT_DTYPE.itemsize == 52


def _copy(p, n, ct, dt):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)).astype(dt, copy=True) if p and n else np.zeros(0, dt)


class Connections:
    """orbn_update_connections' arrays, copied out of the store's blocks: status, kf_max, n_max per target; the counter rows
    (cnt_start, cnt_kf, cnt_w: mConnectedKeyFrameWeights, ascending kf) and the ordered rows (ord_start, ord_kf, ord_w:
    mvpOrderedConnectedKeyFrames / mvOrderedWeights) as CSR"""
    NAMES = ("status", "kf_max", "n_max", "cnt_start", "cnt_kf", "cnt_w", "ord_start", "ord_kf", "ord_w")

    def __init__(self, r):
        K = self.K = r.K
        i32 = lambda p, n: _copy(p, n, C.c_int32, np.int32)
        self.status, self.kf_max, self.n_max = i32(r.status, K), i32(r.kf_max, K), i32(r.n_max, K)
        self.cnt_start = i32(r.cnt_start, K + 1) if K else np.zeros(1, np.int32)
        self.ord_start = i32(r.ord_start, K + 1) if K else np.zeros(1, np.int32)
        self.cnt_kf, self.cnt_w = i32(r.cnt_kf, int(self.cnt_start[-1])), i32(r.cnt_w, int(self.cnt_start[-1]))
        self.ord_kf, self.ord_w = i32(r.ord_kf, int(self.ord_start[-1])), i32(r.ord_w, int(self.ord_start[-1]))

    def counter(self, t):
        a, b = self.cnt_start[t], self.cnt_start[t + 1]
        return self.cnt_kf[a:b], self.cnt_w[a:b]

    def ordered(self, t):
        a, b = self.ord_start[t], self.ord_start[t + 1]
        return self.ord_kf[a:b], self.ord_w[a:b]


class Culling:
    """orbn_culling_counts' arrays, copied out: n_mps, n_redundant, redundant per target"""
    NAMES = ("n_mps", "n_redundant", "redundant")

    def __init__(self, r):
        self.K = r.K
        self.n_mps, self.n_redundant = _copy(r.n_mps, r.K, C.c_int32, np.int32), _copy(r.n_redundant, r.K, C.c_int32, np.int32)
        self.redundant = _copy(r.redundant, r.K, C.c_uint8, np.uint8)


def _concat(lists):
    lists = [_ids(a) for a in lists]
    n = np.array([a.shape[0] for a in lists], np.int32)
    flat = np.concatenate(lists).astype(np.int32) if len(lists) and n.sum() else np.zeros(0, np.int32)
    return n, np.ascontiguousarray(flat)


class LocalMap:
    """what orbu_update_local_map / orbu_local_points left in the store's pinned block: status, kf_max, nkf, nL, nS, and the arrays
    kf (the local keyframes), L (mvpLocalMapPoints), seen, S (= L[seen == 0], derived on the host; KeyFrameStore.resident_list() is the device's own)
    and votes (per slot, update only; else None).  An array is copied out of the block when it is first read: read it before the
    store's next call"""

    def __init__(self, r, kf_capacity, store=None):
        self._store = store
        self.status, self.kf_max, self.nkf, self.nL, self.nS = r.status, r.kf_max, r.nkf, r.nL, r.nS
        self._r, self._kfcap, self._got = r, kf_capacity, {}

    def _arr(self, name, p, n, ct, dt):
        if name not in self._got:
            self._got[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)).astype(dt, copy=True) if p and n else np.zeros(0, dt)
        return self._got[name]

    kf = property(lambda self: self._arr("kf", self._r.kf, self.nkf, C.c_int32, np.int32))
    L = property(lambda self: self._arr("L", self._r.L, self.nL, C.c_int32, np.int32))
    seen = property(lambda self: self._arr("seen", self._r.seen, self.nL, C.c_uint8, np.uint8))
    S = property(lambda self: self.L[self.seen == 0])
    resident = property(lambda self: self._store.resident_list())   # the device's own S (a copy down: for tests)
    votes = property(lambda self: self._arr("votes", self._r.votes, self._kfcap, C.c_int32, np.int32) if self._r.votes else None)


class KeyFrameStore(Handle):
    """`kf_capacity` keyframes (match lists of `stride` pool ids, flags, covisibility / spanning-tree records) in HBM beside
    a MapPool (orbu_*)."""
    _destroy = "orbu_store_destroy"

    def __init__(self, pool, kf_capacity, stride, max_children, max_local_points):
        self._L = lib()
        self._pool = pool
        self.kf_capacity, self.stride, self.max_children, self.max_local_points = int(kf_capacity), int(stride), int(max_children), int(max_local_points)
        self._h = C.c_void_p()
        check(self._L.orbu_store_create(pool._h, self.kf_capacity, self.stride, self.max_children, self.max_local_points, C.byref(self._h)))

    def _records(self, slots, flags, entries, neigh, parent, children):
        slots = _ids(slots)
        nkf = slots.shape[0]
        keep = [slots]
        rec = OrbuKeyFrames(nkf=nkf, slot=ptr(slots))
        if flags is not None:
            fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
            n, ent = _concat(entries)
            assert fl.shape[0] == nkf and n.shape[0] == nkf
            rec.flags, rec.n, rec.entries = ptr(fl), ptr(n), ptr(ent)
            keep += [fl, n, ent]
        ng = np.full((nkf, MAX_NEIGHBOURS), -1, np.int32)
        for i, row in enumerate(neigh):
            row = _ids(row)
            assert row.shape[0] <= MAX_NEIGHBOURS
            ng[i, :row.shape[0]] = row
        par = _ids(parent)
        nc, ch = _concat(children)
        assert par.shape[0] == nkf and nc.shape[0] == nkf
        rec.neigh, rec.parent, rec.nchildren, rec.children = ptr(ng), ptr(par), ptr(nc), ptr(ch)
        keep += [ng, par, nc, ch]
        return rec, keep

    def set(self, slots, flags, entries, neigh, parent, children):
        """orbu_kf_set: whole records.  entries[i]: keyframe i's GetMapPointMatches() as pool ids (-1 empty, | ENTRY_NO_VOTE);
        neigh[i]: up to 10 slots; parent[i]: slot or -1; children[i]: slots"""
        rec, keep = self._records(slots, flags, entries, neigh, parent, children)
        check(self._L.orbu_kf_set(self._h, C.byref(rec)))

    def set_graph(self, slots, neigh, parent, children):
        rec, keep = self._records(slots, None, None, neigh, parent, children)
        check(self._L.orbu_kf_set_graph(self._h, C.byref(rec)))

    def set_flags(self, slots, flags):
        slots = _ids(slots)
        fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        assert fl.shape[0] == slots.shape[0]
        check(self._L.orbu_kf_set_flags(self._h, ptr(slots), ptr(fl), slots.shape[0]))

    def set_entries(self, slot, idx, vals):
        idx, vals = _ids(idx), _ids(vals)
        assert idx.shape[0] == vals.shape[0]
        check(self._L.orbu_kf_set_entries(self._h, int(slot), ptr(idx), ptr(vals), idx.shape[0]))

    def set_octaves(self, slot, octaves):
        """orbu_kf_set_octaves: mvKeysUn[i].octave of a set keyframe, one byte per feature"""
        o = np.ascontiguousarray(octaves, dtype=np.uint8).reshape(-1)
        check(self._L.orbu_kf_set_octaves(self._h, int(slot), ptr(o), o.shape[0]))

    def set_descriptors(self, slot, desc):
        """orbu_kf_set_descriptors: mDescriptors of a set keyframe, n x 32 bytes"""
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        check(self._L.orbu_kf_set_descriptors(self._h, int(slot), ptr(d), d.shape[0]))

    def set_descriptors_frame(self, slot, fs, fs_slot):
        """orbu_kf_set_descriptors_frame: the descriptors of slot fs_slot of a frame set, device to device"""
        check(self._L.orbu_kf_set_descriptors_frame(self._h, int(slot), fs._h, int(fs_slot)))

    def set_centres(self, slots, Ow):
        """orbu_kf_set_centres: GetCameraCenter() of set keyframes, three floats each; a repeated slot takes the last"""
        slots = _ids(slots)
        c = np.ascontiguousarray(Ow, dtype=np.float32).reshape(-1, 3)
        assert c.shape[0] == slots.shape[0]
        check(self._L.orbu_kf_set_centres(self._h, ptr(slots), ptr(c), slots.shape[0]))

    def refresh_points(self, ids, ref_kf, scale_factors, what=REFRESH_DESCRIPTOR | REFRESH_NORMAL_DEPTH, new_pos=None, commit=True):
        """orbr_refresh_points: ComputeDistinctiveDescriptors and / or UpdateNormalAndDepth of the listed pool ids, written into the
        pool when commit -> a REFRESH_DTYPE array, one record per id"""
        ids, ref = _ids(ids), _ids(ref_kf)
        assert ref.shape[0] == ids.shape[0]
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        pos = None
        if new_pos is not None:
            pos = np.ascontiguousarray(new_pos, dtype=np.float32).reshape(-1, 3)
            assert pos.shape[0] == ids.shape[0]
        out = np.zeros(ids.shape[0], REFRESH_DTYPE)
        check(self._L.orbr_refresh_points(self._h, ptr(ids), ptr(ref), ptr(pos), ids.shape[0], int(what), ptr(sf), sf.shape[0], int(bool(commit)), ptr(out)))
        return out

    def set_ref_kf(self, ids, kf_slots):
        """orbu_point_set_ref_kf: mpRefKF of pool ids as store slots (-1: none), resident beside the pool; a repeated id takes the last"""
        ids, kf = _ids(ids), _ids(kf_slots)
        assert kf.shape[0] == ids.shape[0]
        check(self._L.orbu_point_set_ref_kf(self._h, ptr(ids), ptr(kf), ids.shape[0]))

    def correct_sim3(self, slots, Tiw, anchor, Scw, scale_factors, skip_ids=(), commit=True, pts_cap=None):
        """orbe_correct_sim3: the loop Sim3 `Scw` (q x y z w, t, s) propagated over the keyframes `slots` whose poses are Tiw (rows
        [R | t], or 4x4), slots[anchor] being the current keyframe; every point they hold moved once, its normal and depth
        refreshed; written into the pool and the store's centres when commit -> (CORRECT_KF_DTYPE[K] in the caller's order,
        CORRECT_POINT_DTYPE[n] in the reference's visiting order).  pts_cap: room for the moved points (default: the most there can be)"""
        slots, skip = _ids(slots), _ids(skip_ids)
        K = slots.shape[0]
        T = np.asarray(Tiw, dtype=np.float32)
        T = np.ascontiguousarray(T.reshape(K, 4, 4)[:, :3, :] if T.size == 16 * K and K else T.reshape(K, 12))
        S = np.ascontiguousarray(Scw, dtype=np.float64).reshape(8)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        cap = min(self._pool.capacity, K * self.stride) if pts_cap is None else int(pts_cap)
        kf, pts, n = np.zeros(K, CORRECT_KF_DTYPE), np.zeros(cap, CORRECT_POINT_DTYPE), C.c_int(0)
        check(self._L.orbe_correct_sim3(self._h, ptr(slots), ptr(T), K, int(anchor), ptr(S), ptr(skip), skip.shape[0], ptr(sf), sf.shape[0], int(bool(commit)),
                                        ptr(kf), ptr(pts), cap, C.byref(n)))
        return kf, pts[:n.value].copy()

    def update_connections(self, targets, th=15):
        """orbn_update_connections: KeyFrame::UpdateConnections' counter and ordered list of every target -> Connections"""
        tg = _ids(targets)
        r = OrbnConnections()
        check(self._L.orbn_update_connections(self._h, ptr(tg), tg.shape[0], int(th), C.byref(r)))
        return Connections(r)

    def culling_counts(self, targets, th_obs=3):
        """orbn_culling_counts: KeyFrameCulling's nMPs, nRedundantObservations and verdict of every target -> Culling"""
        tg = _ids(targets)
        r = OrbnCulling()
        check(self._L.orbn_culling_counts(self._h, ptr(tg), tg.shape[0], int(th_obs), C.byref(r)))
        return Culling(r)

    def update(self, frame_ids, max_keyframes=80):
        """orbu_update_local_map -> LocalMap (status LOCAL_NO_VOTES: nothing else is meaningful)"""
        ids = _ids(frame_ids)
        r = OrbuResult()
        check(self._L.orbu_update_local_map(self._h, ptr(ids), ids.shape[0], int(max_keyframes), C.byref(r)))
        return LocalMap(r, self.kf_capacity, self)

    def local_points(self, kf_list, frame_ids):
        """orbu_local_points: UpdateLocalPoints alone over the caller's keyframe list"""
        kf, ids = _ids(kf_list), _ids(frame_ids)
        r = OrbuResult()
        check(self._L.orbu_local_points(self._h, ptr(kf), kf.shape[0], ptr(ids), ids.shape[0], C.byref(r)))
        return LocalMap(r, self.kf_capacity, self)

    def debug_set_generation(self, generation):
        check(self._L.orbu_debug_set_generation(self._h, C.c_uint32(int(generation))))

    def resident_list(self):
        """orbu_debug_resident_list: the S of the last completed update as it lies on the device"""
        out, n = np.zeros(self.max_local_points, np.int32), C.c_int(0)
        check(self._L.orbu_debug_resident_list(self._h, ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    def track_local_map(self, fs, slot, view_rec, th, scale_factors, breaks, t_occ=None, th_dist=100, nnratio=0.8, mode=3):
        """orbw_track_local_map_resident: MapPool.track_local_map with ids = the S of this store's last update, read where it
        lies; assign[t] = position in S"""
        v, sf, br, pp, occ = _track_args(fs, view_rec, scale_factors, breaks, t_occ, mode, nnratio, 0, th_dist)
        check(self._L.orbw_track_local_map_resident(fs._h, int(slot), self._pool._h, self._h, C.byref(pp), ptr(v), C.c_float(th), ptr(sf), ptr(br),
                                                    sf.shape[0], ptr(occ)))
