"""Scenes for the map-point pool's projections: a camera pose, a pool of MapPoint records and an id list per
scene family, the restatement's answers (tools/frustum_ref.hpp through tests/cpp/frustum_ref_capi.cpp) and a float64 numpy
model of the same geometry written here.  Shared by tests/test_localmap_cpu.py and tests/test_gpu_localmap.py."""
import ctypes as C
import functools

import numpy as np

from ref_shim import cached_shim, p, rot_axis_angle as _rot

rot_axis_angle = functools.partial(_rot, scale_first=True)   # (how this module's scenes were generated: ref_shim.rot_axis_angle)

f32 = np.float32
W, H = 640, 480
K_A = np.array([517.3, 516.5, 318.6, 255.3], dtype=f32)
K_EXACT = np.array([512.0, 512.0, 320.0, 240.0], dtype=f32)     # u = fx*X + cx is exact at z = 1: points land ON a bound
BOUNDS = (0.0, float(W), 0.0, float(H))
NLEVELS = 8
SCALE_FACTOR = f32(1.2)
LOG_SF = f32(np.log(SCALE_FACTOR))                              # mfLogScaleFactor = log(mfScaleFactor), a float
SF = np.ones(NLEVELS, f32)
for _l in range(1, NLEVELS):
    SF[_l] = SF[_l - 1] * SCALE_FACTOR                          # ORBextractor.cc: mvScaleFactor[i] = mvScaleFactor[i-1]*scaleFactor
SF_B = np.ones(NLEVELS, f32)                                    # a second level table (scale factor 1.3)
for _l in range(1, NLEVELS):
    SF_B[_l] = SF_B[_l - 1] * f32(1.3)
LOG_SF_B = f32(np.log(f32(1.3)))
(ST_BAD, ST_DEPTH, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_VIEW_ANGLE, ST_LEVEL_RANGE, ST_IN_VIEW, ST_NO_POINT) = range(8)
FLAG_BAD, FLAG_OBSERVED = 1, 2
POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("desc", "u1", 32),
                        ("flags", "u1"), ("pad", "u1", 3)])
VIEW_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("K", "<f4", 4), ("min_x", "<f4"), ("max_x", "<f4"),
                       ("min_y", "<f4"), ("max_y", "<f4"), ("viewing_cos_limit", "<f4")])
MARGIN = 1e-3
SEEDS = range(1, 11)

def _declare(L):
    vp = C.c_void_p
    L.frustum_local.argtypes = [vp, vp, vp, C.c_int, C.c_float, vp, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp]
    L.frustum_frame.argtypes = [vp, vp, vp, vp, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp]
    L.frustum_local.restype = None
    L.frustum_frame.restype = None


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("frustum_ref", _declare)


def ref_local(view, points, ids, th, sf=SF, log_sf=LOG_SF):
    """the restatement over a local-map list: dict(uvr, lvl, viewcos, valid, obs, status)"""
    ids = np.ascontiguousarray(ids, np.int32)
    n = ids.shape[0]
    out = dict(uvr=np.zeros((n, 3), f32), lvl=np.zeros((n, 2), np.int8), viewcos=np.zeros(n, f32), valid=np.zeros(n, np.uint8),
               obs=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8))
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    sf = np.ascontiguousarray(sf, f32)
    ref_lib().frustum_local(p(view), p(pts), p(ids), n, C.c_float(th), p(sf), sf.shape[0], C.c_float(log_sf), p(out["uvr"]), p(out["lvl"]),
                            p(out["viewcos"]), p(out["valid"]), p(out["obs"]), p(out["status"]))
    return out


def ref_frame(view, points, last_ids, octaves, th, sf=SF):
    ids = np.ascontiguousarray(last_ids, np.int32)
    octs = np.ascontiguousarray(octaves, np.int32)
    n = ids.shape[0]
    out = dict(uvr=np.zeros((n, 3), f32), lvl=np.zeros((n, 2), np.int8), viewcos=np.zeros(n, f32), valid=np.zeros(n, np.uint8),
               obs=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8))
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    sf = np.ascontiguousarray(sf, f32)
    ref_lib().frustum_frame(p(view), p(pts), p(ids), p(octs), n, C.c_float(th), p(sf), p(out["uvr"]), p(out["lvl"]), p(out["valid"]), p(out["obs"]),
                            p(out["status"]))
    return out


def make_view(R=None, t=None, K=K_A, bounds=BOUNDS, cos_limit=0.5):
    """the OrbwView record of a camera with rotation R (world -> camera) and translation t; Ow = -R^T t as the frame holds it"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    v = np.zeros(1, VIEW_DTYPE)
    R32, t32 = R.astype(f32), t.astype(f32)
    v["Rcw"] = R32.reshape(9)
    v["tcw"] = t32
    v["Ow"] = (-(R32.astype(np.float64).T @ t32.astype(np.float64))).astype(f32)
    v["K"] = K
    v["min_x"], v["max_x"], v["min_y"], v["max_y"] = [f32(b) for b in bounds]
    v["viewing_cos_limit"] = f32(cos_limit)
    return v


def camera_of(view):
    v = view[0]
    return v["Rcw"].reshape(3, 3).astype(np.float64), v["tcw"].astype(np.float64), v["Ow"].astype(np.float64)


def scene_points(rng, view, n, behind=0.05, outside=0.2, cos_range=(0.3, 1.0), sf=SF):
    """n MapPoint records seen from `view`: depths 1 .. 20, pixels over a window wider than the image by `outside`, a share
    behind the camera; each point's reference centre is drawn so that viewCos spreads over cos_range, at a distance of 0.4 .. 2.5
    times the view's own (every distance and level outcome occurs); random descriptors; 10 % bad, 80 % observed"""
    R, t, Ow = camera_of(view)
    K = view[0]["K"].astype(np.float64)
    z = rng.uniform(1.0, 20.0, n)
    z[rng.random(n) < behind] *= -1
    u = rng.uniform(-outside * W, (1 + outside) * W, n)
    v = rng.uniform(-outside * H, (1 + outside) * H, n)
    Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    Xw = (Xc - t) @ R          # R^T (Xc - t), row-wise
    pts = np.zeros(n, POINT_DTYPE)
    pts["pos"] = Xw.astype(f32)
    d = Xw - Ow
    dist = np.linalg.norm(d, axis=1)
    dirv = d / dist[:, None]
    # the normal: the view direction turned by acos(c), c uniform over cos_range, about a random axis orthogonal to it
    c = rng.uniform(cos_range[0], cos_range[1], n)
    rnd = rng.normal(size=(n, 3))
    orth = rnd - (rnd * dirv).sum(1)[:, None] * dirv
    orth /= np.linalg.norm(orth, axis=1)[:, None]
    normal = c[:, None] * dirv + np.sqrt(1 - c * c)[:, None] * orth
    pts["normal"] = normal.astype(f32)
    level = rng.integers(0, len(sf), n)
    dref = dist * np.exp(rng.uniform(np.log(0.4), np.log(2.5), n))
    maxd = dref * sf[level].astype(np.float64)                   # MapPoint::UpdateNormalAndDepth: dist * levelScaleFactor
    pts["max_distance"] = maxd.astype(f32)
    pts["min_distance"] = (pts["max_distance"] / sf[-1]).astype(f32)
    pts["desc"] = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    fl = np.where(rng.random(n) < 0.8, FLAG_OBSERVED, 0) | np.where(rng.random(n) < 0.1, FLAG_BAD, 0)
    pts["flags"] = fl.astype(np.uint8)
    return pts


def pan_view(seed):
    rng = np.random.default_rng(1000 + seed)
    R = rot_axis_angle([0.1, 1.0, 0.05], rng.uniform(-0.6, 0.6))
    return make_view(R, rng.uniform(-0.3, 0.3, 3))


def translation_view(seed):
    rng = np.random.default_rng(2000 + seed)
    R = rot_axis_angle(rng.normal(size=3), rng.uniform(0, 0.05))
    return make_view(R, rng.uniform(-3.0, 3.0, 3))


def _search_scale(target, factor, want):
    """a float m near target / factor with want(factor * m) (float products), or None"""
    m = f32(target / np.float64(factor))
    for _ in range(8):
        m = np.nextafter(m, f32(0))
    for _ in range(17):
        if want(f32(factor) * m):
            return m
        m = np.nextafter(m, f32(np.inf))
    return None


def family_scene(name, seed=1, n=600):
    """(view, points) of a family; its id list is arange(n) unless the caller draws another"""
    rng = np.random.default_rng(sum(map(ord, name)) * 100 + seed)
    if name == "pan":
        view = pan_view(seed)
        return view, scene_points(rng, view, n)
    if name == "translation":
        view = translation_view(seed)
        return view, scene_points(rng, view, n)
    if name == "behind":
        view = pan_view(seed)
        return view, scene_points(rng, view, n, behind=0.6)
    if name == "bad_flags":
        view = pan_view(seed)
        pts = scene_points(rng, view, n)
        pts["flags"] |= np.where(rng.random(n) < 0.5, FLAG_BAD, 0).astype(np.uint8)
        return view, pts
    if name == "nan_position":
        view = pan_view(seed)
        pts = scene_points(rng, view, n)
        for k in range(0, n, 7):
            pts["pos"][k, k % 3] = np.nan
        return view, pts
    if name == "pcz_zero":
        # identity pose: Pc = P exactly.  PcZ = +0 and -0, with PcX == 0 (u is NaN) and without (u is +-inf)
        view = make_view()
        pts = scene_points(rng, view, n)
        for k in range(0, n, 5):
            pts["pos"][k] = [(0.0, 1.0, -1.0)[(k // 5) % 3], (0.0, 0.5)[(k // 15) % 2], (0.0, -0.0)[(k // 30) % 2]]
        return view, pts
    if name == "on_bounds":
        # identity pose, K_EXACT, z = 1: u = 512*X + 320 is exact, so X = -0.625 / 0.625 put u ON 0 / 640 (inclusive: in the
        # image), and the next float outside is outside; the same for v with 240
        view = make_view(K=K_EXACT)
        pts = scene_points(rng, view, n, behind=0.0, outside=0.0)
        edge = [(-0.625, None), (0.625, None), (None, -0.46875), (None, 0.46875)]
        for k in range(0, n, 3):
            ex, ey = edge[(k // 3) % 4]
            outward = (k // 12) % 3          # 0: on the bound, 1: the next float outside, 2: the next float inside
            xy = [f32(rng.uniform(-0.5, 0.5)), f32(rng.uniform(-0.4, 0.4))]
            for a, e in enumerate((ex, ey)):
                if e is None:
                    continue
                x = f32(e)
                if outward == 1:
                    x = np.nextafter(x, f32(np.sign(e) * 10))
                elif outward == 2:
                    x = np.nextafter(x, f32(0))
                xy[a] = x
            pts["pos"][k] = [xy[0], xy[1], 1.0]
            _realistic_bounds(pts, k, view)
        return view, pts
    if name == "on_distance_gates":
        view = pan_view(seed)
        pts = scene_points(rng, view, n, behind=0.0, outside=0.0)
        _, _, Ow = camera_of(view)
        for k in range(0, n, 2):
            PO = pts["pos"][k] - view[0]["Ow"]
            dist = f32(np.sqrt((PO.astype(np.float64) ** 2).sum()))
            which = (k // 2) % 4
            if which == 0:      # dist == 1.2f*max exactly: inside
                m = _search_scale(dist, 1.2, lambda x: x == dist)
                if m is not None:
                    pts["max_distance"][k] = m
                    pts["min_distance"][k] = m / SF[-1]
            elif which == 1:    # the largest max with 1.2f*max < dist: outside
                m = _search_scale(dist, 1.2, lambda x: x >= dist)
                if m is not None:
                    m = np.nextafter(m, f32(0))
                    pts["max_distance"][k] = m
                    pts["min_distance"][k] = m / SF[-1]
            elif which == 2:    # dist == 0.8f*min exactly: inside
                m = _search_scale(dist, 0.8, lambda x: x == dist)
                if m is not None:
                    pts["min_distance"][k] = m
                    pts["max_distance"][k] = m * SF[-1]
            else:               # the smallest min with 0.8f*min > dist: outside
                m = _search_scale(dist, 0.8, lambda x: x > dist)
                if m is not None:
                    pts["min_distance"][k] = m
                    pts["max_distance"][k] = m * SF[-1]
        return view, pts
    if name == "viewcos_edges":
        # normals whose angle to the view direction puts viewCos within 1e-6 .. 1e-3 of 0.5 and of 0.998, on both sides
        view = pan_view(seed)
        pts = scene_points(rng, view, n, behind=0.0, outside=0.0)
        _, _, Ow = camera_of(view)
        d = pts["pos"].astype(np.float64) - Ow
        dirv = d / np.linalg.norm(d, axis=1)[:, None]
        c = np.where(np.arange(n) % 2 == 0, 0.5, 0.998) + rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-7, -3, n)
        rnd = rng.normal(size=(n, 3))
        orth = rnd - (rnd * dirv).sum(1)[:, None] * dirv
        orth /= np.linalg.norm(orth, axis=1)[:, None]
        pts["normal"] = (c[:, None] * dirv + np.sqrt(1 - c * c)[:, None] * orth).astype(f32)
        return view, pts
    if name == "level_edges":
        # max distances that put PredictScale at -1 (dist just inside 1.2 max: ratio at 1/1.2) and at nlevels and above (dist
        # below min), and ratios next to every level's break
        view = pan_view(seed)
        pts = scene_points(rng, view, n, behind=0.0, outside=0.0)
        for k in range(n):
            PO = pts["pos"][k] - view[0]["Ow"]
            dist = f32(np.sqrt((PO.astype(np.float64) ** 2).sum()))
            which = k % 4
            if which == 0:
                m = _search_scale(dist, 1.2, lambda x: x >= dist)      # 1.2f*max >= dist by the least margin: ratio ~ 1/1.2
                if m is not None:
                    pts["max_distance"][k] = m
                    pts["min_distance"][k] = m / SF[-1]
            elif which == 1:
                mn = f32(dist * rng.uniform(1.02, 1.24))                # 0.8 min < dist < min: levels nlevels, nlevels + 1
                pts["min_distance"][k] = mn
                pts["max_distance"][k] = mn * SF[-1]
            elif which == 2:
                lvl = rng.integers(0, NLEVELS)
                ratio = np.float64(SCALE_FACTOR) ** lvl * (1 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-7, -4))
                pts["max_distance"][k] = f32(dist * ratio)
                pts["min_distance"][k] = pts["max_distance"][k] / SF[-1]
        return view, pts
    raise KeyError(name)


def _realistic_bounds(pts, k, view):
    """distance bounds and a normal under which point k passes every later gate from `view`"""
    PO = pts["pos"][k].astype(np.float64) - view[0]["Ow"].astype(np.float64)
    dist = np.linalg.norm(PO)
    pts["normal"][k] = (PO / dist).astype(f32)
    pts["max_distance"][k] = f32(dist * 1.5)
    pts["min_distance"][k] = pts["max_distance"][k] / SF[-1]
    pts["flags"][k] = FLAG_OBSERVED


FAMILIES = ("pan", "translation", "behind", "pcz_zero", "on_bounds", "on_distance_gates", "viewcos_edges", "level_edges", "nan_position", "bad_flags")
# the statuses a family is built for
FAMILY_STATUS = {"pan": (ST_BAD, ST_DEPTH, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_VIEW_ANGLE, ST_LEVEL_RANGE, ST_IN_VIEW),
                 "translation": (ST_DEPTH, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_VIEW_ANGLE, ST_IN_VIEW), "behind": (ST_DEPTH,),
                 "pcz_zero": (ST_OUT_OF_IMAGE,), "on_bounds": (ST_OUT_OF_IMAGE, ST_IN_VIEW), "on_distance_gates": (ST_DISTANCE, ST_IN_VIEW),
                 "viewcos_edges": (ST_VIEW_ANGLE, ST_IN_VIEW), "level_edges": (ST_LEVEL_RANGE, ST_IN_VIEW), "nan_position": (ST_OUT_OF_IMAGE,),
                 "bad_flags": (ST_BAD,)}


def frame_scene(seed, n=500, sf=SF):
    """LastFrame's side of the frame/frame gate set: (view, points, last_ids, octaves): feature i holds pool id last_ids[i] or -1"""
    rng = np.random.default_rng(5000 + seed)
    view = pan_view(seed)
    pts = scene_points(rng, view, n, behind=0.1)
    for k in range(0, n, 25):                                          # z == 0 in both signs, with and without x == 0
        pts["pos"][k] = (view[0]["Ow"].astype(np.float64) + camera_of(view)[0].T @ np.array([(0.0, 1.0)[(k // 25) % 2], 0.2, 0.0])).astype(f32)
    ids = rng.permutation(n).astype(np.int32)
    ids[rng.random(n) < 0.2] = -1
    octaves = rng.integers(0, len(sf), n).astype(np.int32)
    return view, pts, ids, octaves


def model64(view, points, ids, th, sf=SF, log_sf=LOG_SF, margin=MARGIN):
    """Frame::isInFrustum's geometry in float64 numpy over a local-map list: (status, level, u, v, near) -- near marks the points
    within `margin` of a gate they reach (relative for distance, viewCos and the fractional level, pixels for the bounds, depth
    units for z), whose status float rounding may decide either way"""
    R, t, Ow = camera_of(view)
    v = view[0]
    K = v["K"].astype(np.float64)
    P = points[ids]
    X = P["pos"].astype(np.float64)
    n = len(ids)
    status = np.full(n, -1)
    near = np.zeros(n, bool)
    level = np.full(n, -1)
    with np.errstate(all="ignore"):
        Pc = X @ R.T + t
        z = Pc[:, 2]
        u = K[0] * Pc[:, 0] / z + K[2]
        w = K[1] * Pc[:, 1] / z + K[3]
        d = X - Ow
        dist = np.sqrt((d * d).sum(1))
        mn, mx = 0.8 * P["min_distance"].astype(np.float64), 1.2 * P["max_distance"].astype(np.float64)
        vc = (d * P["normal"].astype(np.float64)).sum(1) / dist
        lf = np.log(P["max_distance"].astype(np.float64) / dist) / np.float64(log_sf)
        lv = np.ceil(lf)

    def gate(fails, close, code):
        open_ = status < 0
        near[open_ & close] = True
        status[open_ & fails] = code

    gate((P["flags"] & FLAG_BAD) != 0, np.zeros(n, bool), ST_BAD)
    gate(z < 0, np.abs(z) < margin, ST_DEPTH)
    bx0, bx1, by0, by1 = float(v["min_x"]), float(v["max_x"]), float(v["min_y"]), float(v["max_y"])
    gate(~((u >= bx0) & (u <= bx1) & (w >= by0) & (w <= by1)),
         (np.abs(u - bx0) < margin) | (np.abs(u - bx1) < margin) | (np.abs(w - by0) < margin) | (np.abs(w - by1) < margin), ST_OUT_OF_IMAGE)
    gate((dist < mn) | (dist > mx), (np.abs(dist - mn) < margin * mn) | (np.abs(dist - mx) < margin * mx), ST_DISTANCE)
    gate(vc < float(v["viewing_cos_limit"]), np.abs(vc - float(v["viewing_cos_limit"])) < margin * float(v["viewing_cos_limit"]), ST_VIEW_ANGLE)
    gate(~((lv >= 0) & (lv < len(sf))), np.abs(lf - np.round(lf)) < margin, ST_LEVEL_RANGE)
    inview = status < 0
    near[inview & (np.abs(vc - 0.998) < margin * 0.998)] = True          # the radius switch of RadiusByViewingCos
    status[inview] = ST_IN_VIEW
    level[inview] = lv[inview].astype(int)
    return status, level, u, w, near


def points_from_keys(rng, view, keys, sf=SF, desc=None, jitter=1.0):
    """one MapPoint per keypoint, placed so that `view` sees it within `jitter` pixels of the keypoint, at the keypoint's octave
    (max distance = 0.95 dist x scale[octave]), looking at the camera within 26 degrees (viewCos on both sides of 0.998), with the
    keypoint's descriptor; 90 % observed, 3 % bad"""
    R, t, Ow = camera_of(view)
    K = view[0]["K"].astype(np.float64)
    n = len(keys)
    z = rng.uniform(2.0, 15.0, n)
    u = keys["x"].astype(np.float64) + rng.normal(0, jitter, n)
    v = keys["y"].astype(np.float64) + rng.normal(0, jitter, n)
    Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    Xw = (Xc - t) @ R
    pts = np.zeros(n, POINT_DTYPE)
    pts["pos"] = Xw.astype(f32)
    d = Xw - Ow
    dist = np.linalg.norm(d, axis=1)
    dirv = d / dist[:, None]
    c = np.where(rng.random(n) < 0.5, rng.uniform(0.9985, 1.0, n), rng.uniform(0.9, 0.9975, n))
    rnd = rng.normal(size=(n, 3))
    orth = rnd - (rnd * dirv).sum(1)[:, None] * dirv
    orth /= np.linalg.norm(orth, axis=1)[:, None]
    pts["normal"] = (c[:, None] * dirv + np.sqrt(1 - c * c)[:, None] * orth).astype(f32)
    pts["max_distance"] = (0.95 * dist * sf[keys["octave"]].astype(np.float64)).astype(f32)
    pts["min_distance"] = pts["max_distance"] / sf[-1]
    if desc is not None:
        pts["desc"] = desc
    fl = np.where(rng.random(n) < 0.9, FLAG_OBSERVED, 0) | np.where(rng.random(n) < 0.03, FLAG_BAD, 0)
    pts["flags"] = fl.astype(np.uint8)
    return pts


# ------------------------------------------------------------------ the device side: what tests/test_gpu_localmap.py and
# tests/one_handle_cases.py share
NF = 500
D0 = [0, 0, 0, 0, 0]


class Rig:
    """three 640 x 480 frames of about 500 features resident in a frame set of four slots, their host copies, a matcher, the level
    tables"""

    def __init__(self):
        from orbslamm_amd import ORBextractor, ORBmatcher, level_breaks, make_grid, synth
        self.gex = ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=3, device=0)
        self.sf = np.array(self.gex.GetScaleFactors(), np.float32)
        assert np.array_equal(self.sf, SF)
        self.m = ORBmatcher(0.8, True, device=0)
        self.grid = make_grid(0.0, 0.0, float(W), float(H))
        self.fs = self.new_frame_set()
        self.gex.extract_batch_device(*self.gex.upload_frames(synth.make_frames(W, H, 3, stream=17)))
        self.fs.build_from_extractor(0, self.gex)
        self.host = [self.gex.download(f) for f in range(3)]
        self.breaks = level_breaks(LOG_SF, NLEVELS)
        self.breaks_b = level_breaks(LOG_SF_B, NLEVELS)

    def new_frame_set(self):
        return self.m.frame_set(4, self.gex.max_keypoints, K_A, D0, self.grid, list(BOUNDS), self.sf)


def new_pool(rig, capacity):
    from orbslamm_amd import MapPool
    return MapPool(rig.m, capacity)
