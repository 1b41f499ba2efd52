"""SearchInNeighbors' checker for the tests: the C++ restatement (tools/fuse_ref.hpp) built with g++ -ffp-contract=off behind
a small C shim (tests/cpp/fuse_ref_capi.cpp), seeded scene families on 640 x 480 with real geometry, the per-target
reference (the restatement's projection, then the oracle's window_best with the chi-square gate) and a float64 numpy
recount of the four projection gates and of the level that shares no code with the restatement."""
import ctypes as C
import functools

import numpy as np

from matcher_cases import noisy_copies
from ref_shim import cached_shim, p as _p, rot_axis_angle as _rot, same
from orbslamm_amd._lib import KP_DTYPE
from orbslamm_amd.local_mapping import (FUSE_POINT_DTYPE, FUSE_RESULT_DTYPE, FUSE_ST_DEPTH, FUSE_ST_DISTANCE, FUSE_ST_FOUND,
                                        FUSE_ST_LEVEL_RANGE, FUSE_ST_NO_CANDIDATE, FUSE_ST_OUTSIDE_IMAGE, FUSE_ST_VIEW_ANGLE,
                                        FUSE_TARGET_DTYPE, fuse_points, fuse_target)

rot_axis_angle = functools.partial(_rot, scale_first=True)   # (how this module's scenes were generated: ref_shim.rot_axis_angle)

f32, f64 = np.float32, np.float64
W, H = 640.0, 480.0
K_A = np.array([517.3, 516.5, 318.6, 255.3], dtype=f32)
K_B = np.array([458.7, 457.3, 367.2, 248.4], dtype=f32)     # (mixed_intrinsics: a target from another camera)
NLEVELS = 8
SCALE_FACTOR = f32(1.2)
LOG_SF = f32(np.log(SCALE_FACTOR))                          # mfLogScaleFactor = log(mfScaleFactor), a float
SF = np.array([SCALE_FACTOR ** l for l in range(NLEVELS)], dtype=f32)
INV_SIGMA2 = (f32(1.0) / (SF * SF)).astype(f32)
TH = 3.0
GATES_DTYPE = np.dtype([("z", "<f4"), ("dist3D", "<f4"), ("min", "<f4"), ("max", "<f4"), ("ratio", "<f4"), ("radius", "<f4"), ("dot", "<f8")])

# Bands of the float64 recount, MEASURED from the restatement on the CPU over seeds 0..4 of every family (measure() below,
# `PYTHONPATH=. python tests/fuse_cases.py`), then given the margin of 4x this project uses (newpoints_cases.py):
#   z = (Rcw p + tcw)(2) relative to |p3Dc|                      measured max 2.17e-7  (single_target_many_points)
#   u, v in pixels (against the image bounds)                    measured max 9.26e-4  (behind_camera)
#   dist3D relative to itself (against 0.8 min and 1.2 max)      measured max 1.16e-7  (single_target_many_points)
#   PO.Pn - 0.5 dist3D relative to dist3D                        measured max 7.83e-8  (view_angle)
#   log(ratio)/log(1.2) (against the integers), absolute         measured max 1.44e-6  (level_range)
# Outside the bands no gate decision of those runs disagreed with the float64 recount; the largest share of a case's pairs
# inside a band was 0.0003 (view_angle seed 4): the 2 % cap (a condition, not a measurement) holds for every
# family and seed used.
BAND = dict(z=4 * 2.17e-7, uv=4 * 9.26e-4, dist=4 * 1.16e-7, dot=4 * 7.83e-8, level=4 * 1.44e-6)
BAND_SHARE_CAP = 0.02
SEEDS = range(5)

def _declare(L):
    vp = C.c_void_p
    L.fuseref_project.argtypes = [vp, vp, vp, C.c_int, C.c_float, vp, C.c_int, C.c_float, vp, vp]
    L.fuseref_project.restype = None
    L.fuseref_target.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, vp, vp, C.c_int, C.c_float, vp]
    L.fuseref_target.restype = None
    L.fuseref_level_sweep.argtypes = [C.c_float, C.c_int, vp, C.c_uint32, C.c_uint32, vp]
    L.fuseref_level_sweep.restype = C.c_int64
    L.fuseref_model_new.argtypes = [C.c_float, vp, vp, C.c_int, C.c_float]
    L.fuseref_model_new.restype = vp
    L.fuseref_model_free.argtypes = [vp]
    L.fuseref_model_free.restype = None
    L.fuseref_add_keyframe.argtypes = [vp, vp, vp, vp, C.c_int]
    L.fuseref_set_covisibles.argtypes = [vp, C.c_int, vp, C.c_int]
    L.fuseref_set_covisibles.restype = None
    L.fuseref_add_map_point.argtypes = [vp, vp]
    L.fuseref_add_observation.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.fuseref_add_observation.restype = None
    L.fuseref_search_in_neighbors.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp]
    L.fuseref_search_in_neighbors.restype = None
    L.fuseref_keyframe_slots.argtypes = [vp, C.c_int, vp]
    L.fuseref_keyframe_slots.restype = None
    L.fuseref_map_point.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int]
    assert [L.fuseref_sizes(i) for i in range(5)] == [FUSE_TARGET_DTYPE.itemsize, FUSE_POINT_DTYPE.itemsize, FUSE_RESULT_DTYPE.itemsize,
                                                      KP_DTYPE.itemsize, GATES_DTYPE.itemsize]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("fuse_ref", _declare)


# ------------------------------------------------------------------------------------------------ the references
def ref_project(case, k, idx, want_gates=False):
    """the restatement's :855-892 of the pool's points idx against target k: (results, gates)"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    rec = np.ascontiguousarray(case["targets"][k]["rec"], dtype=FUSE_TARGET_DTYPE)
    out = np.zeros(len(idx), dtype=FUSE_RESULT_DTYPE)
    gates = np.zeros(len(idx), dtype=GATES_DTYPE) if want_gates else None
    ref_lib().fuseref_project(_p(rec), _p(case["points"]), _p(idx), len(idx), C.c_float(case["th"]), _p(case["sf"]), len(case["sf"]),
                              C.c_float(case["log_sf"]), _p(out), _p(gates))
    return out, gates


def ref_target(case, k, idx):
    """the restatement's :855-951 (its own grid and window walk) of the pool's points idx against target k"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    t = case["targets"][k]
    rec = np.ascontiguousarray(t["rec"], dtype=FUSE_TARGET_DTYPE)
    out = np.zeros(len(idx), dtype=FUSE_RESULT_DTYPE)
    ref_lib().fuseref_target(_p(rec), _p(t["keys"]), _p(t["desc"]), len(t["keys"]), _p(case["points"]), _p(idx), len(idx), C.c_float(case["th"]),
                             _p(case["sf"]), _p(case["inv_sigma2"]), len(case["sf"]), C.c_float(case["log_sf"]), _p(out))
    return out


def oracle_grid(oracle, rec):
    g = rec["grid"]
    gp = oracle.OrcGridParams()
    gp.minX, gp.minY, gp.invW, gp.invH, gp.cols, gp.rows = (float(g["minX"]), float(g["minY"]), float(g["invW"]), float(g["invH"]),
                                                             int(g["cols"]), int(g["rows"]))
    return gp


def window_queries(case, res, idx):
    """what ORBmatcherT::Fuse hands to window_best for the pairs that passed the projection gates: (rows, q_uvr, q_pred, qdesc)"""
    rows = np.flatnonzero(res["status"] == FUSE_ST_NO_CANDIDATE)
    uvr = np.stack([res["u"][rows], res["v"][rows], (f32(case["th"]) * case["sf"][res["level"][rows]]).astype(f32)], axis=1).astype(f32)
    return rows, uvr.reshape(-1, 3), res["level"][rows].astype(np.int8), np.ascontiguousarray(case["points"]["desc"][np.asarray(idx)[rows]])


def reference(oracle, case):
    """the per-target reference: the restatement's projection of every job entry, then the oracle's window_best (chi2) for
    the survivors of each target.  A FUSE_RESULT_DTYPE array in job order."""
    js, jp = case["jobs"]
    out = np.zeros(int(js[-1]) if len(js) else 0, dtype=FUSE_RESULT_DTYPE)
    for k, t in enumerate(case["targets"]):
        idx = jp[js[k]:js[k + 1]]
        res, _ = ref_project(case, k, idx)
        rows, uvr, pred, qd = window_queries(case, res, idx)
        if len(rows) and len(t["keys"]):
            gp = oracle_grid(oracle, t["rec"])
            start, cidx = oracle.grid_build(gp, t["keys"])
            bi, bd = oracle.window_best(uvr, pred, qd, None, gp, t["keys"], start, cidx, t["desc"], case["inv_sigma2"], chi2=True)
            res["best_idx"][rows], res["best_dist"][rows] = bi, bd
            res["status"][rows] = np.where(bi >= 0, FUSE_ST_FOUND, FUSE_ST_NO_CANDIDATE)
        out[js[k]:js[k + 1]] = res
    return out


# ------------------------------------------------------------------------------------------------ scenes
def grid_tuple(cols=64, rows=48, minX=0.0, minY=0.0, maxX=W, maxY=H):
    """Frame.cc:212-213 in float"""
    return (f32(minX), f32(minY), f32(cols) / f32(f32(maxX) - f32(minX)), f32(rows) / f32(f32(maxY) - f32(minY)), cols, rows)


# family -> parameters.  targets / points: the ranges the seed draws the counts from; feats: features per target; spread:
# how far beyond the image the cloud reaches (in image widths); turn: the largest rotation of a target away from the
# cloud (radians); the *_share entries spoil that share of the points for one gate
FAMILIES = {
    "general": dict(),
    "behind_camera": dict(turn=2.6, spread=1.5),
    "outside_image": dict(spread=1.0),
    "distance_range": dict(distance_share=0.5),
    "view_angle": dict(normal_share=0.5),
    "level_range": dict(level_share=0.6),
    "crowded_ties": dict(ties=True),
    "chi2_edge": dict(chi2=True),
    "mixed_intrinsics": dict(mixed=True),
    "repeated_target": dict(repeat=True),
    "single_target_many_points": dict(targets=(1, 1), points=(20000, 20000), feats=2000, pix_noise=0.4),
}
# what every family must show: its gate's status code, and a floor on FOUND over its five seeds.  The floors were fixed after
# running the restatement alone on the CPU (measure()): the smallest count of a family, rounded down to about a half.
FAMILY_CODES = {"behind_camera": FUSE_ST_DEPTH, "outside_image": FUSE_ST_OUTSIDE_IMAGE, "distance_range": FUSE_ST_DISTANCE,
                "view_angle": FUSE_ST_VIEW_ANGLE, "level_range": FUSE_ST_LEVEL_RANGE}
FOUND_FLOOR = {"general": 1400, "behind_camera": 290, "outside_image": 250, "distance_range": 990, "view_angle": 2100, "level_range": 2000,
               "crowded_ties": 1900, "chi2_edge": 1100, "mixed_intrinsics": 2100, "repeated_target": 3400, "single_target_many_points": 6700}


def make_case(seed, targets=(3, 6), points=(300, 600), feats=500, spread=0.15, turn=0.12, distance_share=0.0, normal_share=0.0,
              level_share=0.0, ties=False, chi2=False, mixed=False, repeat=False, pix_noise=0.5, flips=10, vis=0.8, all_points=None,
              grid=None):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(targets[0], targets[1] + 1))
    N = int(rng.integers(points[0], points[1] + 1))
    K0 = K_A.astype(f64)
    # the cloud in front of a base camera at a generic pose
    z = rng.uniform(4, 9, N)
    px = rng.uniform(-spread * W, (1 + spread) * W, N)
    py = rng.uniform(-spread * H, (1 + spread) * H, N)
    Xb = np.stack([(px - K0[2]) / K0[0] * z, (py - K0[3]) / K0[1] * z, z], axis=1)
    Rb = rot_axis_angle(rng.normal(size=3), 0.3)
    Ob = rng.normal(size=3) * 2.0
    X = Xb @ Rb + Ob
    # the points' own reference observation: the base camera, at level lref
    lref = rng.integers(1, 6, N)
    dref = np.linalg.norm(X - Ob, axis=1)
    normal = (X - Ob) / dref[:, None]
    maxd = dref * SF.astype(f64)[lref]
    mind = maxd / f64(SF[NLEVELS - 1])
    spoil = rng.uniform(size=N)
    if distance_share:      # bounds that belong to another depth: dist3D falls below 0.8 min or above 1.2 max
        s = spoil < distance_share
        f = np.where(rng.uniform(size=N) < 0.5, rng.uniform(4.5, 7.0, N), rng.uniform(0.08, 0.2, N))
        maxd, mind = np.where(s, maxd * f, maxd), np.where(s, mind * f, mind)
    if normal_share:        # normals that look elsewhere: around and beyond 60 degrees
        s = np.flatnonzero(spoil < normal_share)
        for i in s:
            normal[i] = rot_axis_angle(rng.normal(size=3), rng.uniform(0.6, 2.2)) @ normal[i]
    if level_share:         # a raw maximum distance whose ratio predicts a level above the last, inside the distance gate (the lowest
                            # level's side ends at the distance gate: ratio <= 1/1.2 is dist3D >= 1.2 max)
        s = spoil < level_share
        lref = np.where(s, np.where(rng.uniform(size=N) < 0.5, 0, NLEVELS - 1), lref)
        maxd = dref * SF.astype(f64)[lref] * np.where(s, rng.uniform(0.85, 1.15, N), 1.0)
        mind = maxd / f64(SF[NLEVELS - 1])
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    pool = fuse_points(X, normal, mind, maxd, base)
    sf64 = SF.astype(f64)
    tg = []
    for k in range(T):
        Kt = K_B if (mixed and k % 2 == 0) else K_A
        R = rot_axis_angle(rng.normal(size=3), rng.uniform(0, turn)) @ Rb
        O = Ob + (rng.normal(size=3) * np.array([0.5, 0.3, 0.6])) @ Rb
        bounds = (0.0, W, 0.0, H)
        g = grid if grid is not None else grid_tuple()
        if mixed and k % 2 == 0:       # another camera: undistorted bounds beyond the sensor, and a finer grid than the 64 x 48 cell table
            bounds = (-12.5, 655.25, -9.75, 492.5)
            g = grid_tuple(80, 60, bounds[0], bounds[2], bounds[1], bounds[3])
        rec = fuse_target(R, -R @ O, O, Kt, bounds, g, keys=np.zeros(0, KP_DTYPE), desc=np.zeros((0, 32), np.uint8))["rec"]
        # where the restatement projects the points, and at which level: the features are laid around that
        tmp = dict(targets=[dict(rec=rec)], points=pool, th=TH, sf=SF, log_sf=LOG_SF)
        pr, _ = ref_project(tmp, 0, np.arange(N))
        okp = np.flatnonzero((pr["status"] == FUSE_ST_NO_CANDIDATE) & (rng.uniform(size=N) < vis))
        if len(okp) > feats * 3 // 4:
            okp = rng.choice(okp, feats * 3 // 4, replace=False)
        lvl = pr["level"][okp].astype(np.int64)
        oct_ = np.clip(lvl - (rng.uniform(size=len(okp)) < 0.4), 0, NLEVELS - 1)           # the level window is [pred - 1, pred]
        oct_ = np.where(rng.uniform(size=len(okp)) < 0.08, np.clip(lvl + rng.choice([-2, 1], len(okp)), 0, NLEVELS - 1), oct_)
        u, v = pr["u"][okp].astype(f64), pr["v"][okp].astype(f64)
        if chi2:             # keys around the radius where e2 * invSigma2 meets 5.99, from far inside a float's spacing to a percent
            r = np.sqrt(5.99 * sf64[oct_] ** 2) * (1 + rng.choice([-1, 1], len(okp)) * 10.0 ** rng.uniform(-7.5, -2, len(okp)))
            ang = rng.uniform(0, 2 * np.pi, len(okp))
            ku, kv = u + r * np.cos(ang), v + r * np.sin(ang)
        else:
            ku, kv = u + rng.normal(0, pix_noise, len(okp)) * sf64[oct_], v + rng.normal(0, pix_noise, len(okp)) * sf64[oct_]
        kd = noisy_copies(rng, base[okp], flips)
        parts = [(ku, kv, oct_, kd)]
        if ties:             # a second and third feature inside the same window with the very same descriptor: the first in walk order wins
            for _ in range(2):
                s = rng.uniform(size=len(okp)) < 0.5
                parts.append((ku[s] + rng.uniform(-1.2, 1.2, s.sum()), kv[s] + rng.uniform(-1.2, 1.2, s.sum()), oct_[s], kd[s]))
        nf = sum(len(p[0]) for p in parts)
        nclut = max(feats - nf, feats // 10)
        parts.append((rng.uniform(bounds[0] + 1, bounds[1] - 1, nclut), rng.uniform(bounds[2] + 1, bounds[3] - 1, nclut),
                      rng.integers(0, NLEVELS, nclut), rng.integers(0, 256, (nclut, 32), dtype=np.uint8)))
        n = nf + nclut
        keys = np.zeros(n, dtype=KP_DTYPE)
        keys["x"], keys["y"] = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        keys["octave"] = np.concatenate([p[2] for p in parts])
        keys["size"], keys["angle"], keys["response"], keys["class_id"] = 31.0 * SF[keys["octave"]], rng.uniform(0, 360, n), 50.0, -1
        desc = np.concatenate([p[3] for p in parts])
        perm = rng.permutation(n)
        tg.append(dict(rec=rec, keys=np.ascontiguousarray(keys[perm]), desc=np.ascontiguousarray(desc[perm])))
    if repeat:               # a second neighbour pushed again: the same keyframe further down the list, with other jobs
        tg = tg + [tg[0], tg[len(tg) // 2]]
    # jobs: SearchInNeighbors' first phase lists the same points for every target; the generators also leave points out and shuffle
    starts, jp = [0], []
    for k in range(len(tg)):
        if all_points if all_points is not None else (k % 2 == 0):
            idx = np.arange(N)
        else:
            idx = rng.permutation(N)[:rng.integers(N // 2, N + 1)]
        jp.append(idx)
        starts.append(starts[-1] + len(idx))
    return dict(targets=tg, points=pool, jobs=(np.array(starts, np.int32), np.concatenate(jp).astype(np.int32)), th=TH, sf=SF.copy(),
                inv_sigma2=INV_SIGMA2.copy(), log_sf=LOG_SF, nlevels=NLEVELS)


def family_case(name, seed):
    return make_case(1000 * (sorted(FAMILIES).index(name) + 1) + seed, **FAMILIES[name])


def dropin_scene(seed=0):
    """A small map for tests/cpp/fuse_dropin_gpu.cpp: keyframe 0 is the current one, 1..6 its covisibles, whose own covisibility
    lists name each other and keyframe 0 (second neighbours are pushed again and again).  Every world point the current
    keyframe sees may be a map point A of it; in the targets the same world point is another map point B (a Replace either
    way round, by the observation counts), a free feature (AddObservation) or, sometimes, A itself.  The associations come
    from the restatement: a point belongs to the feature Fuse would pick for it.  Returns a dict of flat arrays."""
    rng = np.random.default_rng(9000 + seed)
    case = make_case(9100 + seed, targets=(7, 7), points=(500, 500), feats=500, spread=0.05, turn=0.06, vis=0.9)
    nk, pool = len(case["targets"]), case["points"]
    assoc = []
    for k in range(nk):
        res = ref_target(case, k, np.arange(len(pool)))
        used, a = set(), {}
        for pi in np.flatnonzero((res["status"] == FUSE_ST_FOUND) & (res["best_dist"] <= 30)):
            if int(res["best_idx"][pi]) not in used:
                used.add(int(res["best_idx"][pi]))
                a[int(pi)] = int(res["best_idx"][pi])
        assoc.append(a)
    points, obs = [], []

    def new_point(pi, where):
        rec = pool[pi].copy()
        rec["desc"] = case["targets"][where[0]]["desc"][assoc[where[0]][pi]]
        points.append(rec)
        obs.extend((len(points) - 1, k, assoc[k][pi]) for k in where)

    for pi in range(len(pool)):
        seen = [k for k in range(1, nk) if pi in assoc[k]]
        rng.shuffle(seen)
        if pi in assoc[0] and rng.uniform() < 0.7:
            extra = seen[:1] if seen and rng.uniform() < 0.3 else []
            new_point(pi, [0] + extra)
            seen = seen[len(extra):]
        if seen and rng.uniform() < 0.6:
            new_point(pi, sorted(seen[:int(rng.integers(1, 4))]))
    covis = [[1, 2, 3, 4, 5, 6]] + [[0, k % 6 + 1, (k + 2) % 6 + 1] for k in range(1, nk)]
    return dict(case=case, points=np.array(points, dtype=FUSE_POINT_DTYPE), obs=np.array(obs, np.int32).reshape(-1, 3), covis=covis)


def write_dropin_scene(scene, path):
    """the scene as the flat file tests/cpp/fuse_dropin_gpu.cpp reads: the counts, the level tables and the log scale factor,
    every keyframe as (record, n, keys, descriptors, its covisibles), the map points' records, the observations"""
    case = scene["case"]
    with open(path, "wb") as f:
        np.array([len(case["targets"]), len(scene["points"]), len(scene["obs"])], np.int32).tofile(f)
        case["sf"][:8].astype(f32).tofile(f)
        case["inv_sigma2"][:8].astype(f32).tofile(f)
        np.array([case["log_sf"]], f32).tofile(f)
        for t, cv in zip(case["targets"], scene["covis"]):
            np.ascontiguousarray(t["rec"], dtype=FUSE_TARGET_DTYPE).tofile(f)
            np.array([len(t["keys"])], np.int32).tofile(f)
            np.ascontiguousarray(t["keys"], dtype=KP_DTYPE).tofile(f)
            np.ascontiguousarray(t["desc"], dtype=np.uint8).tofile(f)
            np.array([len(cv)] + list(cv), np.int32).tofile(f)
        np.ascontiguousarray(scene["points"], dtype=FUSE_POINT_DTYPE).tofile(f)
        np.ascontiguousarray(scene["obs"], dtype=np.int32).tofile(f)


# ------------------------------------------------------------------------------------------------ the float64 recount
def recount64(case, k, idx):
    """the four projection gates and the level in float64 from the same float32 inputs: (status, level, near, gaps): near
    marks the pairs with a gate quantity, up to the deciding gate, inside its band; gaps the distance of the restatement's
    float quantities from these (what BAND is measured from)"""
    rec, P = case["targets"][k]["rec"], case["points"][np.asarray(idx)]
    R, t, O, Kc = (np.asarray(rec[n], f64) for n in ("Rcw", "tcw", "Ow", "K"))
    b = np.asarray(rec["bounds"], f64)
    X, Pn = P["pos"].astype(f64), P["normal"].astype(f64)
    pc = X @ R.T + t
    npc = np.linalg.norm(pc, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = Kc[0] * pc[:, 0] / pc[:, 2] + Kc[2], Kc[1] * pc[:, 1] / pc[:, 2] + Kc[3]
    PO = X - O
    dist = np.linalg.norm(PO, axis=1)
    mn, mx = f64(f32(0.8)) * P["min_distance"].astype(f64), f64(f32(1.2)) * P["max_distance"].astype(f64)
    dot = np.einsum("ij,ij->i", PO, Pn)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.log(P["max_distance"].astype(f64) / dist) / np.log(f64(SCALE_FACTOR))
    lvl = np.ceil(q)
    n = len(P)
    status = np.full(n, FUSE_ST_NO_CANDIDATE, np.uint8)
    near = np.zeros(n, bool)
    decided = np.zeros(n, bool)

    def gate(fails, close, code):
        nonlocal decided
        near[~decided & close] = True
        hit = ~decided & fails
        status[hit] = code
        decided |= hit

    gate(pc[:, 2] < 0, np.abs(pc[:, 2]) <= BAND["z"] * npc, FUSE_ST_DEPTH)
    duv = np.minimum.reduce([np.abs(u - b[0]), np.abs(u - b[1]), np.abs(v - b[2]), np.abs(v - b[3])])
    gate(~((u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])), duv <= BAND["uv"], FUSE_ST_OUTSIDE_IMAGE)
    gate((dist < mn) | (dist > mx), (np.abs(dist - mn) <= BAND["dist"] * dist) | (np.abs(dist - mx) <= BAND["dist"] * dist), FUSE_ST_DISTANCE)
    gate(dot < 0.5 * dist, np.abs(dot - 0.5 * dist) <= BAND["dot"] * dist, FUSE_ST_VIEW_ANGLE)
    gate(~((lvl >= 0) & (lvl < case["nlevels"])), np.abs(q - np.rint(q)) <= BAND["level"], FUSE_ST_LEVEL_RANGE)
    near[~decided & (np.abs(q - np.rint(q)) <= BAND["level"])] = True
    return status, lvl, near, dict(pc=pc, npc=npc, u=u, v=v, dist=dist, dot=dot, q=q)


def check64(case):
    """against float64 over every job entry: (decisions that disagree outside the bands, the share of pairs inside a band,
    pairs).  A decision is the status up to LEVEL_RANGE and, for a pair that reaches the window, the level."""
    js, jp = case["jobs"]
    outside = inband = total = 0
    for k in range(len(case["targets"])):
        idx = jp[js[k]:js[k + 1]]
        res, _ = ref_project(case, k, idx)
        st64, lvl64, near, _ = recount64(case, k, idx)
        differs = res["status"] != st64
        alive = (res["status"] == FUSE_ST_NO_CANDIDATE) & ~differs
        differs[alive] = res["level"][alive] != lvl64[alive]
        outside += int((differs & ~near).sum())
        inband += int(near.sum())
        total += len(idx)
    return outside, (inband / total if total else 0.0), total


def gaps64(case):
    """per gate, the largest gap between the restatement's float quantity and its float64 recount over the pairs that reached it"""
    js, jp = case["jobs"]
    worst = dict(z=0.0, uv=0.0, dist=0.0, dot=0.0, level=0.0)
    for k in range(len(case["targets"])):
        idx = jp[js[k]:js[k + 1]]
        res, g = ref_project(case, k, idx, want_gates=True)
        _, _, _, w = recount64(case, k, idx)
        worst["z"] = max(worst["z"], float(np.max(np.abs(g["z"].astype(f64) - w["pc"][:, 2]) / w["npc"])))
        r = res["status"] >= FUSE_ST_OUTSIDE_IMAGE
        inside = r & (np.abs(w["u"]) < 4 * W) & (np.abs(w["v"]) < 4 * H)      # (pixels far outside carry large absolute errors and decide nothing)
        if inside.any():
            worst["uv"] = max(worst["uv"], float(np.max(np.maximum(np.abs(res["u"].astype(f64) - w["u"]), np.abs(res["v"].astype(f64) - w["v"]))[inside])))
        r = res["status"] >= FUSE_ST_DISTANCE
        if r.any():
            worst["dist"] = max(worst["dist"], float(np.max((np.abs(g["dist3D"].astype(f64) - w["dist"]) / w["dist"])[r])))
        r = res["status"] >= FUSE_ST_VIEW_ANGLE
        if r.any():
            worst["dot"] = max(worst["dot"], float(np.max((np.abs((g["dot"] - 0.5 * g["dist3D"].astype(f64)) - (w["dot"] - 0.5 * w["dist"])) / w["dist"])[r])))
        r = res["status"] >= FUSE_ST_LEVEL_RANGE
        if r.any():
            qf = np.log(g["ratio"].astype(f32)[r]) / LOG_SF       # the float quotient PredictScale rounds up
            worst["level"] = max(worst["level"], float(np.max(np.abs(qf.astype(f64) - w["q"][r]))))
    return worst


def measure():
    """prints what the constants at the top of this file were taken from"""
    from oracle import binding as ob
    ob.build()
    worst_gap = {kind: (0.0, "") for kind in BAND}
    worst_share = (0.0, "")
    for name in sorted(FAMILIES):
        found_total = 0
        for seed in SEEDS:
            case = family_case(name, seed)
            want = reference(ob, case)
            gap = gaps64(case)
            outside, share, total = check64(case)
            counts = np.bincount(want["status"], minlength=7)
            found_total += int(counts[FUSE_ST_FOUND])
            low = int(((want["status"] == FUSE_ST_FOUND) & (want["best_dist"] <= 50)).sum())
            print("%-26s seed %d  targets %d  pairs %6d  codes %s  fused %5d  gaps %s  outside %d  share %.4f" %
                  (name, seed, len(case["targets"]), total, counts.tolist(), low, " ".join("%s %.3g" % kv for kv in sorted(gap.items())), outside, share))
            worst_share = max(worst_share, (share, "%s seed %d" % (name, seed)))
            worst_gap = {kind: max(worst_gap[kind], (gap[kind], name)) for kind in BAND}
        print("%-26s FOUND over the seeds: %d" % (name, found_total))
    print("gate gaps", worst_gap, "band share (at the BAND in force)", worst_share)


if __name__ == "__main__":
    measure()
