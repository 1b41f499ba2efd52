"""SearchAndFuse's checker for the tests: the C++ restatement (tools/loopfuse_ref.hpp) built with g++ -ffp-contract=off behind
a small C shim (tests/cpp/loopfuse_ref_capi.cpp), seeded dense scene families on 640 x 480 (fuse_cases.make_case's geometry,
every point against every target), the reference of the device call (the restatement's projection, then the oracle's
window_best WITHOUT the chi-square gate), a float64 numpy recount of the gates that shares no code with the restatement,
and the map scenes of the serial model."""
import ctypes as C

import numpy as np

import fuse_cases as fc
from fuse_cases import grid_tuple, make_case, rot_axis_angle  # noqa: F401
from ref_shim import cached_shim, p as _p
from orbslamm_amd._lib import KP_DTYPE
from orbslamm_amd.local_mapping import (FUSE_POINT_DTYPE, FUSE_RESULT_DTYPE, FUSE_ST_DEPTH, FUSE_ST_DISTANCE, FUSE_ST_FOUND,
                                        FUSE_ST_LEVEL_RANGE, FUSE_ST_NO_CANDIDATE, FUSE_ST_OUTSIDE_IMAGE, FUSE_ST_VIEW_ANGLE,
                                        FUSE_TARGET_DTYPE, GRID_DTYPE)
from orbslamm_amd.loop_closing import HIT_DTYPE, TH_LOW, decompose_sim3

f32, f64 = np.float32, np.float64
TH = 4.0                                                    # LoopClosing.cc:613 / MultiMapper.cc:687
GATES_DTYPE = fc.GATES_DTYPE

# Bands of the float64 recount, MEASURED from the restatement on the CPU over seeds 0..4 of every family (measure() below,
# `PYTHONPATH=. python tests/loopfuse_cases.py`), then given the margin of 4x this project uses (fuse_cases.py):
#   z = (Rcw p + tcw)(2) relative to |p3Dc|                      measured max 1.81e-7  (sparse_survivors)
#   u, v in pixels (against the image bounds)                    measured max 1.44e-3  (sparse_survivors)
#   dist3D relative to itself (against 0.8 min and 1.2 max)      measured max 1.16e-7  (level_range)
#   PO.Pn - 0.5 dist3D relative to dist3D                        measured max 7.83e-8  (view_angle)
#   log(ratio)/log(1.2) (against the integers), absolute         measured max 1.45e-6  (level_range)
# Outside the bands no gate decision of those runs disagreed with the float64 recount; the largest share of a case's pairs
# inside a band was 0.00030 (scaled_sim3 seed 3; view_angle seed 4 0.00029, sparse_survivors 0.00002, every other family
# 0): the 2 % cap (a condition, not a measurement) holds for every family and seed used.
MEASURED = dict(z=1.81e-7, uv=1.44e-3, dist=1.16e-7, dot=7.83e-8, level=1.45e-6)
MEASURED_SHARE = {"scaled_sim3": 0.00030, "view_angle": 0.00029, "sparse_survivors": 0.00002}
BAND = {k: 4 * v for k, v in MEASURED.items()}
BAND_SHARE_CAP = 0.02
SEEDS = range(5)

def _declare(L):
    vp = C.c_void_p
    L.loopref_project.argtypes = [vp, vp, C.c_int, C.c_float, vp, C.c_int, C.c_float, vp, vp]
    L.loopref_project.restype = None
    L.loopref_target.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_float, vp, C.c_int, C.c_float, vp]
    L.loopref_target.restype = None
    L.loopref_invz_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.loopref_invz_sweep.restype = C.c_int64
    L.loopref_model_new.argtypes = [vp, C.c_int, C.c_float]
    L.loopref_model_new.restype = vp
    L.loopref_model_free.argtypes = [vp]
    L.loopref_model_free.restype = None
    L.loopref_add_keyframe.argtypes = [vp, vp, vp, vp, C.c_int]
    L.loopref_add_map_point.argtypes = [vp, vp]
    L.loopref_add_observation.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.loopref_add_observation.restype = None
    L.loopref_search_and_fuse.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_float, vp, C.c_int, vp, vp]
    L.loopref_keyframe_slots.argtypes = [vp, C.c_int, vp]
    L.loopref_keyframe_slots.restype = None
    L.loopref_map_point.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int]
    assert [L.loopref_sizes(i) for i in range(6)] == [FUSE_TARGET_DTYPE.itemsize, FUSE_POINT_DTYPE.itemsize, FUSE_RESULT_DTYPE.itemsize,
                                                      KP_DTYPE.itemsize, GATES_DTYPE.itemsize, HIT_DTYPE.itemsize]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("loopfuse_ref", _declare)


# ------------------------------------------------------------------------------------------------ the references
def ref_project(case, k, want_gates=False):
    """the restatement's :1010-1051 of every point of the pool against target k: (results, gates)"""
    rec = np.ascontiguousarray(case["targets"][k]["rec"], dtype=FUSE_TARGET_DTYPE)
    P = len(case["points"])
    out = np.zeros(P, dtype=FUSE_RESULT_DTYPE)
    gates = np.zeros(P, dtype=GATES_DTYPE) if want_gates else None
    ref_lib().loopref_project(_p(rec), _p(case["points"]), P, C.c_float(case["th"]), _p(case["sf"]), len(case["sf"]), C.c_float(case["log_sf"]),
                              _p(out), _p(gates))
    return out, gates


def ref_target(case, k):
    """the restatement's :1010-1081 (its own grid and window walk) of every point of the pool against target k"""
    t = case["targets"][k]
    rec = np.ascontiguousarray(t["rec"], dtype=FUSE_TARGET_DTYPE)
    P = len(case["points"])
    out = np.zeros(P, dtype=FUSE_RESULT_DTYPE)
    ref_lib().loopref_target(_p(rec), _p(t["keys"]), _p(t["desc"]), len(t["keys"]), _p(case["points"]), P, C.c_float(case["th"]), _p(case["sf"]),
                             len(case["sf"]), C.c_float(case["log_sf"]), _p(out))
    return out


def oracle_target(oracle, case, k):
    """the restatement's projection of every point against target k, then the oracle's window_best without chi-square"""
    t = case["targets"][k]
    res, _ = ref_project(case, k)
    rows = np.flatnonzero(res["status"] == FUSE_ST_NO_CANDIDATE)
    if len(rows) and len(t["keys"]):
        uvr = np.stack([res["u"][rows], res["v"][rows], (f32(case["th"]) * case["sf"][res["level"][rows]]).astype(f32)], axis=1).astype(f32)
        gp = fc.oracle_grid(oracle, t["rec"])
        start, cidx = oracle.grid_build(gp, t["keys"])
        bi, bd = oracle.window_best(uvr.reshape(-1, 3), res["level"][rows].astype(np.int8), np.ascontiguousarray(case["points"]["desc"][rows]), None, gp,
                                    t["keys"], start, cidx, t["desc"], None, chi2=False)
        res["best_idx"][rows], res["best_dist"][rows] = bi, bd
        res["status"][rows] = np.where(bi >= 0, FUSE_ST_FOUND, FUSE_ST_NO_CANDIDATE)
    return res


def dense_from(per_target, max_dist=TH_LOW):
    """what the device call returns, from one FUSE_RESULT_DTYPE array per target: (hits, hit_start, status)"""
    hits, start, status = [], [0], []
    for k, res in enumerate(per_target):
        rows = np.flatnonzero((res["best_idx"] >= 0) & (res["best_dist"] <= max_dist))
        h = np.zeros(len(rows), dtype=HIT_DTYPE)
        h["target"], h["point"], h["best_idx"], h["best_dist"] = k, rows, res["best_idx"][rows], res["best_dist"][rows]
        hits.append(h)
        start.append(start[-1] + len(rows))
        status.append(res["status"].astype(np.uint8))
    T = len(per_target)
    P = len(per_target[0]) if T else 0
    return (np.concatenate(hits) if T else np.zeros(0, HIT_DTYPE), np.array(start, np.int32),
            np.stack(status) if T else np.zeros((0, P), np.uint8))


_reference_cache = {}


def reference(oracle, case, max_dist=TH_LOW):
    """(hits, hit_start, status) of the whole case by the restatement's projection and the oracle's window walk.  A case that
    carries a "name" is computed once per process and shared; the arrays are not to be written to."""
    key = (case.get("name"), max_dist)
    if case.get("name") is None or key not in _reference_cache:
        per = [oracle_target(oracle, case, k) for k in range(len(case["targets"]))]
        out = dense_from(per, max_dist)
        if case.get("name") is None:
            return out
        _reference_cache[key] = out
    return _reference_cache[key]


def reference_own(case, max_dist=TH_LOW):
    """the same by the restatement alone (its own grid and window walk)"""
    return dense_from([ref_target(case, k) for k in range(len(case["targets"]))], max_dist)


# ------------------------------------------------------------------------------------------------ scenes
def scw_of(rec, s):
    """a 4x4 float32 Scw = [s R | s t] whose decomposition is (about) the record's pose"""
    S = np.eye(4, dtype=f32)
    S[:3, :3] = (f64(s) * rec["Rcw"].astype(f64)).astype(f32)
    S[:3, 3] = (f64(s) * rec["tcw"].astype(f64)).astype(f32)
    return S


def with_pose(t, R, tc, Ow):
    rec = t["rec"].copy()
    rec["Rcw"], rec["tcw"], rec["Ow"] = np.asarray(R, f32).reshape(3, 3), np.asarray(tc, f32).reshape(3), np.asarray(Ow, f32).reshape(3)
    return dict(t, rec=rec)


# family -> (make_case's parameters, what is done to the targets afterwards)
FAMILIES = {
    "general": dict(),
    "behind_camera": dict(turn=2.6, spread=1.5),
    "outside_image": dict(spread=1.0),
    "distance_range": dict(distance_share=0.5),
    "view_angle": dict(normal_share=0.5),
    "level_range": dict(level_share=0.6),
    "crowded_ties": dict(ties=True),
    "mixed_intrinsics": dict(mixed=True),
    "repeated_target": dict(repeat=True),
    "scaled_sim3": dict(),
    "sparse_survivors": dict(),
}
FAMILY_CODES = {"behind_camera": FUSE_ST_DEPTH, "outside_image": FUSE_ST_OUTSIDE_IMAGE, "distance_range": FUSE_ST_DISTANCE,
                "view_angle": FUSE_ST_VIEW_ANGLE, "level_range": FUSE_ST_LEVEL_RANGE, "sparse_survivors": FUSE_ST_DEPTH}
# floors on the hits (best_dist <= TH_LOW) of a family over its five seeds, fixed after running the restatement alone on the
# CPU (measure()): the count (general 4104, behind_camera 630, outside_image 794, distance_range 2345, view_angle 5021,
# level_range 2627, crowded_ties 4522, mixed_intrinsics 6005, repeated_target 4302, scaled_sim3 5506, sparse_survivors 4536),
# rounded down to about a half.  sparse_survivors: 2.4 % of its pairs pass the gates.
HIT_FLOOR = {"general": 2000, "behind_camera": 300, "outside_image": 390, "distance_range": 1100, "view_angle": 2500, "level_range": 1300,
             "crowded_ties": 2200, "mixed_intrinsics": 3000, "repeated_target": 2100, "scaled_sim3": 2700, "sparse_survivors": 2200}
SPARSE_SHARE_CAP = 0.05       # sparse_survivors: the share of pairs that pass the gates


def make_dense(seed, name=None, th=TH, **kw):
    """fuse_cases.make_case's scene as a dense case: every point against every target, no job list, no chi-square"""
    case = make_case(seed, **kw)
    del case["jobs"], case["inv_sigma2"]
    case["th"] = th
    case["name"] = name
    return case


def family_case(name, seed):
    sd = 1000 * (sorted(FAMILIES).index(name) + 1) + seed
    case = make_dense(sd, name="%s/%d" % (name, seed), **FAMILIES[name])
    rng = np.random.default_rng(77000 + sd)
    if name == "scaled_sim3":       # Scw with scale 0.5 and 2.0 (and 1), decomposed by the caller as ORBmatcher.cc:987-992 does
        tg = []
        for k, t in enumerate(case["targets"]):
            R, tc, Ow = decompose_sim3(scw_of(t["rec"], (0.5, 2.0, 1.0)[k % 3]))
            tg.append(with_pose(t, R, tc, Ow))
        case["targets"] = tg
        case["scales"] = [(0.5, 2.0, 1.0)[k % 3] for k in range(len(tg))]
    if name == "sparse_survivors":  # a merge: most keyframes of the map look away from the loop points
        real = list(case["targets"])
        tg = list(real)
        for j in range(100):
            t = real[j % len(real)]
            turn = rot_axis_angle([0.1 * rng.normal(), 1.0, 0.1 * rng.normal()], rng.uniform(1.3, np.pi))
            R = turn @ t["rec"]["Rcw"].astype(f64)
            O = t["rec"]["Ow"].astype(f64) + rng.normal(size=3) * 0.3
            tg.insert(int(rng.integers(0, len(tg) + 1)), with_pose(t, R, -R @ O, O))
        case["targets"] = tg
    return case


# ------------------------------------------------------------------------------------------------ the float64 recount
def recount64(case, k, band=None):
    """the projection gates and the level in float64 from the same float32 inputs, every point against target k: (status,
    level, near, quantities): near marks the pairs with a gate quantity, up to the deciding gate, inside its band"""
    band = BAND if band is None else band
    rec, P = case["targets"][k]["rec"], case["points"]
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
        q = np.log(P["max_distance"].astype(f64) / dist) / np.log(f64(fc.SCALE_FACTOR))
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

    gate(pc[:, 2] < 0, np.abs(pc[:, 2]) <= band["z"] * npc, FUSE_ST_DEPTH)
    duv = np.minimum.reduce([np.abs(u - b[0]), np.abs(u - b[1]), np.abs(v - b[2]), np.abs(v - b[3])])
    gate(~((u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])), duv <= band["uv"], FUSE_ST_OUTSIDE_IMAGE)
    gate((dist < mn) | (dist > mx), (np.abs(dist - mn) <= band["dist"] * dist) | (np.abs(dist - mx) <= band["dist"] * dist), FUSE_ST_DISTANCE)
    gate(dot < 0.5 * dist, np.abs(dot - 0.5 * dist) <= band["dot"] * dist, FUSE_ST_VIEW_ANGLE)
    gate(~((lvl >= 0) & (lvl < case["nlevels"])), np.abs(q - np.rint(q)) <= band["level"], FUSE_ST_LEVEL_RANGE)
    near[~decided & (np.abs(q - np.rint(q)) <= band["level"])] = True
    return status, lvl, near, dict(pc=pc, npc=npc, u=u, v=v, dist=dist, dot=dot, q=q)


def check64(case, band=None):
    """against float64 over every pair: (decisions that disagree outside the bands, the share of pairs inside a band, pairs).
    A decision is the status up to LEVEL_RANGE and, for a pair that reaches the window, the level."""
    outside = inband = total = 0
    for k in range(len(case["targets"])):
        res, _ = ref_project(case, k)
        st64, lvl64, near, _ = recount64(case, k, band)
        differs = res["status"] != st64
        alive = (res["status"] == FUSE_ST_NO_CANDIDATE) & ~differs
        differs[alive] = res["level"][alive] != lvl64[alive]
        outside += int((differs & ~near).sum())
        inband += int(near.sum())
        total += len(res)
    return outside, (inband / total if total else 0.0), total


def gaps64(case):
    """per gate, the largest gap between the restatement's float quantity and its float64 recount over the pairs that reached it"""
    worst = dict(z=0.0, uv=0.0, dist=0.0, dot=0.0, level=0.0)
    for k in range(len(case["targets"])):
        res, g = ref_project(case, k, want_gates=True)
        _, _, _, w = recount64(case, k)
        worst["z"] = max(worst["z"], float(np.max(np.abs(g["z"].astype(f64) - w["pc"][:, 2]) / w["npc"])))
        r = res["status"] >= FUSE_ST_OUTSIDE_IMAGE
        inside = r & (np.abs(w["u"]) < 4 * fc.W) & (np.abs(w["v"]) < 4 * fc.H)      # (pixels far outside carry large absolute errors and decide nothing)
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
            qf = np.log(g["ratio"].astype(f32)[r]) / fc.LOG_SF       # the float quotient PredictScale rounds up
            worst["level"] = max(worst["level"], float(np.max(np.abs(qf.astype(f64) - w["q"][r]))))
    return worst


# ------------------------------------------------------------------------------------------------ the serial map model
class Model:
    """tools/loopfuse_ref.hpp's map model: keyframes, map points, observations, SearchAndFuse by the serial loop or the rule"""

    def __init__(self, sf=fc.SF, log_sf=fc.LOG_SF):
        self.L = ref_lib()
        sf = np.ascontiguousarray(sf, f32)
        self.h = self.L.loopref_model_new(_p(sf), len(sf), C.c_float(log_sf))
        self.n, self.n_points = [], 0

    def keyframe(self, grid, keys, desc):
        g = np.array(tuple(grid), dtype=GRID_DTYPE) if not isinstance(grid, np.ndarray) else np.ascontiguousarray(grid, dtype=GRID_DTYPE)
        keys, desc = np.ascontiguousarray(keys, dtype=KP_DTYPE), np.ascontiguousarray(desc, dtype=np.uint8)
        self.n.append(len(keys))
        return self.L.loopref_add_keyframe(self.h, _p(g), _p(keys), _p(desc), len(keys))

    def point(self, rec):
        rec = np.ascontiguousarray(rec, dtype=FUSE_POINT_DTYPE)
        self.n_points += 1
        return self.L.loopref_add_map_point(self.h, _p(rec))

    def observe(self, mp, kf, idx):
        self.L.loopref_add_observation(self.h, mp, kf, idx)

    def search_and_fuse(self, mode, kfs, recs, loop, th=TH):
        """mode 0: the serial loop, 1: the parallel rule, 2: the rule without the re-score.  (fused, events, rescored)"""
        kfs, loop = np.ascontiguousarray(kfs, np.int32), np.ascontiguousarray(loop, np.int32)
        recs = np.ascontiguousarray(recs, dtype=FUSE_TARGET_DTYPE)
        cap = 4 * len(kfs) * max(len(loop), 1) + 16
        events = np.zeros((cap, 4), np.int32)
        ne, rs = C.c_int(0), C.c_int64(0)
        fused = self.L.loopref_search_and_fuse(self.h, mode, _p(kfs), _p(recs), len(kfs), _p(loop), len(loop), C.c_float(th), _p(events), cap,
                                               C.byref(ne), C.byref(rs))
        assert ne.value <= cap
        return fused, [tuple(e) for e in events[:ne.value].tolist()], rs.value

    def slots(self, kf):
        out = np.zeros(max(self.n[kf], 1), np.int32)
        self.L.loopref_keyframe_slots(self.h, kf, _p(out))
        return out[:self.n[kf]].tolist()

    def map_point(self, mp):
        bad, rep = C.c_int(0), C.c_int(0)
        desc, obs = np.zeros(32, np.uint8), np.zeros((64, 2), np.int32)
        n = self.L.loopref_map_point(self.h, mp, C.byref(bad), C.byref(rep), _p(desc), _p(obs), 64)
        return bool(bad.value), rep.value, desc.tobytes(), [tuple(o) for o in obs[:n].tolist()]

    def state(self):
        """everything the serial part leaves behind: the slots of every keyframe and every point's record"""
        return [self.slots(k) for k in range(len(self.n))], [self.map_point(i) for i in range(self.n_points)]

    def close(self):
        self.L.loopref_model_free(self.h)


def map_scene(seed=0, case=None, targets=(6, 6), points=(400, 400), feats=400):
    """A loop closure as a map: the keyframes of a dense case are the corrected keyframes; every world point of the pool may be a
    LOOP point (observed by keyframes of the loop side, which are bystanders here and only lend descriptors), and in the
    corrected keyframes the same world point is another map point of the current side (a Replace), a free feature
    (AddObservation) or nothing.  The associations come from the restatement: a point belongs to the feature Fuse would pick
    for it.  Loop points that a Replace makes the survivor of get more observations and so, often, another descriptor, which
    is what the later targets then have to be searched with.  Returns a dict of flat arrays."""
    rng = np.random.default_rng(9500 + seed)
    if case is None:
        case = make_dense(9600 + seed, targets=targets, points=points, feats=feats, spread=0.05, turn=0.06, vis=0.9)
    # every corrected keyframe comes with an Scw of scale 0.5, 2 or 1, and is searched under the caller's decomposition of it
    scw = [scw_of(t["rec"], (0.5, 2.0, 1.0)[k % 3]) for k, t in enumerate(case["targets"])]
    case["targets"] = [with_pose(t, *decompose_sim3(S)) for t, S in zip(case["targets"], scw)]
    nk, pool = len(case["targets"]), case["points"]
    assoc = []
    for k in range(nk):
        res = ref_target(case, k)
        used, a = set(), {}
        for pi in np.flatnonzero((res["status"] == FUSE_ST_FOUND) & (res["best_dist"] <= 40)):
            if int(res["best_idx"][pi]) not in used:
                used.add(int(res["best_idx"][pi]))
                a[int(pi)] = int(res["best_idx"][pi])
        assoc.append(a)
    # a bystander keyframe of the loop side holds one feature per loop point, whose descriptor the loop point starts from: far
    # enough from the corrected keyframes' features (10 flips from the pool's) that its hits sit around TH_LOW, so that the
    # descriptor a Replace leaves (a corrected keyframe's, once the point has two observations there) finds what the old one missed
    by_desc = [fc.noisy_copies(rng, pool["desc"], 44)]
    points, obs, loop = [], [], []
    for pi in range(len(pool)):
        rec = pool[pi].copy()
        rec["desc"] = by_desc[0][pi]
        points.append(rec)
        loop.append(len(points) - 1)
        obs.extend((len(points) - 1, nk + b, pi) for b in range(len(by_desc)))
    for pi in range(len(pool)):      # the current side's own points of the same world points
        seen = [k for k in range(nk) if pi in assoc[k]]
        rng.shuffle(seen)
        while seen and rng.uniform() < 0.6:
            m = int(rng.integers(1, 3))
            take, seen = seen[:m], seen[m:]
            rec = pool[pi].copy()
            rec["desc"] = case["targets"][take[0]]["desc"][assoc[take[0]][pi]]
            points.append(rec)
            obs.extend((len(points) - 1, k, assoc[k][pi]) for k in sorted(take))
    by_keys = np.zeros(len(pool), dtype=KP_DTYPE)
    by_keys["x"], by_keys["y"], by_keys["octave"] = rng.uniform(1, 639, len(pool)), rng.uniform(1, 479, len(pool)), 0
    bystanders = [dict(rec=case["targets"][0]["rec"], keys=by_keys, desc=d) for d in by_desc]
    return dict(case=case, scw=np.array(scw, f32), bystanders=bystanders, points=np.array(points, dtype=FUSE_POINT_DTYPE), obs=np.array(obs, np.int32).reshape(-1, 3),
                loop=np.array(rng.permutation(loop), np.int32))


def load_model(scene):
    """the scene as a Model; keyframe ids are the scene's (corrected keyframes first, then the bystanders)"""
    m = Model(scene["case"]["sf"], scene["case"]["log_sf"])
    for t in scene["case"]["targets"] + scene["bystanders"]:
        m.keyframe(t["rec"]["grid"], t["keys"], t["desc"])
    for rec in scene["points"]:
        m.point(rec)
    for mp, kf, idx in scene["obs"].tolist():
        m.observe(mp, kf, idx)
    return m


def write_map_scene(scene, path):
    """the scene as the flat file tests/cpp/loopfuse_dropin_gpu.cpp reads: the counts, the scale factors and the log scale
    factor, the corrected keyframes' Scw, every keyframe as (record, n, keys, descriptors), the map points' records, the observations, the loop points"""
    case = scene["case"]
    kfs = case["targets"] + scene["bystanders"]
    with open(path, "wb") as f:
        np.array([len(kfs), len(case["targets"]), len(scene["points"]), len(scene["obs"]), len(scene["loop"])], np.int32).tofile(f)
        case["sf"][:8].astype(f32).tofile(f)
        np.array([case["log_sf"], case["th"]], f32).tofile(f)
        np.ascontiguousarray(scene["scw"], dtype=f32).tofile(f)          # (4 x 4 each, for the corrected keyframes)
        for t in kfs:
            np.ascontiguousarray(t["rec"], dtype=FUSE_TARGET_DTYPE).tofile(f)
            np.array([len(t["keys"])], np.int32).tofile(f)
            np.ascontiguousarray(t["keys"], dtype=KP_DTYPE).tofile(f)
            np.ascontiguousarray(t["desc"], dtype=np.uint8).tofile(f)
        np.ascontiguousarray(scene["points"], dtype=FUSE_POINT_DTYPE).tofile(f)
        np.ascontiguousarray(scene["obs"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(scene["loop"], dtype=np.int32).tofile(f)


def measure():
    """prints what the constants at the top of this file were taken from"""
    worst_gap = {kind: (0.0, "") for kind in MEASURED}
    gaps_by_case = {}
    for name in sorted(FAMILIES):
        for seed in SEEDS:
            case = family_case(name, seed)
            gap = gaps64(case)
            gaps_by_case[(name, seed)] = gap
            worst_gap = {kind: max(worst_gap[kind], (gap[kind], name)) for kind in MEASURED}
    band = {k: 4 * v[0] for k, v in worst_gap.items()}
    print("gate gaps", worst_gap)
    for name in sorted(FAMILIES):
        hits_total, worst_share, passing, pairs = 0, 0.0, 0, 0
        for seed in SEEDS:
            case = family_case(name, seed)
            hits, start, status = reference_own(case)
            outside, share, total = check64(case, band)
            counts = np.bincount(status.reshape(-1), minlength=7)
            hits_total += len(hits)
            passing += int(counts[FUSE_ST_NO_CANDIDATE] + counts[FUSE_ST_FOUND])
            pairs += total
            worst_share = max(worst_share, share)
            print("%-18s seed %d  targets %3d  pairs %6d  codes %s  hits %5d  outside %d  share %.5f" %
                  (name, seed, len(case["targets"]), total, counts.tolist(), len(hits), outside, share))
        print("%-18s hits over the seeds: %d   worst in-band share %.5f   pass share %.4f" % (name, hits_total, worst_share, passing / pairs))


if __name__ == "__main__":
    measure()
