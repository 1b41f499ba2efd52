"""CreateNewMapPoints' checker for the tests: the C++ restatement (tools/newpoints_ref.hpp) built with g++
-ffp-contract=off behind a small C shim (tests/cpp/newpoints_ref_capi.cpp), seeded scene families with real geometry, the
SERIAL reference loop over the oracle's SearchForTriangulation and the restatement, and a float64 numpy check that shares
no code with the restatement."""
import ctypes as C
import functools

import numpy as np

from matcher_cases import noisy_copies
from ref_shim import cached_shim, p as _p, rot_axis_angle as _rot, same
from orbslamm_amd._lib import KP_DTYPE
from orbslamm_amd.local_mapping import (KF_DTYPE, NEWPOINT_DTYPE, ST_ACCEPTED, ST_DIST_ZERO, ST_FEATURE_SKIPPED, ST_NEIGHBOUR_SKIPPED,
                                        ST_NO_MATCH, ST_PARALLAX, ST_REPROJ1, ST_REPROJ2, ST_SCALE, ST_X3D_ZERO, ST_Z1, ST_Z2, keyframe)

rot_axis_angle = functools.partial(_rot, scale_first=True)   # (how this module's scenes were generated: ref_shim.rot_axis_angle)

f32, f64 = np.float32, np.float64
W, H = 640.0, 480.0
K_A = np.array([517.3, 516.5, 318.6, 255.3], dtype=f32)
K_B = np.array([458.7, 457.3, 367.2, 248.4], dtype=f32)     # (mixed_intrinsics: a neighbour from another camera)
NLEVELS = 8
SCALE_FACTOR = f32(1.2)
SF = np.array([SCALE_FACTOR ** l for l in range(NLEVELS)], dtype=f32)
SIGMA2 = (SF * SF).astype(f32)

# Tolerances of the float64 check, MEASURED from the restatement on the CPU over seeds 0..4 of every family (see measure()
# below, `PYTHONPATH=. python tests/newpoints_cases.py`), then given the margin of 4x this project uses for their
# dependence on conditioning (pnp_cases.py, sim3_cases.py):
#   |pos - X64| / |X64| of an accepted point against numpy's float64 SVD of the same pair
#                                                      measured max 9.46e-6   (wrong_matches; the float Jacobi SVD of the 4x4)
#   the float32 rounding band of each gate's quantity against its float64 recount, relative to the gate's scale:
#     cosParallaxRays (absolute)                       measured max 9.04e-8   (wrong_matches)
#     z1, z2 relative to |x3D|                         measured max 9.51e-6   (wrong_matches)
#     squared reprojection error relative to its threshold, over pairs below 4 thresholds
#                                                      measured max 7.94e-5   (wrong_matches; the error follows x3D)
#     ratioDist relative to itself                     measured max 2.41e-6   (wrong_matches)
# Outside the bands no gate decision of those runs disagreed with the float64 recount; the largest share of a case's
# triangulated pairs inside a band was 0.0010 (low_parallax, whose cosines crowd 0.9998 by design): the 2 % cap (a condition,
# not a measurement) holds for every family and seed used, with the noise levels below.
TOL_POS = 4 * 9.46e-6
BAND = dict(cos=4 * 9.04e-8, z=4 * 9.51e-6, e=4 * 7.94e-5, ratio=4 * 2.41e-6)
BAND_SHARE_CAP = 0.02   # the share of a case's triangulated pairs that may fall inside the band (undecided)
SEEDS = range(5)        # the seeds measured; the tests use these

def _declare(L):
    vp = C.c_void_p
    L.npref_compute_f12.argtypes = [vp, vp, vp, vp]
    L.npref_compute_f12.restype = None
    L.npref_baseline_too_short.argtypes = [vp, vp]
    L.npref_pair.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, vp, vp]
    L.npref_neighbour.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_float, vp, vp]
    assert (L.npref_sizes(0), L.npref_sizes(1), L.npref_sizes(2)) == (KF_DTYPE.itemsize, NEWPOINT_DTYPE.itemsize, KP_DTYPE.itemsize)


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("newpoints_ref", _declare)


def ref_f12(kf1, kf2):
    a, b = np.ascontiguousarray(kf1, dtype=KF_DTYPE), np.ascontiguousarray(kf2, dtype=KF_DTYPE)
    F, e = np.zeros((3, 3), f32), np.zeros(2, f32)
    ref_lib().npref_compute_f12(_p(a), _p(b), _p(F), _p(e))
    return F, e


def ref_gated(kf1, kf2):
    a, b = np.ascontiguousarray(kf1, dtype=KF_DTYPE), np.ascontiguousarray(kf2, dtype=KF_DTYPE)
    return bool(ref_lib().npref_baseline_too_short(_p(a), _p(b)))


def ref_pair(case, k, q, t):
    """the restatement's per-pair function: (status, point record, the gates' float quantities)"""
    a, b = np.ascontiguousarray(case["cur"]["kf"], dtype=KF_DTYPE), np.ascontiguousarray(case["nbs"][k]["kf"], dtype=KF_DTYPE)
    kp1, kp2 = case["cur"]["keys"][q:q + 1].copy(), case["nbs"][k]["keys"][t:t + 1].copy()
    out = np.zeros(1, dtype=NEWPOINT_DTYPE)
    dbg = np.full(9, np.nan, f32)
    st = ref_lib().npref_pair(_p(a), _p(b), _p(kp1), _p(kp2), _p(case["sf"]), _p(case["sigma2"]), len(case["sf"]), C.c_float(case["scale_factor"]),
                              _p(out), _p(dbg))
    out["neighbour"], out["idx1"], out["idx2"] = k, q, t
    return st, out[0], dbg


# ------------------------------------------------------------------------------------------------ the two reference loops
def _search(oracle, case, k, skip1):
    """SearchForTriangulation(current, neighbour k) of the oracle under the given skip1, with the restatement's F12"""
    cur, nb = case["cur"], case["nbs"][k]
    F, e = ref_f12(cur["kf"], nb["kf"])
    if len(cur["keys"]) == 0 or len(nb["keys"]) == 0:
        return np.full(len(cur["keys"]), -1, np.int32), F, e
    m12, _ = oracle.search_for_triangulation(cur["keys"], cur["desc"], skip1, cur["fv"], nb["keys"], nb["desc"], nb["skip"], nb["fv"],
                                             F, float(e[0]), float(e[1]), case["sf"], case["sigma2"], False, False)
    return m12.astype(np.int32), F, e


def serial_reference(oracle, case):
    """The reference's loop, one neighbour after the other: search under the CURRENT skip1, triangulate its pairs, fold the
    successes into skip1.  Returns (points, status table, f12 table, match table)."""
    cur, K = case["cur"], len(case["nbs"])
    n1 = len(cur["keys"])
    skip1 = np.zeros(n1, np.uint8) if cur["skip"] is None else np.ascontiguousarray(cur["skip"], dtype=np.uint8).copy()
    pts = np.zeros(0, dtype=NEWPOINT_DTYPE)
    status, f12, m12s = np.zeros((K, n1), np.uint8), np.zeros((K, 11), f32), np.full((K, n1), -1, np.int32)
    kf1 = np.ascontiguousarray(cur["kf"], dtype=KF_DTYPE)
    for k, nb in enumerate(case["nbs"]):
        kf2 = np.ascontiguousarray(nb["kf"], dtype=KF_DTYPE)
        m12 = None
        if not ref_gated(kf1, kf2):
            m12, F, e = _search(oracle, case, k, skip1)
            f12[k, :9], f12[k, 9:] = F.reshape(9), e
            m12s[k] = m12
        out = np.zeros(max(n1, 1), dtype=NEWPOINT_DTYPE)
        n = ref_lib().npref_neighbour(k, _p(kf1), _p(kf2), _p(cur["keys"]), n1, _p(nb["keys"]), _p(m12), _p(skip1), _p(case["sf"]),
                                      _p(case["sigma2"]), len(case["sf"]), C.c_float(case["scale_factor"]), _p(out), _p(status[k]))
        pts = np.concatenate([pts, out[:n]])
    return pts, status, f12, m12s


def resolved_reference(oracle, case):
    """the batch's form, re-implemented on the test side over the restatement's per-pair function: every neighbour
    independently under the INITIAL skip1, then per feature the first accepting neighbour wins and later ones read
    "feature skipped"; the points in (neighbour, idx1) order"""
    cur, K = case["cur"], len(case["nbs"])
    n1 = len(cur["keys"])
    skip1 = np.zeros(n1, np.uint8) if cur["skip"] is None else np.ascontiguousarray(cur["skip"], dtype=np.uint8)
    status = np.zeros((K, n1), np.uint8)
    recs = {}
    for k, nb in enumerate(case["nbs"]):
        if ref_gated(cur["kf"], nb["kf"]):
            status[k] = ST_NEIGHBOUR_SKIPPED
            continue
        m12, _, _ = _search(oracle, case, k, skip1)
        for q in range(n1):
            if skip1[q]:
                status[k, q] = ST_FEATURE_SKIPPED
            elif m12[q] < 0:
                status[k, q] = ST_NO_MATCH
            else:
                status[k, q], rec, _ = ref_pair(case, k, q, int(m12[q]))
                recs[(k, q)] = rec
    raw = status.copy()
    for q in range(n1):
        taken = False
        for k in range(K):
            if taken and status[k, q] != ST_NEIGHBOUR_SKIPPED:
                status[k, q] = ST_FEATURE_SKIPPED
            elif status[k, q] == ST_ACCEPTED:
                taken = True
    keep = [recs[(k, q)] for k in range(K) for q in range(n1) if status[k, q] == ST_ACCEPTED]
    pts = np.array(keep, dtype=NEWPOINT_DTYPE) if keep else np.zeros(0, dtype=NEWPOINT_DTYPE)
    return pts, status, raw


# ------------------------------------------------------------------------------------------------ scenes
def _featvec(nodes):
    """mFeatVec as CSR: node ids ascending, the features of a node in index order"""
    nodes = np.asarray(nodes, np.int64)
    ids = np.unique(nodes)
    order = np.argsort(nodes, kind="stable")
    counts = np.array([(nodes == i).sum() for i in ids], np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ids.astype(np.uint32), start, order.astype(np.int32)


def _project(R, Ow, K, X):
    Xc = (X - Ow) @ R.T
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = K[0] * Xc[:, 0] / z + K[2], K[1] * Xc[:, 1] / z + K[3]
    return u, v, z


def _camera(rng, R, Ow, K, X, pid, octave, base_desc, nnodes, noise, flips, n_clutter, skip_share, mirrored=None):
    """one keyframe's features: the points `pid` of X seen through (R, Ow, K) with pixel noise of `noise` * the level's
    scale, plus clutter.  mirrored: points that may lie behind the camera (their projection is kept: wrong_matches)."""
    u, v, z = _project(R, Ow, K.astype(f64), X)
    sc = SF.astype(f64)[octave]
    u = u + rng.normal(0, noise, len(u)) * sc
    v = v + rng.normal(0, noise, len(v)) * sc
    ok = (u >= 1) & (u < W - 1) & (v >= 1) & (v < H - 1) & np.isfinite(u) & np.isfinite(v)
    ok &= (z > 0.05) if mirrored is None else ((z > 0.05) | mirrored)
    sel = np.flatnonzero(ok)
    n = len(sel) + n_clutter
    keys = np.zeros(n, dtype=KP_DTYPE)
    keys["x"][:len(sel)], keys["y"][:len(sel)], keys["octave"][:len(sel)] = u[sel], v[sel], octave[sel]
    keys["x"][len(sel):], keys["y"][len(sel):] = rng.uniform(1, W - 1, n_clutter), rng.uniform(1, H - 1, n_clutter)
    keys["octave"][len(sel):] = rng.integers(0, NLEVELS, n_clutter)
    keys["size"], keys["angle"], keys["response"], keys["class_id"] = 31.0 * SF[keys["octave"]], rng.uniform(0, 360, n), 50.0, -1
    desc = np.concatenate([noisy_copies(rng, base_desc[sel], flips), rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
    nodes = np.concatenate([pid[sel] % nnodes, rng.integers(0, nnodes, n_clutter)])
    point = np.concatenate([pid[sel], np.full(n_clutter, -1)])
    perm = rng.permutation(n)
    keys, desc, nodes, point = keys[perm], np.ascontiguousarray(desc[perm]), nodes[perm], point[perm]
    skip = (rng.uniform(size=n) < skip_share).astype(np.uint8) if skip_share > 0 else None
    return dict(keys=keys, desc=desc, fv=_featvec(nodes), skip=skip, point=point)


# family -> parameters.  n: points; nb: neighbours as (offset of the centre from the current one in units of the median
# depth, rotation angle, K, kind); depth: the cloud's range; noise: sigma of the pixel noise at level 0; vis: the chance that a
# neighbour sees a point; skip1 / skip2: the share of features that already hold a map point
_SIDE = [((0.10, 0.02, 0.01), 0.03), ((-0.12, 0.03, 0.02), 0.04), ((0.18, -0.04, 0.03), 0.05), ((-0.07, 0.09, -0.02), 0.02),
         ((0.25, 0.01, -0.03), 0.06), ((-0.2, -0.08, 0.04), 0.05)]
FAMILIES = {
    "general": dict(n=900, nb=[(o, a, K_A, "true") for o, a in _SIDE], depth=(4, 9), noise=0.25, vis=0.45, skip1=0.2, skip2=0.2),
    "repeat_features": dict(n=500, nb=[(o, a, K_A, "true") for o, a in _SIDE[:5]], depth=(4, 9), noise=0.15, vis=0.95, skip1=0.0, skip2=0.0),
    "short_baseline": dict(n=400, nb=[((0.004, 0.001, 0.0), 0.01, K_A, "true"), (_SIDE[0][0], 0.03, K_A, "true"), (_SIDE[1][0], 0.04, K_A, "nodepth"),
                                      ((0.0, 0.0, 0.0095), 0.02, K_A, "true"), (_SIDE[2][0], 0.05, K_A, "true")],
                           depth=(4, 9), noise=0.25, vis=0.7, skip1=0.1, skip2=0.1),
    "low_parallax": dict(n=500, nb=[((0.013, 0.002, 0.0), 0.02, K_A, "true"), ((-0.012, 0.004, 0.001), 0.03, K_A, "true"),
                                    ((0.03, -0.003, 0.0), 0.02, K_A, "true"), ((0.002, 0.015, -0.001), 0.01, K_A, "true")],
                         depth=(40, 60), noise=0.25, vis=0.7, skip1=0.1, skip2=0.1),
    "wrong_matches": dict(n=600, nb=[(_SIDE[2][0], 0.05, K_A, "coarse"), (_SIDE[0][0], 0.03, K_A, "twin"), ((0.02, 0.01, 0.45), 0.02, K_A, "ahead"),
                                     ((-0.02, 0.01, -0.45), 0.02, K_A, "behind")], depth=(4, 9), noise=0.2, vis=0.8, skip1=0.05, skip2=0.05),
    "scale_inconsistent": dict(n=500, nb=[(o, a, K_A, "octaves") for o, a in _SIDE[:4]], depth=(4, 9), noise=0.25, vis=0.7, skip1=0.1, skip2=0.1),
    "already_mapped": dict(n=600, nb=[(o, a, K_A, "true") for o, a in _SIDE[:5]], depth=(4, 9), noise=0.25, vis=0.7, skip1=0.85, skip2=0.8),
    "mixed_intrinsics": dict(n=600, nb=[(o, a, K_B if i % 2 == 0 else K_A, "true") for i, (o, a) in enumerate(_SIDE)], depth=(4, 9), noise=0.25,
                             vis=0.6, skip1=0.15, skip2=0.15),
}
EMPTY_KINDS = ("no_neighbours", "no_features", "no_neighbour_features", "disjoint_nodes")


def make_case(seed, n, nb, depth, noise, vis, skip1, skip2, depth_unit=None, nnodes=None, clutter=0.25, flips=8):
    rng = np.random.default_rng(seed)
    K1 = K_A.astype(f64)
    # the cloud in front of the current keyframe, which sits at a generic pose
    z = rng.uniform(depth[0], depth[1], n)
    X1 = np.stack([(rng.uniform(20, W - 20, n) - K1[2]) / K1[0] * z, (rng.uniform(20, H - 20, n) - K1[3]) / K1[1] * z, z], axis=1)
    R1 = rot_axis_angle(rng.normal(size=3), 0.3)
    Ow1 = rng.normal(size=3) * 2.0
    X = X1 @ R1 + Ow1                       # world points: Xc = R (X - Ow)
    unit = float(np.median(z)) if depth_unit is None else depth_unit
    nnodes = nnodes or max(1, n // 12)
    pid = np.arange(n)
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    o1 = rng.integers(1, 5, n)             # the current keyframe's level of every point
    dist1 = np.linalg.norm(X - Ow1, axis=1)
    nclut = int(clutter * n)
    cur = _camera(rng, R1, Ow1, K_A, X, pid, o1, base, nnodes, noise, flips, nclut, skip1)
    cur["kf"] = keyframe(R1, -R1 @ Ow1, Ow1, K_A)
    nbs = []
    for off, ang, K2, kind in nb:
        R2 = rot_axis_angle(rng.normal(size=3), ang) @ R1
        Ow2 = Ow1 + (np.asarray(off, f64) * unit) @ R1          # the offset in the current camera's axes
        seen = rng.uniform(size=n) < vis
        Xk, mirrored = X.copy(), None
        ray = X - Ow1
        if kind == "twin":        # a descriptor twin further along (or short of) the current keyframe's ray: on the epipolar line
            lam = rng.choice([0.12, 0.3, 3.5, 9.0], n)
            tw = rng.uniform(size=n) < 0.5
            Xk[tw] = Ow1 + ray[tw] * lam[tw, None]
        elif kind == "ahead":     # the neighbour has moved past near points: their mirrored projection triangulates behind it
            tw = rng.uniform(size=n) < 0.6
            Xk[tw] = Ow1 + ray[tw] * rng.uniform(0.08, 0.4, n)[tw, None]
            mirrored = tw
        elif kind == "behind":    # the twin lies behind the current keyframe, in front of a neighbour that has moved back
            tw = rng.uniform(size=n) < 0.6
            Xk[tw] = Ow1 - ray[tw] * rng.uniform(0.05, 0.35, n)[tw, None]
        dist2 = np.linalg.norm(Xk - Ow2, axis=1)
        o2 = np.clip(np.rint(o1 - np.log(dist2 / dist1) / np.log(1.2)), 0, NLEVELS - 1).astype(np.int64)
        nz = noise
        if kind == "octaves":     # levels unrelated to distance: the scale-ratio gate
            o2 = rng.integers(0, NLEVELS, n)
        elif kind == "coarse":    # coarse partners of fine features: the search's gate is the partner's sigma, the first reprojection gate is not
            o2 = np.full(n, NLEVELS - 1)
            nz = 1.6
        c = _camera(rng, R2, Ow2, K2, Xk[seen], pid[seen], o2[seen], base[seen], nnodes, nz, flips, nclut, skip2,
                    None if mirrored is None else mirrored[seen])
        zc = ((X - Ow2) @ R2.T)[:, 2]
        md = -1.0 if kind == "nodepth" else float(np.median(zc))      # ComputeSceneMedianDepth(2); -1: no map points (KeyFrame.cc:656)
        c["kf"] = keyframe(R2, -R2 @ Ow2, Ow2, K2, md)
        nbs.append(c)
    return dict(cur=cur, nbs=nbs, sf=SF.copy(), sigma2=SIGMA2.copy(), scale_factor=float(SCALE_FACTOR))


def family_case(name, seed):
    return make_case(1000 * (sorted(FAMILIES).index(name) + 1) + seed, **FAMILIES[name])


def empty_case(kind, seed=0):
    """zero neighbours, zero features, a neighbour without features, or keyframes that share no vocabulary node"""
    c = make_case(77 + seed, n=60, nb=[(o, a, K_A, "true") for o, a in _SIDE[:2]], depth=(4, 9), noise=0.2, vis=0.8, skip1=0.1, skip2=0.1)
    def strip(side):
        side.update(keys=side["keys"][:0], desc=side["desc"][:0], fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32)),
                    skip=None if side["skip"] is None else side["skip"][:0])
    if kind == "no_neighbours":
        c["nbs"] = []
    elif kind == "no_features":
        strip(c["cur"])
    elif kind == "no_neighbour_features":
        strip(c["nbs"][0])
    elif kind == "disjoint_nodes":
        for nb in c["nbs"]:
            nb["fv"] = ((nb["fv"][0] + 100000).astype(np.uint32), nb["fv"][1], nb["fv"][2])
    else:
        raise KeyError(kind)
    return c


def degenerate_case():
    """Hand-made pairs for the gates that consistent geometry never reaches: the entries take Rcw, tcw and Ow as the caller
    gives them, so a keyframe record need not be a rigid pose.
      neighbour 0  x3D(3) == 0: a sheared Rcw2 whose third column is (a, 0, 1) makes A's third column exactly zero for the
                   pair ((cx, cy), (cx + a fx, cy)) with fx a power of two, while the rays (through the TRANSPOSE) keep parallax
      neighbour 1  reprojection 2: the epipolar line comes from R1w*R2w.t(), the triangulation from the rows of Rcw2: under a
                   shear they disagree, and a fine-level partner on the line reprojects off its key
      neighbour 2  dist == 0: Ow2 is the very x3D the pair triangulates to (x3D does not depend on Ow2)
    The sigma of level 7 is made huge so that the crafted current features pass the search's and the first gates."""
    K = np.array([512.0, 512.0, 320.0, 240.0], f32)
    sf, sigma2 = SF.copy(), SIGMA2.copy()
    sigma2[7] = f32(1.0e9)
    rng = np.random.default_rng(5)
    eye = np.eye(3)
    kf1 = keyframe(eye, np.zeros(3), np.zeros(3), K)
    n1 = 3
    keys1 = np.zeros(n1, dtype=KP_DTYPE)
    keys1["size"], keys1["response"], keys1["class_id"] = 31.0, 50.0, -1
    desc1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    fv1 = _featvec([0, 1, 2])
    nbs = []

    def nb_of(kf, key_xy, octave, d):
        k = np.zeros(1, dtype=KP_DTYPE)
        k["x"], k["y"], k["octave"], k["size"], k["response"], k["class_id"] = key_xy[0], key_xy[1], octave, 31.0, 50.0, -1
        return dict(keys=k, desc=d.reshape(1, 32).copy(), fv=None, skip=None, kf=kf)
    # neighbour 0
    a = 0.5
    R2 = np.array([[1, 0, a], [0, 1, 0], [0, 0, 1]], f64)
    keys1["x"][0], keys1["y"][0], keys1["octave"][0] = 320.0, 240.0, 7
    nb0 = nb_of(keyframe(R2, [0.3, 0.2, 0.1], [1.0, 0.5, 0.0], K, 1.0), (320.0 + a * 512.0, 240.0), 7, desc1[0])
    nb0["fv"] = _featvec([0])
    nbs.append(nb0)
    # neighbour 1: filled below by a seeded search over shears
    keys1["x"][1], keys1["y"][1], keys1["octave"][1] = 250.0, 200.0, 7
    nbs.append(None)
    # neighbour 2
    keys1["x"][2], keys1["y"][2], keys1["octave"][2] = 400.0, 300.0, 2
    Rn = rot_axis_angle([0.2, 1.0, 0.1], 0.05)
    On = np.array([0.6, 0.05, 0.02])
    Xp = np.array([(400.0 - 320.0) / 512.0 * 5.0, (300.0 - 240.0) / 512.0 * 5.0, 5.0])
    u2, v2, _ = _project(Rn, On, K.astype(f64), Xp[None])
    nb2 = nb_of(keyframe(Rn, -Rn @ On, On, K, 5.0), (u2[0], v2[0]), 2, desc1[2])
    nb2["fv"] = _featvec([2])
    nbs.append(nb2)
    case = dict(cur=dict(keys=keys1, desc=desc1, fv=fv1, skip=None, kf=kf1), nbs=nbs, sf=sf, sigma2=sigma2, scale_factor=float(SCALE_FACTOR))
    # neighbour 1: a shear and a partner ON the line F12 gives (so the search takes it) whose pair ends at the second
    # reprojection gate; the first that does, in a fixed seeded order
    found = None
    for trial in range(4000):
        sh = np.eye(3) + rng.uniform(-0.25, 0.25, (3, 3))
        O2 = np.array([0.5, 0.0, 0.0]) + rng.uniform(-0.1, 0.1, 3)
        kf = keyframe(sh, -sh @ O2, O2, K, 5.0)
        F, e = ref_f12(kf1, kf)
        l = np.array([250.0, 200.0, 1.0]) @ F.astype(f64)
        if abs(l[1]) < 1e-12:
            continue
        x = rng.uniform(100, 540)
        y = -(l[0] * x + l[2]) / l[1]
        if not (20 < y < 460) or (x - e[0]) ** 2 + (y - e[1]) ** 2 < 400:
            continue
        nbs[1] = nb_of(kf, (x, y), 0, desc1[1])
        nbs[1]["fv"] = _featvec([1])
        if ref_pair(case, 1, 1, 0)[0] == ST_REPROJ2:
            found = trial
            break
    assert found is not None, "no sheared neighbour reached the second reprojection gate"
    # neighbour 2's centre becomes the point its pair triangulates to
    st, rec, _ = ref_pair(case, 2, 2, 0)
    assert st == ST_ACCEPTED, st
    nb2["kf"]["Ow"] = rec["pos"]
    return case


def write_scene(case, path):
    """the case as the flat file tests/cpp/newpoints_dropin_gpu.cpp reads: K, the two level tables, then the current keyframe
    and every neighbour as (n, keys, descriptors, skip flags, the feature vector as CSR, the keyframe record)"""
    with open(path, "wb") as f:
        np.array([len(case["nbs"])], np.int32).tofile(f)
        case["sf"][:8].astype(f32).tofile(f)
        case["sigma2"][:8].astype(f32).tofile(f)
        for side in [case["cur"]] + case["nbs"]:
            n = len(side["keys"])
            np.array([n], np.int32).tofile(f)
            np.ascontiguousarray(side["keys"], dtype=KP_DTYPE).tofile(f)
            np.ascontiguousarray(side["desc"], dtype=np.uint8).tofile(f)
            (np.zeros(n, np.uint8) if side["skip"] is None else np.ascontiguousarray(side["skip"], dtype=np.uint8)).tofile(f)
            node, start, idx = side["fv"]
            np.array([len(node)], np.int32).tofile(f)
            node.astype(np.uint32).tofile(f)
            start.astype(np.int32).tofile(f)
            idx.astype(np.int32).tofile(f)
            np.ascontiguousarray(side["kf"], dtype=KF_DTYPE).tofile(f)


# ------------------------------------------------------------------------------------------------ the float64 check
def pair64(case, k, q, t):
    """the pair in float64 from the same float32 inputs: numpy's SVD for the linear triangulation, the gates' quantities"""
    a, b = case["cur"]["kf"], case["nbs"][k]["kf"]
    kp1, kp2 = case["cur"]["keys"][q], case["nbs"][k]["keys"][t]
    out = {}
    Rs, ts, Ks, Os = [], [], [], []
    for kf in (a, b):
        Rs.append(np.asarray(kf["Rcw"], f64).reshape(3, 3)); ts.append(np.asarray(kf["tcw"], f64).reshape(3))
        Ks.append(np.asarray(kf["K"], f64).reshape(4)); Os.append(np.asarray(kf["Ow"], f64).reshape(3))
    xn = [np.array([(f64(kp["x"]) - Kc[2]) / Kc[0], (f64(kp["y"]) - Kc[3]) / Kc[1], 1.0]) for kp, Kc in ((kp1, Ks[0]), (kp2, Ks[1]))]
    rays = [Rs[i].T @ xn[i] for i in range(2)]
    out["cos"] = float(rays[0] @ rays[1] / (np.linalg.norm(rays[0]) * np.linalg.norm(rays[1])))
    T = [np.concatenate([Rs[i], ts[i][:, None]], axis=1) for i in range(2)]
    A = np.stack([xn[0][0] * T[0][2] - T[0][0], xn[0][1] * T[0][2] - T[0][1], xn[1][0] * T[1][2] - T[1][0], xn[1][1] * T[1][2] - T[1][1]])
    v = np.linalg.svd(A)[2][3]
    out["w"] = float(v[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        X = v[:3] / v[3]
    out["X"] = X
    for i in range(2):
        Xc = Rs[i] @ X + ts[i]
        out["z%d" % (i + 1)] = float(Xc[2])
        kp = (kp1, kp2)[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, vv = Ks[i][0] * Xc[0] / Xc[2] + Ks[i][2], Ks[i][1] * Xc[1] / Xc[2] + Ks[i][3]
        out["e%d" % (i + 1)] = float((u - f64(kp["x"])) ** 2 + (vv - f64(kp["y"])) ** 2)
        out["th%d" % (i + 1)] = 5.991 * float(f64(case["sigma2"][int(kp["octave"]) & 15]))
        out["d%d" % (i + 1)] = float(np.linalg.norm(X - Os[i]))
    out["ratio"] = out["d2"] / out["d1"] if out["d1"] else np.inf
    out["ro"] = float(f64(case["sf"][int(kp1["octave"]) & 15]) / f64(case["sf"][int(kp2["octave"]) & 15]))
    out["rf"] = 1.5 * float(case["scale_factor"])
    return out


def status64(g, band):
    """(the float64 recount's status, whether a gate up to the deciding one lies inside its relative band)"""
    near = False
    def close(x, th, scale, kind):
        return abs(x - th) <= band[kind] * scale
    near |= close(g["cos"], 0.0, 1.0, "cos") or close(g["cos"], 0.9998, 1.0, "cos")
    if not (g["cos"] > 0 and g["cos"] < 0.9998):
        return ST_PARALLAX, near
    if g["w"] == 0:
        return ST_X3D_ZERO, near
    nX = float(np.linalg.norm(g["X"]))
    for i, st in ((1, ST_Z1), (2, ST_Z2)):
        near |= close(g["z%d" % i], 0.0, nX, "z")
        if g["z%d" % i] <= 0:
            return st, near
    for i, st in ((1, ST_REPROJ1), (2, ST_REPROJ2)):
        near |= close(g["e%d" % i], g["th%d" % i], g["th%d" % i], "e")
        if g["e%d" % i] > g["th%d" % i]:
            return st, near
    if g["d1"] == 0 or g["d2"] == 0:
        return ST_DIST_ZERO, near
    near |= close(g["ratio"] * g["rf"], g["ro"], g["ro"], "ratio") or close(g["ratio"], g["ro"] * g["rf"], g["ro"] * g["rf"], "ratio")
    if g["ratio"] * g["rf"] < g["ro"] or g["ratio"] > g["ro"] * g["rf"]:
        return ST_SCALE, near
    return ST_ACCEPTED, near


def check64(case, pts, status, m12s, band=None):
    """Against float64: (largest relative position error of an accepted point, gate decisions that disagree outside the
    band, the share of triangulated pairs inside the band, triangulated pairs).  status / m12s: the serial reference's tables
    ("feature skipped" rows hold no pair)."""
    band = BAND if band is None else band
    pos = {(int(r["neighbour"]), int(r["idx1"])): r for r in pts}
    worst, outside, inband, total = 0.0, 0, 0, 0
    for k in range(status.shape[0]):
        for q in np.flatnonzero(status[k] >= ST_PARALLAX):
            g = pair64(case, k, int(q), int(m12s[k, q]))
            s64, near = status64(g, band)
            total += 1
            inband += bool(near)
            if s64 != status[k, q] and not near:
                outside += 1
            if status[k, q] == ST_ACCEPTED and s64 == ST_ACCEPTED:
                worst = max(worst, float(np.linalg.norm(pos[(k, int(q))]["pos"].astype(f64) - g["X"]) / np.linalg.norm(g["X"])))
    return worst, outside, (inband / total if total else 0.0), total


def gate_discrepancy(case, k, q, t):
    """per gate kind, the largest relative gap between a gate quantity of the restatement (float) and its float64 recount,
    over the gates both sides reached: what BAND is measured from"""
    st, _, dbg = ref_pair(case, k, q, t)
    g = pair64(case, k, q, t)
    gaps = dict(cos=abs(float(dbg[0]) - g["cos"]), z=0.0, e=0.0, ratio=0.0)
    nX = float(np.linalg.norm(g["X"])) if np.all(np.isfinite(g["X"])) else np.inf
    for i in (1, 2):
        if np.isfinite(dbg[1 + i]) and np.isfinite(nX) and nX > 0:
            gaps["z"] = max(gaps["z"], abs(float(dbg[1 + i]) - g["z%d" % i]) / nX)
        if np.isfinite(dbg[3 + i]) and g["e%d" % i] < 4 * g["th%d" % i]:
            gaps["e"] = max(gaps["e"], abs(float(dbg[3 + i]) - g["e%d" % i]) / g["th%d" % i])
    if np.isfinite(dbg[8]) and np.isfinite(g["ratio"]) and g["ratio"] > 0:
        gaps["ratio"] = abs(float(dbg[8]) - g["ratio"]) / g["ratio"]
    return gaps


def measure():
    """prints what the constants at the top of this file were taken from"""
    from oracle import binding as ob
    ob.build()
    worst_pos, worst_share = (0.0, ""), (0.0, "")
    worst_gap = {kind: (0.0, "") for kind in BAND}
    for name in sorted(FAMILIES):
        for seed in SEEDS:
            case = family_case(name, seed)
            pts, status, _, m12s = serial_reference(ob, case)
            gap = {kind: 0.0 for kind in BAND}
            for k in range(status.shape[0]):
                for q in np.flatnonzero(status[k] >= ST_PARALLAX):
                    for kind, v in gate_discrepancy(case, k, int(q), int(m12s[k, q])).items():
                        gap[kind] = max(gap[kind], v)
            pos, outside, share, total = check64(case, pts, status, m12s)
            counts = np.bincount(status.reshape(-1), minlength=12)
            print("%-20s seed %d  points %4d  pairs %5d  pos %.3g  gaps %s  outside %d  share %.4f  codes %s" %
                  (name, seed, len(pts), total, pos, " ".join("%s %.3g" % kv for kv in sorted(gap.items())), outside, share, counts.tolist()))
            worst_pos, worst_share = max(worst_pos, (pos, name)), max(worst_share, (share, name))
            worst_gap = {kind: max(worst_gap[kind], (gap[kind], name)) for kind in BAND}
    print("position", worst_pos, "gate gaps", worst_gap, "band share (at the BAND in force)", worst_share)


if __name__ == "__main__":
    measure()
