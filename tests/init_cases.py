"""The Initializer's checker for the tests: the C++ restatement (tools/init_ref.hpp) built with g++ -ffp-contract=off
behind a small C shim (tests/cpp/init_ref_capi.cpp), and a two-view scene generator (general 3-D or planar, with noise
and outliers)."""
import ctypes as C
import os

import numpy as np

from ref_shim import cached_shim, p as _p
from orbslamm_amd._lib import KP_DTYPE
from orbslamm_amd.initializer import OrbiResult, result_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], dtype=np.float32)
def _declare(L):
    vp = C.c_void_p
    L.initref_initialize.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_float, C.c_int, C.c_int, vp, vp, C.POINTER(OrbiResult), vp, vp]
    L.initref_svd.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.initref_normalize.argtypes = [vp, C.c_int, vp, vp]
    L.initref_draw_sets.argtypes = [C.c_int, C.c_int, vp]
    L.initref_random_int.argtypes = [C.c_int, C.c_int]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("init_ref", _declare)


def ref_initialize(keys1, keys2, m12, sets, K=K_TUM, sigma=1.0, model="HF"):
    """the restatement's Initializer(keys1, K, sigma, iterations) + Initialize: same dict as Initializer.initialize"""
    L = ref_lib()
    keys1 = np.ascontiguousarray(keys1, dtype=KP_DTYPE)
    keys2 = np.ascontiguousarray(keys2, dtype=KP_DTYPE)
    m12 = np.ascontiguousarray(m12, dtype=np.int32)
    sets = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1)
    K = np.ascontiguousarray(K, dtype=np.float32)
    n1 = keys1.shape[0]
    res = OrbiResult()
    p3d = np.zeros((max(n1, 1), 3), dtype=np.float32)
    tri = np.zeros(max(n1, 1), dtype=np.uint8)
    ok = L.initref_initialize(_p(keys1), n1, _p(keys2), keys2.shape[0], _p(K), float(sigma), sets.shape[0] // 8, int(model == "HF"),
                              _p(m12), _p(sets), C.byref(res), _p(p3d), _p(tri))
    r = result_fields(res)
    assert bool(ok) == bool(r["ok"])
    return dict(ok=bool(ok), R21=r["R21"].reshape(3, 3), t21=r["t21"], p3d=p3d[:n1], triangulated=tri[:n1].astype(bool), res=r)


def ref_svd(a, full=True):
    a = np.ascontiguousarray(a, dtype=np.float32)
    m, n = a.shape
    w = np.zeros(max(m, n), np.float32)
    u = np.zeros(max(m, n) ** 2, np.float32)
    vt = np.zeros(max(m, n) ** 2, np.float32)
    dims = np.zeros(5, np.int32)
    ref_lib().initref_svd(_p(a), m, n, int(full), _p(w), _p(u), _p(vt), _p(dims))
    return w[:dims[0]], u[:dims[1] * dims[2]].reshape(dims[1], dims[2]), vt[:dims[3] * dims[4]].reshape(dims[3], dims[4])


def ref_normalize(keys):
    keys = np.ascontiguousarray(keys, dtype=KP_DTYPE)
    T = np.zeros(9, np.float32)
    pn = np.zeros((max(keys.shape[0], 1), 2), np.float32)
    ref_lib().initref_normalize(_p(keys), keys.shape[0], _p(T), _p(pn))
    return T.reshape(3, 3), pn[:keys.shape[0]]


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def keys_from_xy(xy, rng):
    k = np.zeros(xy.shape[0], dtype=KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"] = 31.0
    k["angle"] = rng.uniform(0, 360, xy.shape[0])
    k["response"] = rng.uniform(0, 100, xy.shape[0])
    k["octave"] = rng.integers(0, 8, xy.shape[0])
    k["class_id"] = -1
    return k


def make_scene(rng, n_match=500, n1=1000, n2=1000, planar=False, noise=0.5, outliers=0.3, K=K_TUM, w=640, h=480,
               R=None, t=None):
    """two frames of n1 / n2 keys; n_match of frame 1's keys are matched (matches12), the rest unmatched; a fraction
    `outliers` of the matches point at random frame 2 keys.  Returns (keys1, keys2, matches12, R, t) with R, t the true
    camera 2 pose (x2 = R x1 + t)."""
    fx, fy, cx, cy = [float(v) for v in K]
    R = rot(0.02, -0.08, 0.01) if R is None else R
    t = np.array([0.6, 0.05, 0.1]) if t is None else t
    pts = []
    while len(pts) < n_match:
        u, v = rng.uniform(20, w - 20), rng.uniform(20, h - 20)
        z = (4.0 + 0.3 * (u - cx) / fx + 0.2 * (v - cy) / fy) if planar else rng.uniform(3.0, 9.0)
        X = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        X2 = R @ X + t
        if X2[2] <= 0.5:
            continue
        u2, v2 = fx * X2[0] / X2[2] + cx, fy * X2[1] / X2[2] + cy
        if not (5 <= u2 < w - 5 and 5 <= v2 < h - 5):
            continue
        pts.append((u, v, u2, v2))
    pts = np.array(pts)
    xy1 = np.concatenate([pts[:, :2], rng.uniform([0, 0], [w, h], (n1 - n_match, 2))])
    xy2m = pts[:, 2:] + rng.normal(0, noise, (n_match, 2))
    xy2 = np.concatenate([xy2m, rng.uniform([0, 0], [w, h], (n2 - n_match, 2))])
    p1 = rng.permutation(n1)       # frame 1 key order
    p2 = rng.permutation(n2)
    inv2 = np.argsort(p2)
    keys1 = keys_from_xy(xy1[p1].astype(np.float32), rng)
    keys2 = keys_from_xy(xy2[p2].astype(np.float32), rng)
    m12 = np.full(n1, -1, np.int32)
    for new_i, old_i in enumerate(p1):
        if old_i < n_match:
            j = inv2[old_i]
            if rng.uniform() < outliers:
                j = int(rng.integers(0, n2))
            m12[new_i] = j
    return keys1, keys2, m12, R, t


def same(a, b):
    """bit-equal float32 arrays (NaN payloads included).  Not ref_shim.same: this one takes ctypes arrays and lists and
    converts them, so it compares neither dtype nor shape."""
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def assert_equal_results(got, want, n_cand_fields=True):
    """every output and diagnostic, as bits"""
    g, w = got["res"], want["res"]
    for k in ("ok", "reconstructed_h", "rt_state", "it_H", "it_F", "inliers_H", "inliers_F", "n_matches", "n_inliers", "n_candidates", "best"):
        assert g[k] == w[k], (k, g[k], w[k])
    for k in ("SH", "SF", "RH", "H21", "F21", "R21", "t21", "parallax"):
        assert same(g[k], w[k]), (k, g[k], w[k])
    assert np.array_equal(g["n_good"], w["n_good"]), (g["n_good"], w["n_good"])
    assert got["ok"] == want["ok"]
    assert same(got["p3d"], want["p3d"]), np.argwhere(got["p3d"].view(np.uint32) != want["p3d"].view(np.uint32))[:5]
    assert np.array_equal(got["triangulated"], want["triangulated"])


# ------------------------------------------------------------------------------------------------ scene families
# make_case(family, rng, variant) builds one named two-view case with its ground truth.  Camera 2's pose is x2 = R x1 + t
# (C2 = -R^T t is its centre in frame 1).  variant: "clean" (no noise, no outliers), "noisy" (0.5 px on both frames) or
# "outliers" (noisy, and a quarter of the matches re-pointed at random frame 2 keys).  Every case carries what its family
# must end as (`expect`), checked by check_result.
FAMILIES = ("lateral", "forward", "backward", "rotation", "near_rotation", "small_parallax", "large_rotation", "wide_inward",
            "plane_fronto", "plane_slanted", "plane_along_t", "two_planes", "coincident_rays", "shared_key2",
            "outside_image", "collapsed1", "collapsed2")
VARIANTS = {"clean": (0.0, 0.0), "noisy": (0.5, 0.0), "outliers": (0.5, 0.25)}
PLANAR = ("plane_fronto", "plane_slanted", "plane_along_t")
ROTATION_ONLY = ("rotation", "near_rotation")
GENERAL = ("lateral", "forward", "backward", "large_rotation", "wide_inward", "outside_image", "shared_key2")


def pose_from_centre(R, C2):
    return R, -R @ np.asarray(C2, np.float64)


def look_at(C2, target):
    """the rotation of a camera at C2 (frame 1) whose optical axis points at target, y kept near frame 1's y"""
    z = np.asarray(target, np.float64) - np.asarray(C2, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def _pixels_depth(rng, m, K, w, h, zfun, margin=20.0):
    """m points of frame 1 from pixels drawn in the image (inset by margin) and a depth per pixel"""
    fx, fy, cx, cy = [float(v) for v in K]
    u, v = rng.uniform(margin, w - margin, m), rng.uniform(margin, h - margin, m)
    rx, ry = (u - cx) / fx, (v - cy) / fy
    z = zfun(rx, ry)
    return np.stack([rx * z, ry * z, z], axis=1)


def _plane(n, d):
    """depth along the ray (rx, ry, 1) on the plane n.X = d"""
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    return lambda rx, ry: d / (n[0] * rx + n[1] * ry + n[2])


def _project(X, R, t, K):
    fx, fy, cx, cy = [float(v) for v in K]
    X2 = X @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        x1 = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], axis=1)
        x2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], axis=1)
    return x1, x2, X2


def _visible(rng, sampler, n, R, t, K, w, h, margin=-5.0, zmax=60.0):
    """n points from sampler(rng, m) seen by both cameras (in front, projected inside the image grown by margin)"""
    out = []
    got = 0
    for _ in range(200):
        X = sampler(rng, max(4 * (n - got), 64))
        x1, x2, X2 = _project(X, R, t, K)
        ok = (X[:, 2] > 0.3) & (X2[:, 2] > 0.3) & (X[:, 2] < zmax) & np.all(np.isfinite(x1) & np.isfinite(x2), axis=1)
        for x in (x1, x2):
            ok &= (x[:, 0] >= -margin) & (x[:, 0] < w + margin) & (x[:, 1] >= -margin) & (x[:, 1] < h + margin)
        out.append(X[ok])
        got += int(ok.sum())
        if got >= n:
            break
    X = np.concatenate(out)[:n]
    assert X.shape[0] == n, "scene sampler starved"
    return X


def _assemble(rng, X, R, t, K, w, h, n1, n2, noise, outliers, x1=None, x2=None, exact=0):
    """keys of both frames in random order: the n_match = len(X) matched ones first (noise on both), the rest uniform in
    the image; a fraction `outliers` of the matches re-pointed at a random frame 2 key.  Returns keys1, keys2, m12 and
    X1 (n1 x 3): the true point of each frame 1 key whose match is true (NaN elsewhere)."""
    m = X.shape[0]
    if x1 is None:
        x1, x2, _ = _project(X, R, t, K)
    if noise:
        e1 = rng.normal(0, noise, x1.shape)
        e1[:exact] = 0                                # (the first `exact` frame 1 keys keep their coordinates)
        x1, x2 = x1 + e1, x2 + rng.normal(0, noise, x2.shape)
    xy1 = np.concatenate([x1, rng.uniform([0, 0], [w, h], (n1 - m, 2))])
    xy2 = np.concatenate([x2, rng.uniform([0, 0], [w, h], (n2 - m, 2))])
    p1, p2 = rng.permutation(n1), rng.permutation(n2)
    inv1, inv2 = np.argsort(p1), np.argsort(p2)
    keys1 = keys_from_xy(xy1[p1].astype(np.float32), rng)
    keys2 = keys_from_xy(xy2[p2].astype(np.float32), rng)
    m12 = np.full(n1, -1, np.int32)
    X1 = np.full((n1, 3), np.nan)
    for k in range(m):
        i = inv1[k]
        if rng.uniform() < outliers:
            m12[i] = int(rng.integers(0, n2))
        else:
            m12[i] = inv2[k]
            X1[i] = X[k]
    return keys1, keys2, m12, X1


def make_case(family, rng, variant="noisy", n_match=300, n1=None, n2=None, K=K_TUM, w=640, h=480, noise=None, baseline=1.0):
    """one case of a family: dict(family, variant, keys1, keys2, m12, R, t, X1, K, expect).  X1 holds the true 3-D point
    (frame 1) of every truly matched frame 1 key.  expect: "never" (may not initialise), "H" / "F" (the model picked in
    HF), "nothing" (no hypothesis scores), or None; succeeds: a noiseless case that must initialise with the true pose.  noise
    overrides the variant's; baseline scales t (and leaves `expect` to the caller)."""
    noise, outl = (VARIANTS[variant][0] if noise is None else noise), VARIANTS[variant][1]
    n1 = n1 or n_match + n_match // 3
    n2 = n2 or n_match + n_match // 4
    K = np.asarray(K, np.float32)
    fx, fy, cx, cy = [float(v) for v in K]
    clean = variant == "clean"
    x1 = x2 = None
    depth = lambda lo, hi: (lambda rng, m: _pixels_depth(rng, m, K, w, h, lambda rx, ry: rng.uniform(lo, hi, rx.shape)))
    expect = None
    if family in ("lateral", "shared_key2", "outside_image", "coincident_rays", "collapsed1", "collapsed2"):
        R, t = rot(0.02, -0.08, 0.01), np.array([0.6, 0.05, 0.1])
        sampler = depth(3.0, 9.0)
        expect = "F" if clean else None
    if family == "forward":
        R, t = pose_from_centre(rot(0.01, 0.03, -0.02), [0.06, -0.04, 1.0])
        sampler = depth(4.0, 12.0)
        expect = "F" if clean else None
    elif family == "backward":
        R, t = pose_from_centre(rot(-0.02, 0.02, 0.03), [-0.05, 0.03, -1.0])
        sampler = depth(3.0, 10.0)
        expect = "F" if clean else None
    elif family == "rotation":
        R, t = rot(0.04, 0.12, -0.03), np.zeros(3)
        sampler = depth(3.0, 9.0)
        expect = "never"
    elif family == "near_rotation":       # baseline 0.01 against depths 3 to 9: every parallax below 0.2 degrees
        R, t = pose_from_centre(rot(0.03, -0.1, 0.02), 0.01 * np.array([0.9, 0.3, 0.3]))
        sampler = depth(3.0, 9.0)
        expect = "never"
    elif family == "small_parallax":      # baseline 0.035 against depths 2.2 to 4.5: parallax 0.45 to 0.9 degrees
        R, t = pose_from_centre(rot(0.02, -0.05, 0.01), 0.035 * np.array([0.95, 0.2, 0.1]))
        sampler = depth(2.2, 4.5)
        expect = "never" if clean else None               # (noise can carry the estimated pose's parallax past 1)
    elif family == "large_rotation":      # 20 to 40 degrees about y, orbiting the scene's centre
        a = np.radians(rng.uniform(20, 40)) * rng.choice([-1, 1])
        target = np.array([0.0, 0.0, 6.0])
        R = rot(rng.uniform(-0.03, 0.03), a, rng.uniform(-0.03, 0.03))
        t = target - R @ target
        sampler = depth(4.5, 7.5)
        expect = "F" if clean else None
    elif family == "wide_inward":         # rays up to ~100 degrees apart: some cosParallax negative
        X0, C2 = np.array([0.22, 0.0, 0.72]), np.array([1.45, 0.0, 0.3])
        R, t = pose_from_centre(look_at(C2, X0), C2)
        sampler = lambda rng, m: X0 + rng.uniform(-0.12, 0.12, (m, 3))
        expect = "F" if clean else None
    elif family == "plane_fronto":
        R, t = rot(0.01, -0.06, 0.02), np.array([0.5, 0.05, 0.05])
        sampler = lambda rng, m: _pixels_depth(rng, m, K, w, h, _plane([0, 0, 1], 4.0))
        expect = "H" if clean else None
    elif family == "plane_slanted":       # normal 55 degrees off the optical axis
        R, t = rot(0.02, -0.05, 0.01), np.array([0.45, -0.08, 0.1])
        sampler = lambda rng, m: _pixels_depth(rng, m, K, w, h, _plane([np.sin(0.96), 0.0, np.cos(0.96)], 3.0))
        expect = "H" if clean else None
    elif family == "plane_along_t":       # moving towards a plane: its normal nearly parallel to t
        R, t = pose_from_centre(rot(0.01, 0.02, 0.0), [0.04, 0.02, 0.9])
        sampler = lambda rng, m: _pixels_depth(rng, m, K, w, h, _plane([0.05, -0.03, 1.0], 5.0))
        expect = "H" if clean else None
    elif family == "two_planes":
        R, t = rot(0.02, -0.07, 0.0), np.array([0.55, 0.0, 0.08])
        pa, pb = _plane([0.3, 0.0, 1.0], 3.5), _plane([-0.4, 0.2, 1.0], 7.0)
        sampler = lambda rng, m: np.concatenate([_pixels_depth(rng, m - m // 2, K, w, h, pa), _pixels_depth(rng, m // 2, K, w, h, pb)])
    if baseline != 1.0:
        t = t * baseline
        expect = None
    if family == "coincident_rays":
        # forward motion; a tenth of the matches lie on the baseline (both rays the same line: the keys are the two
        # epipoles) and a tenth so far away that their rays are parallel (cosParallax >= 0.99998)
        R, t = pose_from_centre(rot(0.01, 0.02, -0.01), [0.08, 0.05, 1.0])
        C2 = -R.T @ t
        nb = n_match // 10
        base = C2[None, :] * rng.uniform(2.0, 8.0, (nb, 1))
        X = np.concatenate([_visible(rng, depth(4.0, 12.0), n_match - 2 * nb, R, t, K, w, h), base,
                            _visible(rng, depth(300.0, 3000.0), nb, R, t, K, w, h, zmax=1e4)])
    elif family == "outside_image":
        # undistorted keys up to 8 px outside the image on either side, and six frame 1 keys on x = 1 or y = 1 exactly
        # (Triangulate's x == 1 branch); their true points move onto those rays, and noise stays off those six keys
        sampler = lambda rng, m: _pixels_depth(rng, m, K, w, h, lambda rx, ry: rng.uniform(3.0, 9.0, rx.shape), margin=-8.0)
        X = _visible(rng, sampler, n_match, R, t, K, w, h, margin=8.0)
        x1, _, _ = _project(X, R, t, K)
        x1[0:12:2, 0], x1[1:12:2, 1] = 1.0, 1.0
        X[:12] = _unproject(x1[:12], X[:12, 2], K)
        _, x2, _ = _project(X, R, t, K)
    else:
        X = _visible(rng, sampler, n_match, R, t, K, w, h)
    keys1, keys2, m12, X1 = _assemble(rng, X, R, t, K, w, h, n1, n2, noise, outl, x1=x1, x2=x2,
                                      exact=12 if family == "outside_image" else 0)
    if family == "shared_key2":
        # a tenth of the matched frame 1 keys get a twin key (0.2 px away) matched to the same frame 2 key
        src = rng.choice(np.flatnonzero(m12 >= 0), n_match // 10, replace=False)
        twins = keys1[src].copy()
        twins["x"] += np.float32(0.2)
        keys1 = np.concatenate([keys1, twins])
        m12 = np.concatenate([m12, m12[src]])
        X1 = np.concatenate([X1, np.full((len(src), 3), np.nan)])
    if family == "collapsed1":
        keys1["x"], keys1["y"] = 300.0, 200.0
        X1[:] = np.nan
        expect = "nothing"
    if family == "collapsed2":
        keys2["x"], keys2["y"] = 100.0, 200.0
        X1[:] = np.nan
        expect = "nothing"
    # noiseless cases that must initialise (plane_along_t's two planar solutions tie: secondBestGood fails)
    succeeds = clean and baseline == 1.0 and family in GENERAL + ("plane_fronto", "plane_slanted", "coincident_rays")
    return dict(family=family, variant=variant, keys1=keys1, keys2=keys2, m12=m12, R=R, t=t, X1=X1, K=K, expect=expect,
                succeeds=succeeds)


def _unproject(x, z, K):
    fx, fy, cx, cy = [float(v) for v in K]
    return np.stack([(x[:, 0] - cx) / fx * z, (x[:, 1] - cy) / fy * z, z], axis=1)


def random_sets(rng, n, iterations):
    """iterations x 8 distinct indices in [0, n) (any sets are valid input; make_sets is the reference's draw)"""
    s = rng.integers(0, n, (iterations, 8))
    for r in range(iterations):
        if len(set(s[r].tolist())) < 8:
            s[r] = rng.permutation(n)[:8]
    return s.astype(np.int32)


# ------------------------------------------------------------------------------------------------ float64 geometric check
# check_result holds any Initialize result (device or restatement) to the geometry in float64 and plain numpy.  Float32
# rounding is bounded per value from the magnitudes involved: U = 2^-24 is float32's unit roundoff and each bound counts
# the roundings of the float32 formula it stands for (one U per product, sum, division), times 2 for the second-order terms.
U32 = 2.0 ** -24
TH_H, TH_F = 5.991, 3.841


def _chi_h(H, x1, x2, inv_s2):
    """CheckHomography's chi-square of x1 mapped by H against x2, and its float32 error bound (H given as float32 values;
    a float32 H12 = inv(H21) adds one rounding to every coefficient: counted as one more U per term)"""
    num_u = H[0, 0] * x1[:, 0] + H[0, 1] * x1[:, 1] + H[0, 2]
    num_v = H[1, 0] * x1[:, 0] + H[1, 1] * x1[:, 1] + H[1, 2]
    den = H[2, 0] * x1[:, 0] + H[2, 1] * x1[:, 1] + H[2, 2]
    a_u = np.abs(H[0, 0] * x1[:, 0]) + np.abs(H[0, 1] * x1[:, 1]) + np.abs(H[0, 2])
    a_v = np.abs(H[1, 0] * x1[:, 0]) + np.abs(H[1, 1] * x1[:, 1]) + np.abs(H[1, 2])
    a_d = np.abs(H[2, 0] * x1[:, 0]) + np.abs(H[2, 1] * x1[:, 1]) + np.abs(H[2, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = num_u / den, num_v / den
        du, dv = x2[:, 0] - u, x2[:, 1] - v
        sq = du * du + dv * dv
        chi = sq * inv_s2
        rel_d = 4 * U32 * a_d / np.abs(den)
        e_u = 4 * U32 * a_u / np.abs(den) + np.abs(u) * rel_d + 2 * U32 * np.abs(u) + U32 * np.abs(du)
        e_v = 4 * U32 * a_v / np.abs(den) + np.abs(v) * rel_d + 2 * U32 * np.abs(v) + U32 * np.abs(dv)
        err = 2 * ((2 * np.abs(du) * e_u + 2 * np.abs(dv) * e_v + e_u * e_u + e_v * e_v) * inv_s2 + 5 * U32 * chi)
    return chi, err


def _chi_f(F, x1, x2, inv_s2):
    """CheckFundamental's chi-square of x2 against the line F x1, and its float32 error bound"""
    a = F[0, 0] * x1[:, 0] + F[0, 1] * x1[:, 1] + F[0, 2]
    b = F[1, 0] * x1[:, 0] + F[1, 1] * x1[:, 1] + F[1, 2]
    c = F[2, 0] * x1[:, 0] + F[2, 1] * x1[:, 1] + F[2, 2]
    ea = 3 * U32 * (np.abs(F[0, 0] * x1[:, 0]) + np.abs(F[0, 1] * x1[:, 1]) + np.abs(F[0, 2]))
    eb = 3 * U32 * (np.abs(F[1, 0] * x1[:, 0]) + np.abs(F[1, 1] * x1[:, 1]) + np.abs(F[1, 2]))
    ec = 3 * U32 * (np.abs(F[2, 0] * x1[:, 0]) + np.abs(F[2, 1] * x1[:, 1]) + np.abs(F[2, 2]))
    num = a * x2[:, 0] + b * x2[:, 1] + c
    e_num = 3 * U32 * (np.abs(a * x2[:, 0]) + np.abs(b * x2[:, 1]) + np.abs(c)) + np.abs(x2[:, 0]) * ea + np.abs(x2[:, 1]) * eb + ec
    den = a * a + b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        e_den = (2 * np.abs(a) * ea + 2 * np.abs(b) * eb) / den + 3 * U32
        chi = num * num / den * inv_s2
        err = 2 * ((2 * np.abs(num) * e_num + e_num * e_num) / den * inv_s2 + chi * (e_den + 4 * U32))
    return chi, err


def _rescore(chis, th, th_score, score_got, inliers_got, what):
    """the score and the inlier count of one hypothesis from its two chi-square columns ((chi, err) pairs) in match
    order.  Terms whose float64 chi-square lies within its float32 error of the threshold are counted (n_at) and may
    go either way; every other term must agree.  The score's bound: each term's error, each ordered float32 addition's
    rounding (U times the partial sum) and, for each term at the threshold, the whole term."""
    (c1, e1), (c2, e2) = chis
    assert np.all(np.isfinite(c1) & np.isfinite(c2)), what + ": non-finite chi-square under the returned hypothesis"
    at1, at2 = np.abs(c1 - th) <= e1, np.abs(c2 - th) <= e2
    in1, in2 = (c1 <= th) & ~at1, (c2 <= th) & ~at2
    terms = np.stack([np.where(in1, th_score - c1, 0.0), np.where(in2, th_score - c2, 0.0)], axis=1).reshape(-1)
    t_err = np.stack([np.where(in1, e1 + U32 * np.abs(th_score - c1), 0.0), np.where(in2, e2 + U32 * np.abs(th_score - c2), 0.0)], axis=1).reshape(-1)
    amb = np.stack([np.where(at1, np.abs(th_score - c1) + e1, 0.0), np.where(at2, np.abs(th_score - c2) + e2, 0.0)], axis=1).reshape(-1)
    partial = np.cumsum(terms + amb)
    score = float(terms.sum())
    bound = float(t_err.sum() + U32 * np.abs(partial).sum() + amb.sum()) + 1e-30
    n_at = int((at1 | at2).sum())
    assert abs(float(score_got) - score) <= bound, (what, "score", float(score_got), score, bound, n_at)
    sure = int((in1 & in2).sum())
    maybe = int(((in1 | at1) & (in2 | at2)).sum())
    assert sure <= inliers_got <= maybe, (what, "inliers", inliers_got, sure, maybe, n_at)
    return n_at


def _inv(v):
    return 1.0 / float(v)


def cos_parallax(P, R, t):
    """float64 cosParallax of points P (frame 1) for camera 2 at O2 = -R^T t"""
    O2 = -R.T @ t
    n1, n2 = P, P - O2
    return np.einsum("ij,ij->i", n1, n2) / (np.linalg.norm(n1, axis=1) * np.linalg.norm(n2, axis=1))


def _angle_deg(Ra, Rb):
    """the angle of Ra^T Rb from its sine and cosine (arccos of the trace alone loses small angles)"""
    M = Ra.T @ Rb
    s = np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2
    return float(np.degrees(np.arctan2(s, (np.trace(M) - 1) / 2)))


def check_result(case, out, sigma=1.0, model="HF"):
    """the float64 check of one Initialize result (a dict of Initializer.initialize / ref_initialize) on a make_case
    case.  Returns a dict of what it saw (chi-square values at a threshold, stored-but-unflagged points, ...)."""
    keys1, keys2, m12, K = case["keys1"], case["keys2"], case["m12"], np.asarray(case["K"], np.float64)
    r = out["res"]
    fx, fy, cx, cy = K
    i1 = np.flatnonzero(m12 >= 0)
    x1 = np.stack([keys1["x"][i1], keys1["y"][i1]], axis=1).astype(np.float64)
    x2 = np.stack([keys2["x"][m12[i1]], keys2["y"][m12[i1]]], axis=1).astype(np.float64)
    inv_s2 = _inv(np.float32(np.float32(sigma) * np.float32(sigma)))
    seen = dict(at_threshold=0, unflagged=0, min_cos=None)
    assert r["n_matches"] == len(i1)
    # ---- scores: the returned hypotheses rescored over every match
    if r["it_F"] >= 0:
        F = r["F21"].astype(np.float64).reshape(3, 3)
        seen["at_threshold"] += _rescore((_chi_f(F, x1, x2, inv_s2), _chi_f(F.T, x2, x1, inv_s2)), TH_F, TH_H, r["SF"], r["inliers_F"], "F")
    else:
        assert r["SF"] == 0 and r["inliers_F"] == 0
    if r["it_H"] >= 0:
        assert model == "HF"
        H = r["H21"].astype(np.float64).reshape(3, 3)
        seen["at_threshold"] += _rescore((_chi_h(np.linalg.inv(H), x2, x1, inv_s2), _chi_h(H, x1, x2, inv_s2)), TH_H, TH_H, r["SH"], r["inliers_H"], "H")
    else:
        assert r["SH"] == 0 and r["inliers_H"] == 0
    # ---- outcome of the family
    exp = case.get("expect")
    if exp == "nothing":
        assert not out["ok"] and r["n_candidates"] == 0 and r["rt_state"] == 0 and r["it_F"] == -1 and r["it_H"] == -1
    if exp == "never" or case["family"] in ROTATION_ONLY:
        assert not out["ok"], "a rotation-only scene initialised"
    if exp in ("H", "F") and model == "HF":
        assert r["reconstructed_h"] == int(exp == "H"), (exp, r["RH"])
    if case.get("succeeds") and (exp == "F" or model == "HF"):
        assert out["ok"] and r["rt_state"] == 2, ("a noiseless %s scene did not initialise" % case["family"], r["n_good"], r["parallax"])
    if not out["ok"]:
        assert not out["p3d"].any() and not out["triangulated"].any()
        return seen
    # ---- every stored point (the winner's good points): flagged ones in front, reprojected within 4 sigma^2, and
    # cosParallax < 0.99998; unflagged ones cosParallax >= 0.99998 (up to rounding)
    R, t = out["R21"].astype(np.float64), out["t21"].astype(np.float64)
    assert abs(np.linalg.det(R) - 1) < 1e-4 and abs(np.linalg.norm(t) - 1) < 1e-5
    P = out["p3d"].astype(np.float64)
    stored = np.any(out["p3d"] != 0, axis=1)
    flagged = out["triangulated"]
    assert not np.any(flagged & ~stored)
    assert np.all(m12[stored] >= 0)
    Ps = P[stored]
    cos = cos_parallax(Ps, R, t)
    cos_tol = 16 * U32
    fl = flagged[stored]
    assert np.all(cos[fl] < 0.99998 + cos_tol), cos[fl].max()
    assert np.all(cos[~fl] >= 0.99998 - cos_tol), cos[~fl].min()
    seen["unflagged"] = int((~fl).sum())
    seen["min_cos"] = float(cos.min()) if cos.size else None
    X2 = Ps @ R.T + t
    mag = np.abs(Ps) @ np.abs(R).T + np.abs(t)
    assert np.all(Ps[fl, 2] > 0)
    assert np.all(X2[fl, 2] > -4 * U32 * mag[fl, 2])
    j = np.flatnonzero(stored)
    th2 = float(np.float32(4.0 * float(np.float32(np.float32(sigma) * np.float32(sigma)))))
    for X, kp in ((Ps, keys1[j]), (X2, keys2[m12[j]])):
        X = np.where(np.abs(X[:, 2:]) > 0, X, np.nan)                  # (only flagged points are held to it; they have z > 0)
        u, v = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy
        e_u = 6 * U32 * (np.abs(fx * X[:, 0] / X[:, 2]) + abs(cx) + np.abs(kp["x"])) + 4 * U32 * np.abs(fx) * mag[:, 0] / np.abs(X[:, 2])
        e_v = 6 * U32 * (np.abs(fy * X[:, 1] / X[:, 2]) + abs(cy) + np.abs(kp["y"])) + 4 * U32 * np.abs(fy) * mag[:, 1] / np.abs(X[:, 2])
        du, dv = u - kp["x"], v - kp["y"]
        err2 = du * du + dv * dv
        tol = 2 * (2 * np.abs(du) * e_u + 2 * np.abs(dv) * e_v + e_u * e_u + e_v * e_v) + 4 * U32 * th2
        assert np.all(err2[fl] <= th2 + tol[fl]), (err2[fl].max(), th2)
    # ---- a noiseless success recovers the true pose and points (p3d = X_true / |t_true|)
    if case["variant"] == "clean" and (exp == "F" or (exp == "H" and model == "HF")):
        Rt, tt = case["R"], case["t"]
        ang_r = _angle_deg(R, Rt)
        assert ang_r < (0.2 if r["reconstructed_h"] else 0.05), ang_r
        u_t = tt / np.linalg.norm(tt)
        c_t = float(np.dot(t, u_t))
        assert c_t > (0.999 if r["reconstructed_h"] else 0.9999), c_t
        ang_t = float(np.arctan2(np.linalg.norm(np.cross(t, u_t)), c_t))
        Xt = case["X1"][stored] / np.linalg.norm(tt)
        have = np.all(np.isfinite(Xt), axis=1) & fl
        # the error a point inherits from the pose's (rotation + direction error) and from the float32 4x4 SVD, over
        # its parallax, relative to its distance
        par = np.arccos(np.clip(cos_parallax(Xt[have], Rt, u_t), -1, 1))
        ray_err = 4 * (np.radians(ang_r) + ang_t) + 64 * U32
        rel = np.linalg.norm(Ps[have] - Xt[have], axis=1) / np.linalg.norm(Xt[have], axis=1)
        assert np.all(rel <= ray_err / par), (rel.max(), (ray_err / par).min())
    return seen


# ------------------------------------------------------------------------------------------------ outcomes
def outcomes(out):
    """the decision branches of Initialize one result took, read from its fields alone (ReconstructF :514-535 /
    ReconstructH :704-746 of Initializer.cc restated on n_good, parallax, n_inliers).  A failure is named only when it
    is the single condition that failed, so each name marks a branch that decided the result."""
    r = out["res"]
    L = set()
    nc = r["n_candidates"]
    ng = np.asarray(r["n_good"][:nc])
    par = np.asarray(r["parallax"][:nc])
    if out["ok"]:
        L.add("H succeeds" if r["reconstructed_h"] else "F succeeds")
    if nc == 4 and not out["ok"]:
        mx = int(ng.max())
        fails = dict(nsimilar=int((ng > 0.7 * mx).sum()) > 1, nMinGood=mx < max(int(0.9 * r["n_inliers"]), 50))
        if not any(fails.values()):
            assert not par[r["best"]] > np.float32(1.0)          # (a cosParallax rounded above 1 gives NaN)
            L.add("F fails on parallax")
        elif sum(fails.values()) == 1:
            L.add("F fails on " + [k for k, v in fails.items() if v][0])
    if nc == 8 and not out["ok"]:
        best, second = 0, 0
        for g in ng:
            if g > best:
                best, second = g, best
            elif g > second:
                second = g
        fails = dict(secondBestGood=second >= 0.75 * best, parallax=not par[r["best"]] >= np.float32(1.0), minTriangulated=best <= 50,
                     inliers=best <= 0.9 * r["n_inliers"])
        for k, v in fails.items():
            if v:
                L.add("H fails on " + k + ("" if sum(fails.values()) == 1 else " among others"))
    if nc == 0:
        L.add("d1/d2 early exit" if r["reconstructed_h"] else "nothing scores")
    if np.any((ng >= 1) & (ng <= 50)):
        L.add("nGood between 1 and 50")
    if out["ok"]:
        stored = np.any(out["p3d"] != 0, axis=1)
        if np.any(stored & ~out["triangulated"]):
            L.add("stored but not flagged")
        cos = cos_parallax(out["p3d"][stored].astype(np.float64), out["R21"].astype(np.float64), out["t21"].astype(np.float64))
        if cos.size and cos.min() < -1e-3:                     # (the smallest is always among the 51 selected)
            L.add("negative cosParallax selected")
    return L
