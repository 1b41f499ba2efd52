"""The Initializer's checker for the tests: the C++ restatement (tools/init_ref.hpp) built with g++ -ffp-contract=off
behind a small C shim (tests/cpp/init_ref_capi.cpp), and a two-view scene generator (general 3-D or planar, with noise
and outliers)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from orbslamm_amd._lib import KP_DTYPE
from orbslamm_amd.initializer import OrbiResult, result_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], dtype=np.float32)
_ref = None


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    global _ref
    if _ref is None:
        out = os.path.join(tempfile.mkdtemp(prefix="init_ref_"), "libinit_ref.so")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "cpp", "init_ref_capi.cpp"), "-o", out])
        L = C.CDLL(out)
        vp = C.c_void_p
        L.initref_initialize.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_float, C.c_int, C.c_int, vp, vp, C.POINTER(OrbiResult), vp, vp]
        L.initref_svd.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.initref_normalize.argtypes = [vp, C.c_int, vp, vp]
        L.initref_draw_sets.argtypes = [C.c_int, C.c_int, vp]
        L.initref_random_int.argtypes = [C.c_int, C.c_int]
        _ref = L
    return _ref


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


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
    """bit-equal float32 arrays (NaN payloads included)"""
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
