"""Two-view scenes for the initial-map entry (include/orbslamm_initmap.h) and the restatement's shim (tools/initmap_ref.hpp
through tests/cpp/initmap_ref_capi.cpp).  A case is what Tracking::CreateInitialMapMonocular holds at src/Tracking.cc:728: two
poses, mvKeysUn of both frames, mvIniMatches, mvIniP3D.  Each family forces a branch; the sizes are the smallest at which the
summation tree and the compaction can go wrong; seeds 1 .. 10 are open, chosen by no comparison."""
import ctypes as C
import importlib

import numpy as np

import ref_shim
from orbslamm_amd._lib import KP_DTYPE

im = importlib.import_module("orbslamm_amd.initial_map")   # (the package exports the function of the same name over the module)

SERIAL, DEFINED = 0, 1
NLEVELS = 8
SIZES = (1, 2, 63, 64, 65, 89, 90, 130, 600)
SEEDS = tuple(range(1, 11))
K = np.array([520.0, 515.0, 322.5, 241.25], dtype=np.float32)

# family: what differs from `noisy` (1 px, octave 0, first pose fixed, 20 iterations, robust)
FAMILIES = {
    "clean": dict(noise=0.0),
    "noisy": dict(),
    "gross_20": dict(gross=0.2),
    "mixed_octaves": dict(octaves=True),
    "both_free": dict(fixed_first=False),
    "first_fixed": dict(noise=0.5, start_pose=0.02),
    "second_fixed": dict(fixed_first=False, fixed_second=True, start_pose=0.0),
    "from_truth": dict(noise=0.3, start_pose=0.0, start_points=0.0),
    "far_start": dict(start_pose=0.12, start_points=0.08),
    "ten_trials": dict(zero_level=7),
    "behind": dict(behind=True, start_pose=0.0, start_points=0.0),
    "few": dict(sizes=(89, 90)),
    "z_zero": dict(z_zero=True),
    "parallel_rays": dict(depth=(4000.0, 9000.0), start_points=0.0),
    "iterations_0": dict(iterations=0),
    "no_points": dict(no_points=True),
}
# a family's random stream: its rank among the names (second_fixed came later and takes the next number: the others keep theirs)
STREAM = {name: i for i, name in enumerate(sorted(f for f in FAMILIES if f != "second_fixed"))}
STREAM["second_fixed"] = len(STREAM)
REF_KEY = np.dtype([("u", "<f4"), ("v", "<f4"), ("octave", "<i4")])
REF_DIAG = np.dtype([("rejected_trials", "<i4"), ("failed_solves", "<i4"), ("huber_gap", "<f8")])


def scale_factors():
    return (1.2 ** np.arange(NLEVELS)).astype(np.float32)            # mvScaleFactors


def inv_level_sigma2(family="noisy"):
    sf = scale_factors()
    sig = (np.float32(1.0) / (sf * sf)).astype(np.float32)            # mvInvLevelSigma2
    z = FAMILIES[family].get("zero_level")
    if z is not None:
        sig[z] = 0.0                                                  # every edge's information is the zero matrix: ten_trials
    return sig


def _pose(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_case(family, n, seed):
    f = FAMILIES[family]
    rng = np.random.RandomState((1000003 * seed + 7919 * n + STREAM[family]) % 2 ** 32)
    noise, depth = f.get("noise", 1.0), f.get("depth", (4.0, 9.0))
    # the truth: camera 1 at a fixed pose of the world (not the identity: the centres and depths are then no copies of inputs),
    # camera 2 a baseline to its right with a small rotation
    R1 = ref_shim.rot_axis_angle([0.0, 1.0, 0.0], 0.25 if not f.get("z_zero") else np.pi / 4)
    t1 = np.array([0.3, -0.2, 0.5])
    R21 = ref_shim.rot_axis_angle(rng.normal(size=3), 0.05 + 0.03 * rng.rand())
    t21 = np.array([-0.6, 0.05 * rng.normal(), 0.05 * rng.normal()])
    R2, t2 = R21 @ R1, R21 @ t1 + t21
    sgn = -1.0 if f.get("behind") else 1.0
    z = sgn * rng.uniform(depth[0], depth[1], size=n)
    Pc1 = np.stack([rng.uniform(-0.45, 0.45, size=n) * z, rng.uniform(-0.35, 0.35, size=n) * z, z], axis=1)
    Xw = (Pc1 - t1) @ R1                                              # R1^T (Pc - t1)
    n1, n2 = n + n // 3 + 2, n + 5
    feat1 = np.sort(rng.choice(n1, size=n, replace=False))            # the matched features of frame 1, ascending
    feat2 = rng.permutation(n2)[:n]
    octave = rng.randint(0, NLEVELS, size=(2, n)) if f.get("octaves") else np.zeros((2, n), dtype=np.int64)
    if f.get("zero_level") is not None:
        octave[:] = f["zero_level"]
    sf = scale_factors().astype(np.float64)
    keys = [np.zeros(n1, dtype=KP_DTYPE), np.zeros(n2, dtype=KP_DTYPE)]
    for kk in keys:
        kk["x"], kk["y"] = rng.uniform(0, 640, size=kk.shape[0]), rng.uniform(0, 480, size=kk.shape[0])
        kk["octave"] = rng.randint(0, NLEVELS, size=kk.shape[0])
    for s, (R, t, feat) in enumerate(((R1, t1, feat1), (R2, t2, feat2))):
        Pc = Xw @ R.T + t
        uv = np.stack([K[0] * Pc[:, 0] / Pc[:, 2] + K[2], K[1] * Pc[:, 1] / Pc[:, 2] + K[3]], axis=1)
        uv += noise * sf[octave[s]][:, None] * rng.normal(size=(n, 2))
        if f.get("gross") and s == 1:
            bad = rng.rand(n) < f["gross"]
            uv[bad] += rng.uniform(12.0, 40.0, size=(int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2))
        keys[s]["x"][feat], keys[s]["y"][feat], keys[s]["octave"][feat] = uv[:, 0], uv[:, 1], octave[s]
    matches12 = np.full(n1, -1, dtype=np.int32)
    matches12[feat1] = feat2
    # the start: the second pose and the points perturbed
    sp, sx = f.get("start_pose", 0.01), f.get("start_points", 0.01)
    dR = ref_shim.rot_axis_angle(rng.normal(size=3), sp * rng.uniform(0.5, 1.0)) if sp else np.eye(3)
    R2s, t2s = dR @ R2, t2 + sp * rng.normal(size=3)
    if f.get("z_zero") and seed % 2:
        # the world turned so that the second pose STARTS with the identity as its rotation: its quaternion is (0, 0, 0, 1) and
        # a point's camera z is exactly Xw.z + t.z (the projections do not change)
        W = R2s
        Xw, R1, R2, R2s = Xw @ W.T, R1 @ W.T, R2 @ W.T, np.eye(3)
    P3D = np.zeros((n1, 3), dtype=np.float32)
    P3D[feat1] = Xw * (1.0 + sx * rng.normal(size=(n, 1))) if sx else Xw
    if f.get("z_zero"):
        if seed % 2:
            P3D[feat1[0], 2] = -np.float32(t2s[2])                    # ON camera 2's plane: z = 0 exactly, x / z and y / z infinite
        else:
            r = R1.astype(np.float32)[2]                              # finite, but its depth in camera 1 is not as a float
            P3D[feat1[0]] = np.array([3.0e38 * np.sign(r[0]), 0.0, 3.0e38 * np.sign(r[2])], dtype=np.float32)
    if f.get("no_points"):
        matches12[:] = -1
    return dict(family=family, n=n, seed=seed, Tcw1=_pose(R1, t1), Tcw2=_pose(R2s, t2s), K=K, keys_un1=keys[0], keys_un2=keys[1],
                matches12=matches12, P3D=P3D, fixed_first=f.get("fixed_first", True), fixed_second=f.get("fixed_second", False), iterations=f.get("iterations", 20), robust=True,
                truth=dict(R1=R1, t1=t1, R2=R2, t2=t2, Xw=Xw, feat1=feat1))


_cases, _refs = {}, {}


def family_cases(family):
    """every size x open seed of a family, in one fixed order"""
    if family not in _cases:
        _cases[family] = [make_case(family, n, s) for n in FAMILIES[family].get("sizes", SIZES) for s in SEEDS]
    return _cases[family]


def _declare(L):
    L.initmapref_sizes.restype = C.c_int
    L.initmapref_run.restype = None
    L.initmapref_run.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3
    L.initmapref_inverse3.argtypes = [C.c_void_p] * 2
    L.initmapref_ldlt.restype = C.c_int
    L.initmapref_ldlt.argtypes = [C.c_int] + [C.c_void_p] * 3
    assert [L.initmapref_sizes(i) for i in range(5)] == [im.PROBLEM_DTYPE.itemsize, im.RESULT_DTYPE.itemsize, im.POINT_DTYPE.itemsize,
                                                         REF_KEY.itemsize, REF_DIAG.itemsize]


def ref_lib():
    return ref_shim.cached_shim("initmap_ref", _declare)


def ref_keys(keys_un):
    k = np.zeros(keys_un.shape[0], dtype=REF_KEY)
    k["u"], k["v"], k["octave"] = keys_un["x"], keys_un["y"], keys_un["octave"]
    return k


def ref_run(case, mode, sig=None, sf=None):
    """the restatement on one case: (result record, points, diagnostics)"""
    L = ref_lib()
    pr = np.zeros(1, dtype=im.PROBLEM_DTYPE)
    pr[0] = im.pack_problem(case)
    k1, k2 = ref_keys(case["keys_un1"]), ref_keys(case["keys_un2"])
    m12, p3d = np.ascontiguousarray(case["matches12"], dtype=np.int32), np.ascontiguousarray(case["P3D"], dtype=np.float32)
    sig = inv_level_sigma2(case["family"]) if sig is None else sig
    sf = scale_factors() if sf is None else sf
    out, pts, dg = np.zeros(1, dtype=im.RESULT_DTYPE), np.zeros(max(m12.shape[0], 1), dtype=im.POINT_DTYPE), np.zeros(1, dtype=REF_DIAG)
    L.initmapref_run(mode, ref_shim.p(pr), ref_shim.p(k1), ref_shim.p(k2), ref_shim.p(m12), ref_shim.p(p3d), ref_shim.p(sig), ref_shim.p(sf),
                     NLEVELS, ref_shim.p(out), ref_shim.p(pts), ref_shim.p(dg))
    return out[0], pts[:m12.shape[0]], dg[0]


def family_ref(family, mode):
    """the restatement over family_cases(family): a list of (result, points, diagnostics), computed once and left unchanged"""
    if (family, mode) not in _refs:
        _refs[(family, mode)] = [ref_run(c, mode) for c in family_cases(family)]
    return _refs[(family, mode)]


def pose_distance(Ta, Tb):
    """(the rotation between as an angle, the distance between the translations) of two poses given as 3x4 or 4x4; two float32
    poses that differ in no entry give (0, 0)"""
    Ta, Tb = np.asarray(Ta, dtype=np.float64).reshape(-1, 4)[:3], np.asarray(Tb, dtype=np.float64).reshape(-1, 4)[:3]
    d = Ta[:, :3] - Tb[:, :3]                          # (for a small angle a: |d|_F = sqrt(2) a; arccos would lose it)
    return float(np.linalg.norm(d) / np.sqrt(2.0)), float(np.linalg.norm(Ta[:, 3] - Tb[:, 3]))
