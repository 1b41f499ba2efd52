"""The PnPsolver's checker for the tests: the C++ restatement (tools/pnp_ref.hpp) built with g++ -ffp-contract=off behind
a small C shim (tests/cpp/pnp_ref_capi.cpp), named scene families with their true pose, and a float64 numpy check of a
returned result that shares no code with the restatement."""
import ctypes as C
import os

import numpy as np

from ref_shim import cached_shim, p as _p, rot_axis_angle, same
from orbslamm_amd.pnp import EXTRA_SETS, HYP_DTYPE, OrbpResult, make_pnp_sets, result_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], dtype=np.float32)
SIGMA2 = np.array([np.float32(1.2) ** (2 * l) for l in range(8)], dtype=np.float32)   # (the tests' stand-in for mvLevelSigma2)
TRACKING = (0.99, 10, 300, 4, 0.5, 5.991)    # Tracking::Relocalization's SetRansacParameters
DEFAULTS = (0.99, 8, 300, 4, 0.4, 5.991)     # the constructor's

# Tolerances of the float64 check, MEASURED from the restatement on the CPU over seeds 0..9 of every family (every return
# of an iterate(5) replay: see measure() below, `python tests/pnp_cases.py`), then given the margin of 4x this
# project uses for their dependence on conditioning (sim3_cases.py):
#   rotation error of a noiseless volumetric family    measured max 2.93e-8 rad  (far; the pose leaves as CV_32F)
#   |t - t_true| / (1 + |t_true|)                      measured max 1.23e-7     (defaults)
#   the float32 rounding band of error2 against its threshold: |err32 - err64| / th over the points with err < 4 th
#                                                      measured max 7.68e-6     (wrong_40; error2 is a float sum of float squares)
# No mask of those returns disagreed with the float64 recount outside (or inside) the band; the largest share of a case's
# points inside the band was 0: the 2 % cap (a condition, not a measurement) holds for every family and seed used.
TOL_ROT = 4 * 2.93e-8
TOL_T = 4 * 1.23e-7
BAND_REL = 4 * 7.68e-6
BAND_SHARE_CAP = 0.02   # the share of a case's points that may fall inside the band (undecided)
SEEDS = range(10)       # the seeds measured; the tests use these

def _declare(L):
    vp = C.c_void_p
    L.pnpref_svd.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.pnpref_solve_svd.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.pnpref_invert3.argtypes = [vp, vp]
    L.pnpref_qr_solve.argtypes = [vp, vp, vp]
    L.pnpref_mul_transposed.argtypes = [vp, C.c_int, C.c_int, vp]
    L.pnpref_draw_sets.argtypes = [C.c_int, C.c_int, vp]
    L.pnpref_create.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.pnpref_create.restype = vp
    L.pnpref_destroy.argtypes = [vp]
    L.pnpref_destroy.restype = None
    L.pnpref_set_ransac.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
    for f in ("max_iterations", "min_inliers", "iterations"):
        getattr(L, "pnpref_" + f).argtypes = [vp]
    L.pnpref_epsilon.argtypes = [vp]
    L.pnpref_epsilon.restype = C.c_float
    L.pnpref_thresholds.argtypes = [vp, vp]
    L.pnpref_iterate.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(OrbpResult), vp, vp, C.c_int]
    L.pnpref_compute_pose.argtypes = [vp, vp, C.c_int, vp, vp]
    L.pnpref_compute_pose.restype = C.c_double


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("pnp_ref", _declare)


def ref_svd(A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, n = A.shape
    w, ut, vt = np.zeros(n), np.zeros((n, m)), np.zeros((n, n))
    ref_lib().pnpref_svd(_p(A), m, n, _p(w), _p(ut), _p(vt))
    return w, ut, vt


def ref_solve_svd(A, b):
    A, b = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(A.shape[1])
    ref_lib().pnpref_solve_svd(_p(A), A.shape[0], A.shape[1], _p(b), _p(x))
    return x


def ref_invert3(A):
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(3, 3)
    out = np.zeros((3, 3))
    ref_lib().pnpref_invert3(_p(A), _p(out))
    return out


def ref_qr_solve(A, b, x0=None):
    A, b = np.array(A, dtype=np.float64).reshape(6, 4), np.array(b, dtype=np.float64).reshape(6)
    x = np.zeros(4) if x0 is None else np.array(x0, dtype=np.float64)
    ok = ref_lib().pnpref_qr_solve(_p(A), _p(b), _p(x))
    return bool(ok), x


def ref_mul_transposed(M):
    M = np.ascontiguousarray(M, dtype=np.float64)
    out = np.zeros((M.shape[1], M.shape[1]))
    ref_lib().pnpref_mul_transposed(_p(M), M.shape[0], M.shape[1], _p(out))
    return out


def ref_draw_sets(n, iterations):
    out = np.zeros((iterations, 4), np.int32)
    ref_lib().pnpref_draw_sets(n, iterations, _p(out))
    return out


class RefSolver:
    """the restatement's PnPsolver with the interface of orbslamm_amd.pnp.PnPsolver (sets always given)"""

    def __init__(self, case):
        self._L = ref_lib()
        self.case = case
        self.n, self.n_all = case["idx"].shape[0], case["n_all"]
        f = np.float32
        a = [np.ascontiguousarray(case[k], dtype=f) for k in ("P2D", "sigma2", "P3Dw", "K")]
        idx = np.ascontiguousarray(case["idx"], dtype=np.int32)
        self._h = self._L.pnpref_create(self.n_all, _p(idx), self.n, *[_p(x) for x in a])
        self.sets = None
        self.table = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.pnpref_destroy(self._h)
            self._h = None

    max_iterations = property(lambda self: self._L.pnpref_max_iterations(self._h))
    min_inliers = property(lambda self: self._L.pnpref_min_inliers(self._h))
    iterations = property(lambda self: self._L.pnpref_iterations(self._h))
    epsilon = property(lambda self: self._L.pnpref_epsilon(self._h))

    def set_ransac(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        return self._L.pnpref_set_ransac(self._h, float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), float(th2))

    def thresholds(self):
        e = np.zeros(max(self.n, 1), np.float32)
        self._L.pnpref_thresholds(self._h, _p(e))
        return e[:self.n]

    def use_sets(self, sets):
        self.sets = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
        self.table = np.zeros(max(0 if self.sets is None else len(self.sets), 1), dtype=HYP_DTYPE)

    def iterate(self, n_iterations, stop_on_refine=True):
        """the result dict with "rc" (0, or -4: the call would pass the sets, state untouched)"""
        res = OrbpResult()
        inl = np.zeros(max(self.n_all, 1), dtype=np.uint8)
        rc = self._L.pnpref_iterate(self._h, int(n_iterations), _p(self.sets), 0 if self.sets is None else len(self.sets), C.byref(res), _p(inl),
                                    _p(self.table), int(stop_on_refine))
        r = result_fields(res, inl[:self.n_all])
        r["rc"] = rc
        return r

    def find(self):
        return self.iterate(self.max_iterations)

    def compute_pose(self, sel):
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        R, t = np.zeros((3, 3)), np.zeros(3)
        err = self._L.pnpref_compute_pose(self._h, _p(sel), len(sel), _p(R), _p(t))
        return err, R, t

    def all_hypotheses(self):
        """the table of EVERY hypothesis of the sets, from a fresh copy of this solver that never returns early"""
        full = RefSolver(self.case)
        full.set_ransac(*self.case["ransac"])
        if full.n < full.min_inliers:
            return full_table_empty()
        full.use_sets(self.sets)
        full.iterate(len(self.sets), stop_on_refine=False)   # (fewer sets than mRansacMaxIts: stops at the last one, table written)
        return full.table[:len(self.sets)]


def full_table_empty():
    return np.zeros(0, dtype=HYP_DTYPE)


# ------------------------------------------------------------------------------------------------ scenes
def make_case(rng, n=100, R=None, t=None, shape="general", depth=(4.0, 9.0), wrong=0.0, noise=0.0, behind=0, octaves=1, ransac=TRACKING, n_all=None):
    """n correspondences of a frame with pose Xc = R Xw + t.  shape: general | planar | collinear (the camera-frame layout).
    depth: the range of camera depths.  wrong: the share of matches whose keypoint is replaced by a random image point.
    noise: pixel noise (sigma, scaled by the octave's factor).  behind: that many points are mirrored behind the camera
    (their keypoints stay where the mirrored point projects).  octaves: levels the keypoints are spread over."""
    R = rot_axis_angle([0.3, 1, 0.2], 0.5) if R is None else R
    t = np.array([0.4, -0.2, 0.3]) if t is None else np.asarray(t, dtype=np.float64)
    z = rng.uniform(depth[0], depth[1], n)
    if shape == "general":
        Xc = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], axis=1)
    elif shape == "planar":
        xy = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)], axis=1)
        Xc = np.concatenate([xy, (6.0 + 0.3 * xy[:, :1] - 0.2 * xy[:, 1:])], axis=1)
    elif shape == "collinear":
        a = rng.uniform(-2, 2, n)
        Xc = np.array([0.2, -0.1, 6.0]) + a[:, None] * np.array([1.0, 0.4, 0.5]) + rng.normal(0, 1e-3, (n, 3))
    else:
        raise ValueError(shape)
    if behind:
        Xc[:behind] = -Xc[:behind]
    f = np.float32
    Xw = ((Xc - t) @ R).astype(f)                      # R^T (Xc - t), row-wise
    Xc = Xw.astype(np.float64) @ R.T + t               # (the keypoints see the float32 map points)
    K = K_TUM.astype(np.float64)
    uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)
    level = rng.integers(0, octaves, n)
    if noise:
        uv = uv + rng.normal(0, noise, uv.shape) * np.sqrt(SIGMA2[level].astype(np.float64))[:, None]
    if wrong:
        bad = rng.choice(n, int(round(wrong * n)), replace=False)
        uv[bad] = np.stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))], axis=1)
    n_all = int(n * 1.5) + 3 if n_all is None else n_all
    idx = np.sort(rng.choice(n_all, n, replace=False)).astype(np.int32)
    case = dict(n_all=n_all, idx=idx, P2D=uv.astype(f), sigma2=SIGMA2[level], P3Dw=Xw, K=K_TUM, ransac=ransac)
    case["true"] = dict(R=R, t=t)
    return case


# name -> (kwargs of make_case, exact: a noiseless volumetric scene, the true pose must come back)
FAMILIES = {
    "general": (dict(n=100), True),
    "planar": (dict(n=100, shape="planar"), False),
    "near_collinear": (dict(n=60, shape="collinear"), False),
    "far": (dict(n=100, depth=(40.0, 90.0), t=[0.5, 0.2, 20.0]), True),
    "near": (dict(n=100, depth=(0.3, 1.2), t=[0.05, -0.02, 0.1]), True),
    "wrong_20": (dict(n=200, wrong=0.2, noise=0.5), False),
    "wrong_40": (dict(n=200, wrong=0.4, noise=0.5), False),
    "wrong_60": (dict(n=200, wrong=0.6, noise=0.5), False),
    "behind_camera": (dict(n=80, behind=10), False),
    "n_below_min": (dict(n=7), False),
    "n_equal_min": (dict(n=10), False),
    "mixed_octaves": (dict(n=150, octaves=8, noise=0.3), False),
    "defaults": (dict(n=100, ransac=DEFAULTS), True),
}


def family_case(name, seed=0, **over):
    kw, _ = FAMILIES[name]
    kw = dict(kw)
    kw.update(over)
    return make_case(np.random.default_rng(1000 * (sorted(FAMILIES).index(name) + 1) + seed), **kw)


def case_sets(case, count, seed=0):
    """the sets of a case, drawn as the reference draws them (repeated points included); None below 4 points"""
    n = case["idx"].shape[0]
    return make_pnp_sets(n, count, seed=seed) if n >= 4 else None


def ref_solve(case, sets=None, seed=0):
    """a RefSolver with the case's RANSAC parameters and its sets installed (max_iterations + EXTRA_SETS by default)"""
    s = RefSolver(case)
    s.set_ransac(*case["ransac"])
    s.use_sets(case_sets(case, s.max_iterations + EXTRA_SETS, seed) if sets is None else sets)
    return s


def replay(solver, step):
    """iterate(step) until bNoMore or until mnIterations has reached mRansacMaxIts (a call that returns through Refine
    does not set bNoMore, however far it has run): the list of result dicts"""
    outs = []
    for _ in range(100000):
        r = solver.iterate(step)
        assert r.get("rc", 0) == 0, {k: v for k, v in r.items() if k != "inliers"}
        outs.append(r)
        if r["no_more"] or r["iterations"] >= solver.max_iterations:
            return outs
    raise AssertionError("iterate never ran out")


# ------------------------------------------------------------------------------------------------ float64 check
def check64(case, out):
    """a returned result against float64 geometry: (rotation error [rad], relative t error) against the case's true pose,
    and (disagreements outside the band, share of band points, the widest |err32-ish margin| among disagreeing points) of
    the mask against a float64 recount under the returned Tcw"""
    d = np.float64
    tr = case["true"]
    T = out["Tcw"].astype(d)
    R, t = T[:3, :3], T[:3, 3]
    A = R.T @ tr["R"]   # the angle from the skew part as well: arccos alone cannot resolve below 1e-4 rad of a float32 matrix
    ang = np.arctan2(np.linalg.norm([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]]) / 2, (np.trace(A) - 1) / 2)
    pose = (float(ang), float(np.linalg.norm(t - tr["t"]) / (1 + np.linalg.norm(tr["t"]))))
    Xc = case["P3Dw"].astype(d) @ R.T + t
    K = case["K"].astype(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)
        e = ((case["P2D"].astype(d) - uv) ** 2).sum(axis=1)
        th = case["sigma2"].astype(d) * d(np.float32(case["ransac"][5]))
        want = e < th
        rel = np.abs(e - th) / th
    band = rel <= BAND_REL
    got = out["inliers"][case["idx"]]
    dis = want != got
    worst = float(np.nanmax(np.where(dis, np.nan_to_num(rel, nan=np.inf), 0.0))) if dis.any() else 0.0
    return pose, (int((dis & ~band).sum()), float(band.mean()), worst)


def band_width(case, out):
    """the float32 rounding of error2 as a share of its threshold, over the points with err < 4 th: max |err32 - err64| / th,
    err32 from a float32 numpy mirror of CheckInliers under the returned pose's float64 source is not available here, so
    the returned CV_32F Tcw is used on both sides (the mirror's widths: Xc, Yc, invZc, the differences and error2 float)"""
    d, f = np.float64, np.float32
    T = out["Tcw"].astype(d)
    R, t = T[:3, :3], T[:3, 3]
    X = case["P3Dw"].astype(d)
    K = case["K"].astype(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        Xc = X @ R.T + t
        uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)
        e64 = ((case["P2D"].astype(d) - uv) ** 2).sum(axis=1)
        xc, yc, iz = Xc[:, 0].astype(f), Xc[:, 1].astype(f), (1 / Xc[:, 2]).astype(f)
        ue = K[2] + K[0] * xc.astype(d) * iz.astype(d)
        ve = K[3] + K[1] * yc.astype(d) * iz.astype(d)
        dx, dy = (case["P2D"][:, 0].astype(d) - ue).astype(f), (case["P2D"][:, 1].astype(d) - ve).astype(f)
        e32 = f(f(dx * dx) + f(dy * dy))
        th = case["sigma2"].astype(d) * d(np.float32(case["ransac"][5]))
        near = e64 < 4 * th
    return float((np.abs(e32.astype(d) - e64)[near] / th[near]).max()) if near.any() else 0.0


def measure():
    """the figures at the top of this file: run as `python tests/pnp_cases.py`"""
    worst = dict(rot=(0, ""), t=(0, ""), band=(0, ""), share=(0, ""), outside=(0, ""))
    for name in sorted(FAMILIES):
        for seed in SEEDS:
            case = family_case(name, seed)
            s = ref_solve(case, seed=seed)
            for r in replay(s, 5):
                if not r["returned"]:
                    continue
                (rot, te), (outside, share, _) = check64(case, r)
                bw = band_width(case, r)
                tag = "%s/%d" % (name, seed)
                if FAMILIES[name][1]:
                    worst["rot"] = max(worst["rot"], (rot, tag))
                    worst["t"] = max(worst["t"], (te, tag))
                worst["band"] = max(worst["band"], (bw, tag))
                worst["share"] = max(worst["share"], (share, tag))
                worst["outside"] = max(worst["outside"], (outside, tag))
    for k, v in worst.items():
        print("%-8s %.3e  %s" % (k, v[0], v[1]))


# ------------------------------------------------------------------------------------------------ device against restatement
RESULT_BITS = ("Tcw", "best_Tcw", "inliers")
RESULT_INTS = ("returned", "no_more", "n_inliers", "hypothesis", "refined", "iterations", "best_inliers", "best_hypothesis")
TABLE_FIELDS = ("n_inliers", "is_record", "refine_inliers", "refine_ok", "R", "t", "refine_R", "refine_t")


def device_solver(matcher, case):
    from orbslamm_amd.pnp import PnPsolver
    s = PnPsolver(matcher, case["n_all"], case["idx"], case["P2D"], case["sigma2"], case["P3Dw"], case["K"])
    s.set_ransac(*case["ransac"])
    return s


def assert_same_table(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in TABLE_FIELDS:
        if not same(got[k], want[k]):
            bad = [i for i in range(len(got)) if not same(got[k][i], want[k][i])]
            raise AssertionError("%s: %s differs at hypotheses %s: device %r restatement %r" % (what, k, bad[:8], got[k][bad[0]], want[k][bad[0]]))


def assert_same_result(got, want, what=""):
    for k in RESULT_INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in RESULT_BITS:
        assert same(got[k], want[k]), (what, k, got[k], want[k])


def compare_solver(dev, case, sets, step, what=""):
    """a device solver that has run `sets` against the restatement: the whole table as bits, then iterate(step) to
    the end of a replay (see replay), every field of every call as bits.  Returns the restatement's results."""
    ref = ref_solve(case, sets=sets)
    assert dev.max_iterations == ref.max_iterations and dev.min_inliers == ref.min_inliers, (what, dev.max_iterations, ref.max_iterations)
    assert_same_table(dev.hypotheses(), ref.all_hypotheses(), what)
    outs = []
    for call in range(100000):
        g, w = dev.iterate(step), ref.iterate(step)
        assert w["rc"] == 0, (what, call)
        assert_same_result(g, w, "%s call %d" % (what, call))
        outs.append(w)
        if w["no_more"] or w["iterations"] >= ref.max_iterations:
            return outs
    raise AssertionError("iterate never ran out")


if __name__ == "__main__":
    measure()
