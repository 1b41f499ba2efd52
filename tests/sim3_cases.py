"""The Sim3Solver's checker for the tests: the C++ restatement (tools/sim3_ref.hpp) built with g++ -ffp-contract=off
behind a small C shim (tests/cpp/sim3_ref_capi.cpp), named scene families with their true Sim3, and a float64 numpy
check of a returned result that shares no code with the restatement."""
import ctypes as C
import os

import numpy as np

from ref_shim import cached_shim, p as _p, rot_axis_angle, same
from orbslamm_amd.sim3 import HYP_DTYPE, OrbsResult, make_sim3_sets, result_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TUM = np.array([517.3, 516.5, 318.6, 255.3], dtype=np.float32)
K_B = np.array([535.4, 539.2, 320.1, 247.6], dtype=np.float32)
SIGMA2 = np.array([np.float32(1.2) ** (2 * l) for l in range(8)], dtype=np.float32)   # (the tests' stand-in for mvLevelSigma2)

# Tolerances of the float64 check, MEASURED from the restatement on the CPU over seeds 0..9 of every family (find's
# return for the pose, every return of an iterate-to-exhaustion replay for the mask: 28 989 returns), then given a margin
# of 4x for their dependence on conditioning:
#   rotation error of a noiseless family   measured max 4.25e-5 rad  (planar: a near-collinear minimal set)
#   |t - t_true| / (1 + |t_true|)          measured max 1.53e-4     (planar)
#   |s - s_true| / s_true                  measured max 4.94e-7     (scale_5)
#   the float32 rounding band of err against its threshold: |err32 - err64| / th over the points of the outlier
#   families with err < 4 th                measured max 5.04e-5     (err is a squared pixel distance of float projections)
# No mask of those returns disagreed with the float64 recount outside (or inside) the band; the closest any point came to
# its threshold was 4.5e-3 th, so no seed of 0..9 leaves a point undecided: the 2 % cap holds with room.
TOL_ROT = 4 * 4.25e-5
TOL_T = 4 * 1.53e-4
TOL_S = 4 * 4.94e-7
BAND_REL = 4 * 5.04e-5
BAND_SHARE_CAP = 0.02   # the share of a case's points that may fall inside the band (undecided)
SEEDS = range(10)       # the seeds measured; the tests use these

def _declare(L):
    vp = C.c_void_p
    L.sim3ref_eigen.argtypes = [vp, vp, vp]
    L.sim3ref_rodrigues.argtypes = [vp, vp]
    L.sim3ref_draw_sets.argtypes = [C.c_int, C.c_int, vp]
    L.sim3ref_create.argtypes = [C.c_int, vp, C.c_int] + [vp] * 10 + [C.c_int]
    L.sim3ref_create.restype = vp
    L.sim3ref_destroy.argtypes = [vp]
    L.sim3ref_destroy.restype = None
    L.sim3ref_set_ransac.argtypes = [vp, C.c_double, C.c_int, C.c_int]
    L.sim3ref_max_iterations.argtypes = [vp]
    L.sim3ref_iterate.argtypes = [vp, C.c_int, vp, C.POINTER(OrbsResult), vp, vp]
    L.sim3ref_thresholds.argtypes = [vp, vp, vp]
    L.sim3ref_compute.argtypes = [vp, vp, C.c_int, vp]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("sim3_ref", _declare)


def ref_eigen(a):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(4, 4)
    w, v = np.zeros(4, np.float32), np.zeros((4, 4), np.float32)
    ref_lib().sim3ref_eigen(_p(a), _p(w), _p(v))
    return w, v


def ref_rodrigues(v):
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(3)
    R = np.zeros((3, 3), np.float32)
    ref_lib().sim3ref_rodrigues(_p(v), _p(R))
    return R


def ref_draw_sets(n, iterations):
    out = np.zeros((iterations, 3), np.int32)
    ref_lib().sim3ref_draw_sets(n, iterations, _p(out))
    return out


def ref_compute(P1, P2, fix_scale):
    """ComputeSim3 on two 3x3 float32 matrices, one point per column"""
    P1 = np.ascontiguousarray(P1, dtype=np.float32).reshape(3, 3)
    P2 = np.ascontiguousarray(P2, dtype=np.float32).reshape(3, 3)
    o = np.zeros(49, np.float32)
    ref_lib().sim3ref_compute(_p(P1), _p(P2), int(fix_scale), _p(o))
    return dict(T12=o[:16].reshape(4, 4), T21=o[16:32].reshape(4, 4), R=o[32:41].reshape(3, 3), t=o[41:44], s=o[44], quat=o[45:49])


class RefSolver:
    """the restatement's Sim3Solver with the interface of orbslamm_amd.sim3.Sim3Solver (sets always given)"""

    def __init__(self, case):
        self._L = ref_lib()
        self.case = case
        self.n, self.n1 = case["idx1"].shape[0], case["n1"]
        a = [np.ascontiguousarray(case[k], dtype=np.float32) for k in ("X1w", "X2w", "Rcw1", "tcw1", "Rcw2", "tcw2", "K1", "K2", "sigma2_1", "sigma2_2")]
        idx1 = np.ascontiguousarray(case["idx1"], dtype=np.int32)
        self._h = self._L.sim3ref_create(self.n1, _p(idx1), self.n, *[_p(x) for x in a], int(case["fix_scale"]))
        self.sets = None
        self.table = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.sim3ref_destroy(self._h)
            self._h = None

    @property
    def max_iterations(self):
        return self._L.sim3ref_max_iterations(self._h)

    def set_ransac(self, probability=0.99, min_inliers=6, max_iterations=300):
        self._L.sim3ref_set_ransac(self._h, float(probability), int(min_inliers), int(max_iterations))
        self.table = None

    def thresholds(self):
        e1, e2 = np.zeros(max(self.n, 1), np.float32), np.zeros(max(self.n, 1), np.float32)
        self._L.sim3ref_thresholds(self._h, _p(e1), _p(e2))
        return e1[:self.n], e2[:self.n]

    def use_sets(self, sets):
        self.sets = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 3)
        self.table = np.zeros(max(self.max_iterations, 1), dtype=HYP_DTYPE)
        self.evaluated = 0

    def iterate(self, n_iterations):
        if self.table is None:
            self.use_sets(self.sets)
        res = OrbsResult()
        inl = np.zeros(max(self.n1, 1), dtype=np.uint8)
        self._L.sim3ref_iterate(self._h, int(n_iterations), _p(self.sets), C.byref(res), _p(inl), _p(self.table))
        r = result_fields(res, inl[:self.n1])
        self.evaluated = r["iterations"]
        return r

    def find(self):
        return self.iterate(self.max_iterations)

    def all_hypotheses(self):
        """the table of EVERY hypothesis, from a fresh copy of this solver (iterate stops at its first return)"""
        full = RefSolver(self.case)
        full.set_ransac(*self.case["ransac"])
        full.use_sets(self.sets)
        while not full.iterate(full.max_iterations)["no_more"]:
            pass
        return full.table[:full.max_iterations if full.n >= self.case["ransac"][1] else 0]


# ------------------------------------------------------------------------------------------------ scenes
def make_case(rng, n=100, s=1.0, R=None, t=None, fix_scale=False, shape="general", outliers=0.0, noise=0.0, identity_cameras=False,
              grid=False, ransac=(0.99, 6, 300), n1=None, behind=0, zero_depth=0):
    """n correspondences of two keyframes whose camera-frame points obey X1c = s R X2c + t.  shape: general | planar |
    collinear.  outliers: the share of correspondences whose second point is replaced by another one.  noise: relative
    3-D noise on X2c.  grid: coordinates on a 1/64 lattice with identity cameras (exact in float32).  behind / zero_depth:
    that many points get a negative / exactly zero depth in camera 2 (identity cameras).  Returns the case dict with the
    true Sim3 under "true"."""
    R = np.eye(3) if R is None else R
    t = np.array([0.4, -0.2, 0.3]) if t is None else np.asarray(t, dtype=np.float64)
    if shape == "general":
        X1c = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)], axis=1)
    elif shape == "planar":
        xy = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)], axis=1)
        X1c = np.concatenate([xy, (6.0 + 0.3 * xy[:, :1] - 0.2 * xy[:, 1:])], axis=1)
    elif shape == "collinear":
        a = rng.uniform(-2, 2, n)
        X1c = np.array([0.2, -0.1, 6.0]) + a[:, None] * np.array([1.0, 0.4, 0.5])
    else:
        raise ValueError(shape)
    if grid:
        X1c = np.round(X1c * 64) / 64
        t = np.round(t * 64) / 64
    X2c = (X1c - t) @ R / s            # R^T (X1c - t) / s, row-wise
    if noise:
        X2c = X2c * (1 + rng.normal(0, noise, X2c.shape))
    if outliers:
        bad = rng.choice(n, int(round(outliers * n)), replace=False)
        X2c[bad] = X2c[rng.permutation(bad)] + rng.normal(0, 0.5, (len(bad), 3))
    if behind:
        X2c[:behind, 2] = -np.abs(X2c[:behind, 2])
    if zero_depth:
        X2c[behind:behind + zero_depth, 2] = 0.0
    if identity_cameras or grid or behind or zero_depth:
        Rcw1, tcw1, Rcw2, tcw2 = np.eye(3), np.zeros(3), np.eye(3), np.zeros(3)
    else:
        Rcw1, tcw1 = rot_axis_angle([0.2, 1.0, -0.3], 0.7), np.array([0.5, -1.0, 2.0])
        Rcw2, tcw2 = rot_axis_angle([-0.5, 0.3, 1.0], -1.1), np.array([-3.0, 0.4, 1.0])
    X1w = (X1c - tcw1) @ Rcw1          # Rcw^T (Xc - tcw)
    X2w = (X2c - tcw2) @ Rcw2
    n1 = int(n * 1.5) + 3 if n1 is None else n1
    idx1 = np.sort(rng.choice(n1, n, replace=False)).astype(np.int32)
    f = np.float32
    case = dict(n1=n1, idx1=idx1, X1w=X1w.astype(f), X2w=X2w.astype(f), Rcw1=Rcw1.astype(f).reshape(9), tcw1=tcw1.astype(f),
                Rcw2=Rcw2.astype(f).reshape(9), tcw2=tcw2.astype(f), K1=K_TUM, K2=K_B, sigma2_1=SIGMA2[rng.integers(0, 8, n)],
                sigma2_2=SIGMA2[rng.integers(0, 8, n)], fix_scale=bool(fix_scale), ransac=ransac)
    case["true"] = dict(s=float(s), R=R, t=t)
    return case


# name -> (kwargs of make_case, noiseless: the true Sim3 must be recovered, quirk: asserted from the restatement's fields)
FAMILIES = {
    "general": (dict(n=100, s=1.3, R=rot_axis_angle([0.3, 1, 0.2], 0.5)), True, None),
    "scale_0p2": (dict(n=100, s=0.2, R=rot_axis_angle([1, 0.1, 0.2], -0.3)), True, None),
    "scale_5": (dict(n=100, s=5.0, R=rot_axis_angle([0.1, 0.2, 1], 0.4), t=[0.5, 0.2, -20.0]), True, None),
    "fixed_scale": (dict(n=100, s=1.0, R=rot_axis_angle([0.3, 1, 0.2], 0.5), fix_scale=True), True, None),
    "small_rotation": (dict(n=100, s=1.1, R=rot_axis_angle([0.3, 1, 0.2], 1e-4)), True, None),
    "near_pi": (dict(n=100, s=0.9, R=rot_axis_angle([0.05, 0.02, 1], np.pi - 1e-3), t=[0.1, 0.1, 0.2]), True, None),
    "identity_rotation": (dict(n=50, s=1.0, t=[0, 0, 0], grid=True), False, "nan"),
    "planar": (dict(n=100, s=1.2, R=rot_axis_angle([0.3, 1, 0.2], 0.3), shape="planar"), True, None),
    "collinear": (dict(n=60, s=1.0, R=rot_axis_angle([0.3, 1, 0.2], 0.3), shape="collinear", fix_scale=True), False, "any"),
    "outliers_30": (dict(n=200, s=1.3, R=rot_axis_angle([0.3, 1, 0.2], 0.5), outliers=0.3, noise=2e-3, ransac=(0.99, 20, 300)), False, None),
    "outliers_60": (dict(n=200, s=0.8, R=rot_axis_angle([1, 0.3, 0.2], -0.4), outliers=0.6, noise=2e-3, ransac=(0.99, 20, 300)), False, None),
    "n_3": (dict(n=3, s=1.3, R=rot_axis_angle([0.3, 1, 0.2], 0.5), ransac=(0.99, 2, 300)), True, None),
    "n_below_min": (dict(n=5, s=1.3, R=rot_axis_angle([0.3, 1, 0.2], 0.5)), False, "no_more"),
    "n_equal_min": (dict(n=10, s=1.3, R=rot_axis_angle([0.3, 1, 0.2], 0.5), ransac=(0.99, 10, 300)), False, "any"),
    "behind_camera": (dict(n=80, s=1.0, R=rot_axis_angle([0.3, 1, 0.2], 0.2), behind=10, ransac=(0.99, 20, 300)), False, None),
    "zero_depth": (dict(n=80, s=1.0, R=rot_axis_angle([0.3, 1, 0.2], 0.2), zero_depth=3, ransac=(0.99, 20, 300)), False, None),
}


def family_case(name, seed=0, **over):
    kw, _, _ = FAMILIES[name]
    kw = dict(kw)
    kw.update(over)
    return make_case(np.random.default_rng(1000 * (sorted(FAMILIES).index(name) + 1) + seed), **kw)


def case_sets(case, iterations, seed=0):
    """the sets of a case, drawn as the reference draws them (repeated points included); None below 3 points"""
    n = case["idx1"].shape[0]
    return make_sim3_sets(n, iterations, seed=seed) if n >= 3 else None


def ref_solve(case, sets=None, seed=0):
    """a RefSolver with the case's RANSAC parameters and its sets installed"""
    s = RefSolver(case)
    s.set_ransac(*case["ransac"])
    s.use_sets(case_sets(case, s.max_iterations, seed) if sets is None else sets)
    return s


# ------------------------------------------------------------------------------------------------ float64 check
def check64(case, out):
    """a returned result against float64 geometry: (rotation error [rad], relative t error, relative s error) against the
    case's true Sim3, and (disagreements outside the band, share of band points, the largest |err64 - th| / th among
    disagreeing points) of the mask against a float64 recount under the returned T12"""
    d = np.float64
    tr = case["true"]
    T = out["T12"].astype(d)
    sR, t = T[:3, :3], T[:3, 3]
    s = np.cbrt(np.linalg.det(sR))
    R = sR / s
    cosang = np.clip((np.trace(R.T @ tr["R"]) - 1) / 2, -1, 1)
    pose = (float(np.arccos(cosang)), float(np.linalg.norm(t - tr["t"]) / (1 + np.linalg.norm(tr["t"]))), float(abs(s - tr["s"]) / tr["s"]))
    X1c = case["X1w"].astype(d) @ case["Rcw1"].astype(d).reshape(3, 3).T + case["tcw1"].astype(d)
    X2c = case["X2w"].astype(d) @ case["Rcw2"].astype(d).reshape(3, 3).T + case["tcw2"].astype(d)

    def pin(X, K):
        K = K.astype(d)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)
    p1, p2 = pin(X1c, case["K1"]), pin(X2c, case["K2"])
    Tinv = np.linalg.inv(T)
    with np.errstate(invalid="ignore"):
        e1 = ((p1 - pin(X2c @ sR.T + t, case["K1"])) ** 2).sum(axis=1)
        e2 = ((pin(X1c @ Tinv[:3, :3].T + Tinv[:3, 3], case["K2"]) - p2) ** 2).sum(axis=1)
    th1 = np.floor(9.210 * case["sigma2_1"].astype(d))
    th2 = np.floor(9.210 * case["sigma2_2"].astype(d))
    with np.errstate(invalid="ignore"):
        want = (e1 < th1) & (e2 < th2)
        r1, r2 = np.abs(e1 - th1) / th1, np.abs(e2 - th2) / th2
    band = (r1 <= BAND_REL) | (r2 <= BAND_REL)
    got = out["inliers"][case["idx1"]]
    dis = want != got
    worst = float(np.nanmax(np.where(dis, np.minimum(np.nan_to_num(r1, nan=np.inf), np.nan_to_num(r2, nan=np.inf)), 0.0))) if dis.any() else 0.0
    return pose, (int((dis & ~band).sum()), float(band.mean()), worst)


# ------------------------------------------------------------------------------------------------ device against restatement
RESULT_BITS = ("T12", "best_R", "best_t", "best_s", "inliers")
RESULT_INTS = ("returned", "no_more", "n_inliers", "hypothesis", "iterations", "best_inliers", "has_best")


def device_solver(matcher, case):
    from orbslamm_amd.sim3 import Sim3Solver
    s = Sim3Solver(matcher, case["n1"], case["idx1"], case["X1w"], case["X2w"], case["Rcw1"], case["tcw1"], case["Rcw2"], case["tcw2"],
                   case["K1"], case["K2"], case["sigma2_1"], case["sigma2_2"], case["fix_scale"])
    s.set_ransac(*case["ransac"])
    return s


def assert_same_table(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in ("n_inliers", "s12", "T12", "R12", "t12"):
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
    exhaustion, every field of every call as bits.  Returns the restatement's results."""
    ref = ref_solve(case, sets=sets)
    assert dev.max_iterations == ref.max_iterations, (what, dev.max_iterations, ref.max_iterations)
    assert_same_table(dev.hypotheses(), ref.all_hypotheses(), what)
    outs = []
    for call in range(10000):
        g, w = dev.iterate(step), ref.iterate(step)
        assert_same_result(g, w, "%s call %d" % (what, call))
        outs.append(w)
        if w["no_more"]:
            return outs
    raise AssertionError("iterate never ran out")
