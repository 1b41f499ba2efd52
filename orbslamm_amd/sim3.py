"""Sim3Solver (src/Sim3Solver.cc) on the device: Horn's closed-form similarity under RANSAC for loop and map-merge
candidates, over the orbs_* block of include/orbslamm_hip.h.

    s = Sim3Solver(matcher, n1, idx1, X1w, X2w, Rcw1, tcw1, Rcw2, tcw2, K1, K2, sigma2_1, sigma2_2, fix_scale)
    s.set_ransac(0.99, 10, 300)
    run_all([s, ...])                  # one device call for all of a query's candidates (or s.run())
    out = s.iterate(5)                 # the reference's iterate; s.find() is iterate(max_iterations)

The sets are drawn by make_sim3_sets as the reference draws them (its draw can repeat a point)."""
import ctypes as C

import numpy as np

from ._lib import K4, check, lib, ptr
from ._solver import RansacHandle, draw_sets, f32 as _f32, given_sets, run_batch

MAX_POINTS = 65535
MAX_ITERATIONS = 4096


class OrbsHypothesis(C.Structure):
    _fields_ = [("n_inliers", C.c_int32), ("s12", C.c_float), ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3)]


class OrbsResult(C.Structure):
    _fields_ = [("returned", C.c_int32), ("no_more", C.c_int32), ("n_inliers", C.c_int32), ("hypothesis", C.c_int32),
                ("iterations", C.c_int32), ("best_inliers", C.c_int32), ("has_best", C.c_int32), ("T12", C.c_float * 16),
                ("best_R", C.c_float * 9), ("best_t", C.c_float * 3), ("best_s", C.c_float)]


HYP_DTYPE = np.dtype([("n_inliers", "<i4"), ("s12", "<f4"), ("T12", "<f4", (4, 4)), ("R12", "<f4", (3, 3)), ("t12", "<f4", (3,))])
assert HYP_DTYPE.itemsize == C.sizeof(OrbsHypothesis) == 120


def result_fields(r, inliers):
    """an OrbsResult (or anything with its layout) and the mask as a dict of numpy values"""
    return dict(returned=bool(r.returned), no_more=bool(r.no_more), n_inliers=int(r.n_inliers), hypothesis=int(r.hypothesis),
                iterations=int(r.iterations), best_inliers=int(r.best_inliers), has_best=bool(r.has_best),
                T12=np.array(r.T12[:], dtype=np.float32).reshape(4, 4), best_R=np.array(r.best_R[:], dtype=np.float32).reshape(3, 3),
                best_t=np.array(r.best_t[:], dtype=np.float32), best_s=np.float32(r.best_s), inliers=inliers.astype(bool))


def make_sim3_sets(n, iterations, seed=0):
    """iterate's set drawing (Sim3Solver.cc:163-177; _solver.draw_sets): iterations x 3 indices into the solver's
    correspondences; seed None continues the process's rand() stream"""
    return draw_sets(n, 3, iterations, seed)


class Sim3Solver(RansacHandle):
    """Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) after its pointer chasing, on a matcher's device and stream: the n
    usable correspondences with idx1 their positions in vpMatched12 (n1 long)."""
    _destroy, _max_iterations = "orbs_destroy", "orbs_max_iterations"

    def __init__(self, matcher, n1, idx1, X1w, X2w, Rcw1, tcw1, Rcw2, tcw2, K1, K2, sigma2_1, sigma2_2, fix_scale=True):
        self._L = lib()
        self.matcher = matcher   # (keeps the handle alive)
        idx1 = np.ascontiguousarray(idx1, dtype=np.int32).reshape(-1)
        n = idx1.shape[0]
        self.n, self.n1 = n, int(n1)
        self._h = C.c_void_p()
        args = [_f32(X1w, (n, 3)), _f32(X2w, (n, 3)), _f32(Rcw1, 9), _f32(tcw1, 3), _f32(Rcw2, 9), _f32(tcw2, 3), K4(K1), K4(K2),
                _f32(sigma2_1, n), _f32(sigma2_2, n)]
        check(self._L.orbs_create(matcher._h, self.n1, ptr(idx1), n, *[ptr(a) for a in args], int(bool(fix_scale)), C.byref(self._h)))
        self.sets = None

    def set_ransac(self, probability=0.99, min_inliers=6, max_iterations=300):
        """SetRansacParameters"""
        check(self._L.orbs_set_ransac(self._h, float(probability), int(min_inliers), int(max_iterations)))
        self.min_inliers = int(min_inliers)
        self.sets = None

    def points(self):
        """the constructor's products: dict(X1c, X2c (n x 3), p1, p2 (n x 2), max_error1, max_error2 (n))"""
        rec = np.zeros((3, max(self.n, 1), 4), dtype=np.float32)
        check(self._L.orbs_points(self._h, ptr(rec)))
        rec = rec[:, :self.n]
        return dict(X1c=rec[0, :, :3].copy(), max_error1=rec[0, :, 3].copy(), X2c=rec[1, :, :3].copy(), max_error2=rec[1, :, 3].copy(),
                    p1=rec[2, :, :2].copy(), p2=rec[2, :, 2:].copy())

    def run(self, sets=None):
        """every hypothesis of this solver in one device call (see run_all)"""
        run_all([self], None if sets is None else [sets])

    def hypotheses(self):
        """the table of the last run: a HYP_DTYPE record per hypothesis"""
        out = np.zeros(max(self.max_iterations, 1), dtype=HYP_DTYPE)
        k = C.c_int(0)
        check(self._L.orbs_hypotheses(self._h, ptr(out), out.shape[0], C.byref(k)))
        return out[:k.value]

    def last_run_ms(self):
        """host-clock milliseconds of the last run's legs: (up + fit + down, host libm, up + pose + score + down)"""
        ms = np.zeros(3, dtype=np.float64)
        check(self._L.orbs_last_run_ms(self._h, ptr(ms)))
        return ms

    def iterate(self, n_iterations):
        """iterate(nIterations, bNoMore, vbInliers, nInliers): dict(returned, no_more, n_inliers, inliers (n1, bool), T12,
        hypothesis, iterations, best_inliers, has_best, best_R, best_t, best_s)"""
        res = OrbsResult()
        inl = np.zeros(max(self.n1, 1), dtype=np.uint8)
        check(self._L.orbs_iterate(self._h, int(n_iterations), C.byref(res), ptr(inl)))
        return result_fields(res, inl[:self.n1])

    def find(self):
        return self.iterate(self.max_iterations)


def run_all(solvers, sets=None):
    """orbs_run for a list of solvers of one matcher: every hypothesis of every solver in one chain of launches.  sets:
    per solver max_iterations x 3 indices (default: make_sim3_sets continuing the process's rand() stream, solver by
    solver in list order); kept as solver.sets."""
    if not solvers:
        return
    keep = []
    for i, s in enumerate(solvers):
        its = s.max_iterations
        a = given_sets(sets, i)
        if a is not None:
            if a.shape[0] != its * 3:
                raise ValueError("sets[%d]: %d entries, want %d" % (i, a.shape[0], its * 3))
        elif s.n >= 3:
            a = make_sim3_sets(s.n, its, seed=None).reshape(-1)
        keep.append(a)
    run_batch(solvers[0]._L.orbs_run, solvers, keep, 3)
