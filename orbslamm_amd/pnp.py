"""PnPsolver (src/PnPsolver.cc) on the device: EPnP under RANSAC with an n-point Refine for the relocalisation candidates
of a lost frame, over the orbp_* block of include/orbslamm_hip.h.

    s = PnPsolver(matcher, n_all, idx, P2D, sigma2, P3Dw, K)
    s.set_ransac(0.99, 10, 300, 4, 0.5, 5.991)
    run_all([s, ...])                  # one device call for all of a frame's candidates (or s.run())
    out = s.iterate(5)                 # the reference's iterate; s.find() is iterate(max_iterations)

The sets are drawn by make_pnp_sets as the reference draws them (its draw can repeat a point)."""
import ctypes as C

import numpy as np

from ._lib import K4, check, lib, ptr
from ._solver import RansacHandle, draw_sets, f32 as _f32, given_sets, run_batch

MAX_POINTS = 65535
MAX_ITERATIONS = 4096
EXTRA_SETS = 4   # iterate's loop is an OR: iterate(5) can evaluate hypotheses up to max_iterations + 3


class OrbpHypothesis(C.Structure):
    _fields_ = [("n_inliers", C.c_int32), ("is_record", C.c_int32), ("refine_inliers", C.c_int32), ("refine_ok", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("refine_R", C.c_double * 9), ("refine_t", C.c_double * 3)]


class OrbpResult(C.Structure):
    _fields_ = [("returned", C.c_int32), ("no_more", C.c_int32), ("n_inliers", C.c_int32), ("hypothesis", C.c_int32),
                ("refined", C.c_int32), ("iterations", C.c_int32), ("best_inliers", C.c_int32), ("best_hypothesis", C.c_int32),
                ("Tcw", C.c_float * 16), ("best_Tcw", C.c_float * 16)]


HYP_DTYPE = np.dtype([("n_inliers", "<i4"), ("is_record", "<i4"), ("refine_inliers", "<i4"), ("refine_ok", "<i4"), ("R", "<f8", (3, 3)),
                      ("t", "<f8", (3,)), ("refine_R", "<f8", (3, 3)), ("refine_t", "<f8", (3,))])
assert HYP_DTYPE.itemsize == C.sizeof(OrbpHypothesis) == 208
assert C.sizeof(OrbpResult) == 160


def result_fields(r, inliers):
    """an OrbpResult (or anything with its layout) and the mask as a dict of numpy values"""
    return dict(returned=bool(r.returned), no_more=bool(r.no_more), n_inliers=int(r.n_inliers), hypothesis=int(r.hypothesis),
                refined=bool(r.refined), iterations=int(r.iterations), best_inliers=int(r.best_inliers),
                best_hypothesis=int(r.best_hypothesis), Tcw=np.array(r.Tcw[:], dtype=np.float32).reshape(4, 4),
                best_Tcw=np.array(r.best_Tcw[:], dtype=np.float32).reshape(4, 4), inliers=inliers.astype(bool))


def make_pnp_sets(n, iterations, seed=0):
    """iterate's set drawing (PnPsolver.cc:191-201; _solver.draw_sets): iterations x 4 indices into the solver's
    correspondences; seed None continues the process's rand() stream"""
    return draw_sets(n, 4, iterations, seed)


class PnPsolver(RansacHandle):
    """PnPsolver(F, vpMapPointMatches) after its pointer chasing, on a matcher's device and stream: the n usable
    correspondences with idx their positions in vpMapPointMatches (n_all long)."""
    _destroy, _max_iterations = "orbp_destroy", "orbp_max_iterations"

    def __init__(self, matcher, n_all, idx, P2D, sigma2, P3Dw, K, frame=None, level_sigma2=None):
        """frame (an opaque device-resident frame of this matcher's device) with level_sigma2: P2D and sigma2 are gathered
        from the frame's undistorted keys on the device (orbp_create_frame); n_all, P2D and sigma2 are then ignored"""
        self._L = lib()
        self.matcher = matcher   # (keeps the handle alive)
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = idx.shape[0]
        self._h = C.c_void_p()
        if frame is None:
            self.n, self.n_all = n, int(n_all)
            args = [_f32(P2D, (n, 2)), _f32(sigma2, n), _f32(P3Dw, (n, 3)), K4(K)]
            check(self._L.orbp_create(matcher._h, self.n_all, ptr(idx), n, *[ptr(a) for a in args], C.byref(self._h)))
        else:
            lev = _f32(level_sigma2, -1)
            check(self._L.orbp_create_frame(matcher._h, frame, ptr(idx), n, ptr(_f32(P3Dw, (n, 3))), ptr(lev), lev.shape[0], ptr(K4(K)),
                                            C.byref(self._h)))
            a, b = C.c_int(0), C.c_int(0)
            check(self._L.orbp_size(self._h, C.byref(a), C.byref(b)))
            self.n, self.n_all = a.value, b.value
        self.sets = None

    @property
    def min_inliers(self):
        """mRansacMinInliers"""
        v = C.c_int(0)
        check(self._L.orbp_min_inliers(self._h, C.byref(v)))
        return v.value

    def set_ransac(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        """SetRansacParameters"""
        check(self._L.orbp_set_ransac(self._h, float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), float(th2)))
        self.sets = None

    def run(self, sets=None):
        """every hypothesis of this solver in one device call (see run_all)"""
        run_all([self], None if sets is None else [sets])

    def extend(self, sets):
        """more hypotheses behind the table of a solver that has iterated (see run_all)"""
        run_all([self], [sets], extend=True)

    def hypotheses(self):
        """the table of the runs so far: a HYP_DTYPE record per hypothesis"""
        out = np.zeros(max(1, 0 if self.sets is None else len(self.sets)), dtype=HYP_DTYPE)
        k = C.c_int(0)
        check(self._L.orbp_hypotheses(self._h, ptr(out), out.shape[0], C.byref(k)))
        return out[:k.value].copy()

    def last_run_ms(self):
        """the last run: (whole chain on the host's clock, fit, score + records, Refine on the device's)"""
        ms = np.zeros(4, dtype=np.float64)
        check(self._L.orbp_last_run_ms(self._h, ptr(ms)))
        return ms

    def iterate(self, n_iterations):
        """iterate(nIterations, bNoMore, vbInliers, nInliers): dict(returned, no_more, n_inliers, inliers (n_all, bool), Tcw,
        hypothesis, refined, iterations, best_inliers, best_hypothesis, best_Tcw)"""
        res = OrbpResult()
        inl = np.zeros(max(self.n_all, 1), dtype=np.uint8)
        check(self._L.orbp_iterate(self._h, int(n_iterations), C.byref(res), ptr(inl)))
        return result_fields(res, inl[:self.n_all])

    def find(self):
        return self.iterate(self.max_iterations)


def run_all(solvers, sets=None, extend=False):
    """orbp_run for a list of solvers of one matcher: every hypothesis of every solver in one chain of launches.  sets:
    per solver k x 4 indices, k >= 1 (default: make_pnp_sets of max_iterations + EXTRA_SETS continuing the process's rand()
    stream, solver by solver in list order); kept as solver.sets.  extend: the solvers have iterated and the sets given are
    those of the hypotheses BEHIND their tables (orbp_run continues a table, the state kept); solver.sets grows."""
    if not solvers:
        return
    keep = []
    for i, s in enumerate(solvers):
        a = given_sets(sets, i)
        if a is not None:
            if a.shape[0] % 4:
                raise ValueError("sets[%d]: %d entries, not a multiple of 4" % (i, a.shape[0]))
        elif s.n >= s.min_inliers:
            a = make_pnp_sets(s.n, s.max_iterations + EXTRA_SETS, seed=None).reshape(-1)
        keep.append(a)
    counts = np.array([0 if a is None else a.shape[0] // 4 for a in keep], dtype=np.int32)
    run_batch(solvers[0]._L.orbp_run, solvers, keep, 4, extend, ptr(counts))
