"""What the solver mirrors (initializer.py, sim3.py, pnp.py) share: the float32 argument helper, the handle's life cycle,
the RANSAC set drawing of Sim3Solver and PnPsolver, and the call behind their run_all."""
import ctypes as C

import numpy as np

from ._lib import check, ptr, random_int, seed_rand


def f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))


def draw_sets(n, k, iterations, seed):
    """iterate's set drawing (Sim3Solver.cc:163-177, PnPsolver.cc:191-201) through libc's rand(), as
    DUtils::Random::RandomInt makes it (int(rand() / (RAND_MAX + 1.0) * k)); seed None continues the process's stream.
    The reference overwrites vAvailableIndices[idx] with idx the drawn VALUE, not the drawn position, so a set can hold a
    point twice: kept.  Returns iterations x k indices into the solver's correspondences."""
    if n < k:
        raise ValueError("%d correspondences: a set needs %d" % (n, k))
    seed_rand(seed)
    sets = np.zeros((iterations, k), dtype=np.int32)
    for it in range(iterations):
        avail = list(range(n))
        live = n
        for j in range(k):
            randi = random_int(live)
            idx = avail[randi]
            sets[it, j] = idx
            avail[idx] = avail[live - 1]
            live -= 1
    return sets


class Handle:
    """owns self._h, a handle of the library self._L, until close(); _destroy names the entry that frees it"""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._L, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RansacHandle(Handle):
    """a RANSAC solver's handle; _max_iterations names the getter of mRansacMaxIts"""
    _max_iterations = None

    @property
    def max_iterations(self):
        """mRansacMaxIts"""
        v = C.c_int(0)
        check(getattr(self._L, self._max_iterations)(self._h, C.byref(v)))
        return v.value


def given_sets(sets, i):
    """the caller's sets of solver i as one flat int32 array, or None where run_all is to draw them"""
    if sets is None or sets[i] is None:
        return None
    return np.ascontiguousarray(sets[i], dtype=np.int32).reshape(-1)


def run_batch(entry, solvers, flat, k, extend=False, *extra):
    """the family's run entry on a list of solvers and their flat set arrays (None: the solver draws nothing), kept as
    solver.sets (x k; extend: behind the sets the solver holds)"""
    for s, a in zip(solvers, flat):
        if a is not None and extend and s.sets is not None:
            s.sets = np.concatenate([s.sets, a.reshape(-1, k)])
        else:
            s.sets = None if a is None else a.reshape(-1, k)
    hs = (C.c_void_p * len(solvers))(*[s._h for s in solvers])
    ps = (C.c_void_p * len(solvers))(*[ptr(a) for a in flat])
    check(entry(hs, len(solvers), ps, *extra))
