"""Initializer (src/Initializer.cc) on the device: the H / F RANSAC and the two-view reconstruction of monocular map
initialisation, over the orbi_* block of include/orbslamm_hip.h.

    ini = Initializer(matcher, keys1_un | frame, K, sigma=1.0, iterations=200, model="HF" | "F")
    out = ini.initialize(keys2_un | frame, matches12)          # sets drawn by make_sets, as the reference draws them

model "HF" is SingleRobotScenario's Initializer, "F" MultipleRobotsScenario's (ReconstructF only)."""
import ctypes as C

import numpy as np

from ._lib import K4, KP_DTYPE, RAND_MAX, check, lib, ptr, random_int, seed_rand  # noqa: F401 (RAND_MAX: part of this module's names)
from ._solver import Handle

ORBI_MODEL_HF, ORBI_MODEL_F = 0, 1
MAX_ITERATIONS = 4096
MAX_FEATURES = 65535


class OrbiResult(C.Structure):
    _fields_ = [("ok", C.c_int32), ("reconstructed_h", C.c_int32), ("rt_state", C.c_int32), ("R21", C.c_float * 9), ("t21", C.c_float * 3),
                ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float), ("H21", C.c_float * 9), ("F21", C.c_float * 9),
                ("it_H", C.c_int32), ("it_F", C.c_int32), ("inliers_H", C.c_int32), ("inliers_F", C.c_int32),
                ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("n_candidates", C.c_int32), ("best", C.c_int32),
                ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8)]


def result_fields(r):
    """an OrbiResult (or anything with its layout) as a dict of numpy values (float32 arrays, ints)"""
    out = {}
    for name, t in OrbiResult._fields_:
        v = getattr(r, name)
        out[name] = np.array(v[:], dtype=np.float32 if t._type_ == C.c_float else np.int32) if hasattr(t, "_length_") else \
            (np.float32(v) if t == C.c_float else int(v))
    return out


def make_sets(n, iterations, seed=0):
    """Initialize's set drawing (Initializer.cc:67-97) through libc's rand(), as DUtils::Random makes it: SeedRandOnce(seed)
    is srand(seed) (seed None: continue the process's stream), RandomInt(0, k - 1) = int(rand() / (RAND_MAX + 1.0) * k).
    Returns iterations x 8 indices into the compacted match list."""
    if n < 8:
        raise ValueError("%d matches: the 8-point sets need at least 8" % n)
    seed_rand(seed)
    sets = np.zeros((iterations, 8), dtype=np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = random_int(len(avail))
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


class Initializer(Handle):
    """Initializer(ReferenceFrame, sigma, iterations) on a matcher's device and stream; the reference frame is mvKeysUn
    (KP_DTYPE records) or a device-resident frame (ORBmatcher.frame_from_device)."""
    _destroy = "orbi_destroy"

    def __init__(self, matcher, ref, K, sigma=1.0, iterations=200, model="HF"):
        self._L = lib()
        self.matcher = matcher   # (keeps the handle alive)
        self.iterations = int(iterations)
        self.model = {"HF": ORBI_MODEL_HF, "F": ORBI_MODEL_F}[model]
        self._h = C.c_void_p()
        k4 = K4(K)
        if isinstance(ref, np.ndarray):
            keys = np.ascontiguousarray(ref, dtype=KP_DTYPE)
            check(self._L.orbi_create(matcher._h, ptr(keys), keys.shape[0], ptr(k4), float(sigma), self.iterations, self.model, C.byref(self._h)))
        else:
            check(self._L.orbi_create_frame(matcher._h, ref, ptr(k4), float(sigma), self.iterations, self.model, C.byref(self._h)))
        n = C.c_int(0)
        check(self._L.orbi_size(self._h, C.byref(n)))
        self.n1 = n.value

    def normalization(self):
        """frame 1's Normalize: (meanX, meanY, sX, sY)"""
        out = np.zeros(4, dtype=np.float32)
        check(self._L.orbi_normalization(self._h, ptr(out)))
        return out

    def initialize(self, cur, matches12, sets=None):
        """Initialize(CurrentFrame, vMatches12, ...): cur is mvKeysUn (KP_DTYPE) or a device-resident frame; sets default to
        make_sets over the matches.  Returns dict(ok, R21 (3x3), t21 (3), p3d (n1 x 3), triangulated (n1, bool), res):
        p3d / triangulated are zeros unless ok (the reference leaves its vectors untouched then); res holds every field
        of OrbiResult (result_fields)."""
        m12 = np.ascontiguousarray(matches12, dtype=np.int32)
        if m12.shape[0] != self.n1:
            raise ValueError("matches12 has %d entries, frame 1 %d keys" % (m12.shape[0], self.n1))
        if sets is None:
            sets = make_sets(int((m12 >= 0).sum()), self.iterations)
        sets = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1)
        if sets.shape[0] != self.iterations * 8:
            raise ValueError("sets: %d entries, want %d" % (sets.shape[0], self.iterations * 8))
        res = OrbiResult()
        p3d = np.zeros((max(self.n1, 1), 3), dtype=np.float32)
        tri = np.zeros(max(self.n1, 1), dtype=np.uint8)
        if isinstance(cur, np.ndarray):
            keys = np.ascontiguousarray(cur, dtype=KP_DTYPE)
            check(self._L.orbi_initialize(self._h, ptr(keys), keys.shape[0], ptr(m12), ptr(sets), C.byref(res), ptr(p3d), ptr(tri)))
        else:
            check(self._L.orbi_initialize_frame(self._h, cur, ptr(m12), ptr(sets), C.byref(res), ptr(p3d), ptr(tri)))
        r = result_fields(res)
        return dict(ok=bool(res.ok), R21=r["R21"].reshape(3, 3), t21=r["t21"], p3d=p3d[:self.n1], triangulated=tri[:self.n1].astype(bool), res=r)
