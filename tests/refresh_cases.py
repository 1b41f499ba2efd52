"""Scenes for MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth over a keyframe store (orbr_*),
shared by test_refresh_cpu.py and test_gpu_refresh.py: covis_cases' seeded random store with descriptors, centres, pool records
and reference keyframes added, a few crafted points behind it, each family named after the branch of MapPoint.cc:242-371 it
forces, and the restatement (tools/refresh_ref.hpp) behind tests/ref_shim.py."""
import ctypes as C

import numpy as np

import covis_cases as cc
from ref_shim import cached_shim, p

NO_VOTE, KF_BAD, KF_SET = cc.NO_VOTE, cc.KF_BAD, cc.KF_SET
DESCRIPTOR, NORMAL_DEPTH, BOTH = 1, 2, 3
ST_NOT_ASKED, ST_DONE, ST_BAD, ST_NO_OBSERVATION, ST_ALL_KF_BAD, ST_NO_REF, ST_LEVEL_RANGE = range(7)
MAX_OBS = 1024
NLEVELS = 8
SF = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)
BRANCHES = ["bad_point", "no_observation", "bad_kf_skipped", "all_kf_bad", "n1", "n2", "n_odd", "n_even", "tie_at_best", "duplicate_entry", "no_ref",
            "level_range", "single_observer"]
POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("desc", "u1", 32),
                        ("n_obs", "<i4"), ("n_desc", "<i4"), ("best_kf", "<i4"), ("best_idx", "<i4"), ("st_descriptor", "u1"),
                        ("st_normal_depth", "u1"), ("pad", "u1", 2)])
FLOAT_FIELDS = ("pos", "normal", "min_distance", "max_distance")
T0 = 40              # the first crafted slot


class RScene:
    """a covis_cases.Scene (entries, octaves, keyframe flags, bad points) with what the refresh reads beside it: a descriptor per
    feature, a centre per keyframe, the pool's records, mpRefKF per pool id"""

    def __init__(self, s, rng):
        self.s, self.rng = s, rng
        self.desc = rng.integers(0, 256, (s.kfcap, s.stride, 32), dtype=np.uint8)
        self.centres = rng.uniform(-4, 4, (s.kfcap, 3)).astype(np.float32)
        P = s.pool_cap
        self.pos = rng.uniform(-6, 6, (P, 3)).astype(np.float32)
        self.normal = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
        self.min_d = rng.uniform(0.1, 1, P).astype(np.float32)
        self.max_d = rng.uniform(5, 9, P).astype(np.float32)
        self.pt_desc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
        self.observed = (rng.random(P) < 0.5).astype(np.uint8)          # flags bit 1: carried, never touched
        self.ref_kf = np.full(P, -1, np.int32)
        self.named = {}                                                  # family points by name

    # ---- what covis_cases.Scene gives
    kfcap = property(lambda self: self.s.kfcap)
    stride = property(lambda self: self.s.stride)
    pool_cap = property(lambda self: self.s.pool_cap)

    def observers(self, pt):
        """the (slot, feature) observations of a point in ascending order"""
        e = self.s.entries
        k, i = np.nonzero((e == pt) & ((self.s.kf_flags & KF_SET) != 0)[:, None])
        return list(zip(k.tolist(), i.tolist()))

    def default_refs(self):
        """mpRefKF of every point: mostly one of its observers, now and then -1 or a keyframe that does not observe it"""
        slots = self.s.set_slots()
        by_pt = {}
        e = self.s.entries
        for k, i in np.argwhere((e >= 0) & ((e & NO_VOTE) == 0) & ((self.s.kf_flags & KF_SET) != 0)[:, None]):
            by_pt.setdefault(int(e[k, i]), []).append((int(k), int(i)))
        for pt in range(self.pool_cap):
            obs = by_pt.get(pt, [])
            r = self.rng.random()
            if obs and r < 0.85:
                self.ref_kf[pt] = obs[self.rng.integers(len(obs))][0]
            elif r < 0.93 and len(slots):
                self.ref_kf[pt] = slots[self.rng.integers(len(slots))]
            else:
                self.ref_kf[pt] = -1

    def pt_flags(self):
        return (self.s.pt_bad.astype(np.uint8) & 1) | (self.observed << 1)

    def pool_records(self):
        from_fields = np.zeros(self.pool_cap, np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"),
                                                       ("desc", "u1", 32), ("flags", "u1"), ("pad", "u1", 3)]))
        from_fields["pos"], from_fields["normal"] = self.pos, self.normal
        from_fields["min_distance"], from_fields["max_distance"] = self.min_d, self.max_d
        from_fields["desc"], from_fields["flags"] = self.pt_desc, self.pt_flags()
        return from_fields

    def apply(self, ids, out, with_pos):
        """what a commit leaves in the pool: the DONE halves of `out`, and with new_pos every position"""
        ids = np.asarray(ids, np.int32)
        nd, dd = out["st_normal_depth"] == ST_DONE, out["st_descriptor"] == ST_DONE
        self.normal[ids[nd]] = out["normal"][nd]
        self.min_d[ids[nd]], self.max_d[ids[nd]] = out["min_distance"][nd], out["max_distance"][nd]
        self.pt_desc[ids[dd]] = out["desc"][dd]
        if with_pos:
            self.pos[ids] = out["pos"]

    # ---- crafting
    def observe(self, pt, slots, octave=None, descs=None, no_vote=False):
        """point pt into every keyframe of `slots`, with the given descriptors (else random ones)"""
        for n, k in enumerate(slots):
            i = self.s.put(int(k), pt, octave, no_vote)
            if descs is not None:
                self.desc[k, i] = descs[n]
        return pt


def base_scene(rng, crafted=cc.CRAFTED, **kw):
    r = RScene(cc.random_scene(rng, crafted=crafted, octave_255=kw.pop("octave_255", True), **kw), rng)
    return r


OBSERVER_COUNTS = (1, 2, 3, 4, 63, 64, 65, 257)
# family -> the branch counters that must be non-zero in it, for every seed 1..10
FAMILIES = {
    "random": ["bad_point", "no_observation", "n_odd", "n_even", "duplicate_entry", "no_ref"],
    "observers_1": ["n1", "single_observer"], "observers_2": ["n2"], "observers_3": ["n_odd"], "observers_4": ["n_even"],
    "observers_63": ["n_odd"], "observers_64": ["n_even"], "observers_65": ["n_odd"], "observers_257": ["n_odd"],
    "equal_medians": ["tie_at_best"],
    "identical_descriptors": ["tie_at_best", "n_even"],
    "complement": ["n2", "n_odd"],
    "bad_keyframe_among": ["bad_kf_skipped"],
    "all_observers_bad": ["all_kf_bad"],
    "bad_point": ["bad_point"],
    "no_vote_only": ["no_observation"],
    "twice_in_one_keyframe": ["duplicate_entry"],
    "ref_minus_1": ["no_ref"],
    "ref_not_observing": ["no_ref"],
    "ref_octave_edges": ["level_range"],
    "single_observer": ["single_observer", "n1"],
    "at_camera_centre": [],
}


def family_scene(family, seed):
    """the random scene of 40 keyframes by stride 64 with the family's points behind it, in crafted keyframes from slot T0 on"""
    rng = np.random.default_rng(7000 * (sorted(FAMILIES).index(family) + 1) + seed)
    nobs = int(family.split("_")[1]) if family.startswith("observers_") else 0
    r = base_scene(rng, crafted=max(cc.CRAFTED, nobs + 2))
    s, a = r.s, T0
    if family == "random":
        pass
    elif nobs:
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + nobs))
    elif family == "equal_medians":               # one-hot descriptors: every row is 0, 2, 2, 2, 2 and every median 2
        d = np.zeros((5, 32), np.uint8)
        d[np.arange(5), np.arange(5)] = 1 << np.arange(5)
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 5), descs=d)
    elif family == "identical_descriptors":
        d = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 6, axis=0)
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 6), descs=d)
    elif family == "complement":                  # distance 256: as the other element of a row of two, as the median of a row of three
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        r.named["p"] = r.observe(s.fresh()[0], [a, a + 1], descs=np.stack([d, ~d]))
        r.named["q"] = r.observe(s.fresh()[0], [a, a + 1, a + 2], descs=np.stack([d, ~d, ~d]))
    elif family == "bad_keyframe_among":
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 5))
        s.kf_flags[a + 2] |= KF_BAD
    elif family == "all_observers_bad":
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 3))
        s.kf_flags[a:a + 3] |= KF_BAD
    elif family == "bad_point":
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 4))
        s.pt_bad[r.named["p"]] = 1
    elif family == "no_vote_only":
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 3), no_vote=True)
    elif family == "twice_in_one_keyframe":
        r.named["p"] = r.observe(s.fresh()[0], [a, a + 1, a + 1, a + 2])
    elif family in ("ref_minus_1", "ref_not_observing", "single_observer", "at_camera_centre"):
        r.named["p"] = r.observe(s.fresh()[0], [a] if family == "single_observer" else range(a, a + 4))
        s.kf_flags[a + 5] |= KF_SET                                       # a set keyframe without the point
    elif family == "ref_octave_edges":
        r.named["p"] = r.observe(s.fresh()[0], range(a, a + 3), octave=NLEVELS - 1)
        r.named["q"] = r.observe(s.fresh()[0], range(a, a + 3), octave=NLEVELS)
    else:
        raise KeyError(family)
    r.default_refs()
    for pt in r.named.values():
        obs = r.observers(pt)
        r.ref_kf[pt] = obs[len(obs) // 2][0] if obs else a
    if family == "ref_minus_1":
        r.ref_kf[r.named["p"]] = -1
    if family == "ref_not_observing":
        r.ref_kf[r.named["p"]] = a + 5
    if family == "at_camera_centre":
        r.pos[r.named["p"]] = r.centres[a + 1]
    return r


def long_scene(nobs, seed=1):
    """a store of 1 100 keyframes by stride 8 with one point in `nobs` of them, and a few ordinary points"""
    rng = np.random.default_rng(90000 + nobs + seed)
    s = cc.Scene(1100, 8, 64, rng)
    r = RScene(s, rng)
    r.named["p"] = r.observe(s.fresh()[0], rng.permutation(1100)[:nobs], octave=3)
    for _ in range(20):
        r.observe(s.fresh()[0], rng.permutation(1100)[:int(rng.integers(1, 12))], octave=2)
    s.kf_flags[:] |= KF_SET
    r.default_refs()
    return r


# ---- the restatement
class RefStore(C.Structure):
    _fields_ = [("kfcap", C.c_int), ("stride", C.c_int), ("entries", C.c_void_p), ("kfFlags", C.c_void_p), ("octaves", C.c_void_p), ("desc", C.c_void_p),
                ("centres", C.c_void_p), ("poolCap", C.c_int), ("pos", C.c_void_p), ("normal", C.c_void_p), ("minD", C.c_void_p), ("maxD", C.c_void_p),
                ("ptDesc", C.c_void_p), ("ptFlags", C.c_void_p)]


def _declare(L):
    L.rfr_open.restype = C.c_void_p
    L.rfr_open.argtypes = [C.c_void_p]
    L.rfr_close.argtypes = [C.c_void_p]
    L.rfr_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.rfr_refresh.restype = None


def shim():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("refresh_ref", _declare)


class Ref:
    """the restatement over a scene as it is NOW (copies are taken, the observation index is built here)"""

    def __init__(self, r, count_branches=True):
        s = r.s
        self._keep = [np.ascontiguousarray(a).copy() for a in (s.entries, s.kf_flags, s.octaves, r.desc, r.centres, r.pos, r.normal, r.min_d, r.max_d,
                                                                r.pt_desc, r.pt_flags())]
        k = [p(a) for a in self._keep]
        self._st = RefStore(s.kfcap, s.stride, k[0], k[1], k[2], k[3], k[4], s.pool_cap, k[5], k[6], k[7], k[8], k[9], k[10])
        self._h = shim().rfr_open(C.byref(self._st))
        self.branches = np.zeros(len(BRANCHES), np.int32) if count_branches else None

    def __del__(self):
        if getattr(self, "_h", None):
            shim().rfr_close(self._h)
            self._h = None

    def refresh(self, ids, ref_kf, what=BOTH, new_pos=None, sf=SF):
        ids, ref = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(ref_kf, np.int32)
        pos = None if new_pos is None else np.ascontiguousarray(new_pos, np.float32)
        sf = np.ascontiguousarray(sf, np.float32)
        out = np.zeros(len(ids), POINT_DTYPE)
        shim().rfr_refresh(self._h, p(ids), p(ref), p(pos), len(ids), int(what), p(sf), len(sf), p(out), p(self.branches))
        return out

    def seen(self):
        return dict(zip(BRANCHES, [int(x) for x in self.branches]))


def same_records(a, b):
    """every field of every record: integers and bytes equal, floats equal as bits -- or both NaN, whose sign and payload IEEE 754
    leaves to the implementation (a point exactly at a camera centre: 0 * inf)"""
    if a.shape != b.shape:
        return False
    for n in POINT_DTYPE.names:
        x, y = a[n], b[n]
        if n in FLOAT_FIELDS:
            ok = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
            if not ok.all():
                return False
        elif not np.array_equal(x, y):
            return False
    return True
