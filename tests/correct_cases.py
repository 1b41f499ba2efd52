"""Scenes for the correction of LoopClosing::CorrectLoop / MultiMapper::UpdatePosesAndAdd over a keyframe store (orbe_*,
DESIGN.md §8x), shared by test_correct_cpu.py and test_gpu_correct.py: refresh_cases' seeded random store (24 keyframes by stride
96, a pool of 1 024) with poses, a loop Sim3, a list of keyframes and a few crafted points behind it, each family named after the
branch of LoopClosing.cc:440-524 it forces, and the restatement (tools/correct_ref.hpp) behind tests/ref_shim.py."""
import ctypes as C

import numpy as np

import covis_cases as cc
import refresh_cases as rc
from ref_shim import cached_shim, p, rot_axis_angle

NO_VOTE, KF_BAD, KF_SET = cc.NO_VOTE, cc.KF_BAD, cc.KF_SET
ST_DONE, ST_NO_OBSERVATION, ST_NO_REF, ST_LEVEL_RANGE = rc.ST_DONE, rc.ST_NO_OBSERVATION, rc.ST_NO_REF, rc.ST_LEVEL_RANGE
NLEVELS, SF = rc.NLEVELS, rc.SF
BRANCHES = ["anchor_kf", "other_kf", "anchor_first", "anchor_last", "anchor_middle", "single_kf", "scale_one", "scale_other",
            "null_entry", "empty_row", "bad_point", "skipped_point", "again_in_owners_row", "again_in_later_kf", "moved", "moved_through_no_vote",
            "obs_reposed", "obs_pending", "obs_owner", "obs_unlisted", "ref_reposed", "ref_pending", "ref_owner", "ref_unlisted", "ref_none",
            "no_observation", "no_ref", "level_range", "done"]
KF_DTYPE = np.dtype([("corrected", "<f8", 8), ("non_corrected", "<f8", 8), ("Tiw", "<f4", 12), ("Ow", "<f4", 3), ("n_points", "<i4")])
POINT_DTYPE = np.dtype([("id", "<i4"), ("owner_slot", "<i4"), ("owner_idx", "<i4"), ("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"),
                        ("max_distance", "<f4"), ("n_obs", "<i4"), ("status", "u1"), ("pad", "u1", 3)])
NKF, KFCAP, STRIDE, T0 = 16, 24, 96, 16          # the random keyframes, the store, the first crafted slot


class CScene:
    """a refresh_cases.RScene (store, pool, mpRefKF) with what the correction takes beside it: GetPose() per slot, the listed
    keyframes in the caller's order, the anchor's position among them, Scw, the skipped ids"""

    def __init__(self, r, rng):
        self.r, self.s, self.rng = r, r.s, rng
        self.poses = np.zeros((r.kfcap, 12), np.float32)
        for k in range(r.kfcap):
            R = rot_axis_angle(rng.normal(size=3), rng.uniform(-np.pi, np.pi)).astype(np.float32)
            self.poses[k] = np.concatenate([R, rng.uniform(-3, 3, (3, 1)).astype(np.float32)], axis=1).reshape(12)
        self.slots = np.zeros(0, np.int32)
        self.anchor = 0
        self.skip = np.zeros(0, np.int32)
        self.Scw = np.zeros(8)
        self.set_scw(rng.uniform(0.6, 1.6))

    kfcap = property(lambda self: self.r.kfcap)
    stride = property(lambda self: self.r.stride)
    pool_cap = property(lambda self: self.r.pool_cap)
    named = property(lambda self: self.r.named)
    Tiw = property(lambda self: np.ascontiguousarray(self.poses[self.slots]))

    def set_scw(self, scale):
        q = self.rng.normal(size=4)
        self.Scw = np.concatenate([q / np.linalg.norm(q), self.rng.uniform(-2, 2, 3), [scale]]).astype(np.float64)

    def list_keyframes(self, slots, anchor_slot):
        """the listed keyframes, shuffled; the anchor by its slot"""
        slots = self.rng.permutation(np.asarray(slots, np.int32))
        self.slots, self.anchor = slots.astype(np.int32), int(np.flatnonzero(slots == anchor_slot)[0])

    def holders(self, pt):
        """the (slot, index) entries of the LISTED keyframes that hold pt, NO_VOTE ones included, in visiting order"""
        e = self.s.entries
        return [(int(k), int(i)) for k in np.sort(self.slots) for i in np.flatnonzero((e[k] >= 0) & ((e[k] & ~NO_VOTE) == pt))]

    def apply(self, kf, pts):
        """what a commit leaves: positions, the DONE points' normals and bounds, the listed keyframes' centres"""
        r = self.r
        ids = pts["id"]
        r.pos[ids] = pts["pos"]
        d = pts["status"] == ST_DONE
        r.normal[ids[d]], r.min_d[ids[d]], r.max_d[ids[d]] = pts["normal"][d], pts["min_distance"][d], pts["max_distance"][d]
        r.centres[self.slots] = kf["Ow"]


def base_scene(rng, nkf=NKF, kfcap=KFCAP, stride=STRIDE, npts=600, pool_extra=424, **kw):
    r = rc.RScene(cc.random_scene(rng, nkf=nkf, stride=stride, npts=npts, kfcap=kfcap, pool_extra=pool_extra, crafted=kfcap - nkf, **kw), rng)
    return CScene(r, rng)


# family -> the branch counters that must be non-zero in it, for every seed 1..10; what else a family must show is asserted by name
# in test_correct_cpu.py.  A listed keyframe that observes a point holds it, so no observer and no OBSERVING reference keyframe
# of a rank below the owner's exists in a store (rules 1 and 3 of the header): obs_reposed stays zero in every scene, the family
# for the other ranks has its lower-ranked holder hold the point through a NO_VOTE slot (it owns, and does not observe), and the
# reference keyframe of lower rank is one that does not observe.
FAMILIES = {
    "random": ["moved", "null_entry", "bad_point", "again_in_later_kf", "moved_through_no_vote", "obs_owner", "obs_pending", "obs_unlisted", "done"],
    "one_holder": ["moved", "obs_owner", "ref_owner"],
    "several_holders_shuffled": ["again_in_later_kf", "obs_pending"],
    "twice_in_owners_row": ["again_in_owners_row"],
    "no_vote_only": ["moved_through_no_vote", "no_observation"],
    "bad_point": ["bad_point"],
    "skipped_point": ["skipped_point"],
    "observers_outside_list": ["obs_unlisted"],
    "observers_of_other_ranks": ["obs_pending", "moved_through_no_vote"],
    "ref_lower_rank": ["ref_reposed", "no_ref"],
    "ref_higher_rank": ["ref_pending"],
    "ref_outside_list": ["ref_unlisted"],
    "ref_minus_1": ["ref_none", "no_ref"],
    "ref_not_observing": ["no_ref"],
    "octave_out_of_range": ["level_range"],
    "anchor_first": ["anchor_first"],
    "anchor_middle": ["anchor_middle"],
    "anchor_last": ["anchor_last"],
    "k_1": ["single_kf", "anchor_first", "anchor_last"],
    "scale_one": ["scale_one"],
    "scale_other": ["scale_other"],
    "empty_keyframe": ["empty_row"],
}


def family_scene(family, seed):
    """the random scene with the family's points behind it in crafted keyframes from slot T0 on: T0 .. T0 + 5 listed, T0 + 6 set
    and not listed, T0 + 7 listed and empty in its own family; eight of the random keyframes listed beside them"""
    rng = np.random.default_rng(9000 * (sorted(FAMILIES).index(family) + 1) + seed)
    c = base_scene(rng)
    r, s, a = c.r, c.s, T0
    s.kf_flags[a:a + 7] |= KF_SET
    new = lambda: s.fresh()[0]
    ref = {}
    if family == "one_holder":
        r.named["p"] = r.observe(new(), [a + 1])
    elif family == "several_holders_shuffled":
        r.named["p"] = r.observe(new(), [a + 5, a + 1, a + 3])
    elif family == "twice_in_owners_row":
        r.named["p"] = r.observe(new(), [a + 1, a + 1, a + 2])
    elif family == "no_vote_only":
        r.named["p"] = r.observe(new(), [a + 2], no_vote=True)
    elif family == "bad_point":
        r.named["p"] = r.observe(new(), [a + 1, a + 2])
        s.pt_bad[r.named["p"]] = 1
    elif family == "skipped_point":
        r.named["p"] = r.observe(new(), [a + 1, a + 2])
        c.skip = np.array([r.named["p"]], np.int32)
    elif family == "observers_outside_list":
        r.named["p"] = r.observe(new(), [a + 1, a + 6])
    elif family == "observers_of_other_ranks":
        pt = new()
        r.observe(pt, [a + 1], no_vote=True)                              # the lower-ranked holder: it owns, it does not observe
        r.named["p"] = r.observe(pt, [a + 3, a + 5, a + 6])
        ref["p"] = a + 3
    elif family in ("ref_lower_rank", "ref_higher_rank", "ref_outside_list", "ref_minus_1", "ref_not_observing"):
        r.named["p"] = r.observe(new(), [a + 2, a + 4, a + 6])
        ref["p"] = {"ref_lower_rank": a, "ref_higher_rank": a + 4, "ref_outside_list": a + 6, "ref_minus_1": -1, "ref_not_observing": a + 5}[family]
    elif family == "octave_out_of_range":
        r.named["p"] = r.observe(new(), [a + 1, a + 2], octave=NLEVELS)
        r.named["q"] = r.observe(new(), [a + 1, a + 2], octave=NLEVELS - 1)
    elif family == "empty_keyframe":
        s.kf_flags[a + 7] |= KF_SET
    elif family not in ("random", "anchor_first", "anchor_middle", "anchor_last", "k_1", "scale_one", "scale_other"):
        raise KeyError(family)
    r.default_refs()
    for name, pt in r.named.items():
        obs = r.observers(pt)
        r.ref_kf[pt] = ref.get(name, obs[0][0] if obs else -1)
    some = rng.permutation(s.set_slots()[s.set_slots() < NKF])[:8]
    listed = sorted(list(some) + list(range(a, a + 6)) + ([a + 7] if family == "empty_keyframe" else []))
    anchor = {"anchor_first": listed[0], "anchor_last": listed[-1], "anchor_middle": listed[len(listed) // 2]}.get(family, listed[int(rng.integers(len(listed)))])
    if family == "k_1":
        listed, anchor = [a + 1], a + 1
        r.named["p"] = r.observe(new(), [a + 1, a + 2])
        r.ref_kf[r.named["p"]] = a + 2
    if family == "scale_one":
        c.set_scw(1.0)
    c.list_keyframes(listed, anchor)
    return c


def long_scene(nobs, seed=1, nkf=1030, stride=4):
    """a store of 1 030 keyframes by stride 4 with one point in `nobs` of them and a few ordinary points; every keyframe listed"""
    rng = np.random.default_rng(91000 + nobs + seed)
    s = cc.Scene(nkf, stride, 64, rng)
    r = rc.RScene(s, rng)
    r.named["p"] = r.observe(s.fresh()[0], rng.permutation(nkf)[:nobs], octave=3)
    for _ in range(20):
        r.observe(s.fresh()[0], rng.permutation(nkf)[:int(rng.integers(1, 3))], octave=2)
    s.kf_flags[:] |= KF_SET
    r.default_refs()
    c = CScene(r, rng)
    c.list_keyframes(np.arange(nkf), int(rng.integers(nkf)))
    return c


def observer_scene(seed=1, nkf=48, stride=32):
    """points of 17 .. 40 observers (the refresh's long path) among points of a few, every keyframe listed"""
    rng = np.random.default_rng(92000 + seed)
    s = cc.Scene(nkf, stride, 128, rng)
    r = rc.RScene(s, rng)
    for n in (16, 17, 18, 31, 32, 33, 40):
        r.named["n%d" % n] = r.observe(s.fresh()[0], rng.permutation(nkf)[:n], octave=int(rng.integers(0, 8)))
    for _ in range(60):
        r.observe(s.fresh()[0], rng.permutation(nkf)[:int(rng.integers(1, 9))])
    s.kf_flags[:] |= KF_SET
    r.default_refs()
    c = CScene(r, rng)
    c.list_keyframes(np.arange(nkf), int(rng.integers(nkf)))
    return c


def dense_scene(seed=1, nkf=130, stride=256, npts=6000):
    """a 130 x 256 store over a pool of 8 192 for the K = 1, 63, 64, 65 and all-keyframes calls"""
    rng = np.random.default_rng(93000 + seed)
    c = base_scene(rng, nkf=nkf, kfcap=nkf, stride=stride, npts=npts, pool_extra=8192 - npts, p_unset=0.0, octave_255=False)
    c.r.default_refs()
    return c


# ---- the restatement
class RefWorld(C.Structure):
    _fields_ = [("kfcap", C.c_int), ("stride", C.c_int), ("entries", C.c_void_p), ("kfFlags", C.c_void_p), ("octaves", C.c_void_p), ("centres", C.c_void_p),
                ("poolCap", C.c_int), ("pos", C.c_void_p), ("normal", C.c_void_p), ("minD", C.c_void_p), ("maxD", C.c_void_p), ("ptFlags", C.c_void_p),
                ("refKf", C.c_void_p)]


class RefArgs(C.Structure):
    _fields_ = [("K", C.c_int), ("slots", C.c_void_p), ("Tiw", C.c_void_p), ("anchor", C.c_int), ("Scw", C.c_void_p), ("skip", C.c_void_p), ("nSkip", C.c_int),
                ("sf", C.c_void_p), ("nlevels", C.c_int)]


def _declare(L):
    L.cor_correct.argtypes = [C.c_void_p] * 5
    L.cor_index.restype = C.c_void_p
    L.cor_index.argtypes = [C.c_void_p]
    L.cor_index_free.argtypes = [C.c_void_p]
    L.cor_correct_indexed.argtypes = [C.c_void_p] * 5
    assert L.cor_kf_size() == KF_DTYPE.itemsize and L.cor_point_size() == POINT_DTYPE.itemsize


def shim():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("correct_ref", _declare)


class After:
    """what the restatement's loop left in its copies of the arrays"""

    def __init__(self, k):
        self.centres, self.pos, self.normal, self.min_d, self.max_d = k[3].reshape(-1, 3), k[4].reshape(-1, 3), k[5].reshape(-1, 3), k[6], k[7]


def ref_correct(c, slots=None, anchor=None, branches=None, sf=SF):
    """the restatement over the scene as it is NOW, on copies -> (kf records in the caller's order, the moved points in visiting
    order, After).  branches: an int32 array of len(BRANCHES) added to, or None"""
    r, s = c.r, c.s
    slots = np.ascontiguousarray(c.slots if slots is None else slots, np.int32)
    anchor = c.anchor if anchor is None else anchor
    k = [np.ascontiguousarray(a).copy() for a in (s.entries, s.kf_flags, s.octaves, r.centres, r.pos, r.normal, r.min_d, r.max_d, r.pt_flags(), r.ref_kf)]
    w = RefWorld(s.kfcap, s.stride, p(k[0]), p(k[1]), p(k[2]), p(k[3]), s.pool_cap, p(k[4]), p(k[5]), p(k[6]), p(k[7]), p(k[8]), p(k[9]))
    Tiw, Scw, skip, sf = np.ascontiguousarray(c.poses[slots]), np.ascontiguousarray(c.Scw), np.ascontiguousarray(c.skip, np.int32), np.ascontiguousarray(sf, np.float32)
    a = RefArgs(len(slots), p(slots), p(Tiw), int(anchor), p(Scw), p(skip), len(skip), p(sf), len(sf))
    kf, pts = np.zeros(len(slots), KF_DTYPE), np.zeros(s.pool_cap, POINT_DTYPE)
    n = shim().cor_correct(C.byref(w), C.byref(a), p(kf), p(pts), p(branches))
    return kf, pts[:n].copy(), After(k)


def seen(branches):
    return dict(zip(BRANCHES, [int(x) for x in branches]))
