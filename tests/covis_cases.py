"""Scenes for KeyFrame::UpdateConnections and KeyFrameCulling's counts over a keyframe store (orbn_*), shared by
test_covis_cpu.py and test_gpu_covis.py: seeded random covisibility with a few crafted keyframes behind it, each family named
after the branch of KeyFrame.cc:300-400 / LocalMapping.cc:632-698 it forces, and the restatement (tools/covis_ref.hpp) behind
tests/ref_shim.py."""
import ctypes as C

import numpy as np

from ref_shim import cached_shim, p

NO_VOTE = 1 << 30
KF_BAD, KF_SET = 1, 2
TH, TH_OBS = 15, 3
BRANCHES = ["empty_counter", "fallback_to_max", "tie_at_max", "ordered_ties", "self_skipped", "bad_point_skipped", "no_vote_target_slot", "duplicate_entry",
            "obs_at_th", "obs_at_th_plus_1", "octave_plus_1", "octave_plus_2", "qualifying_below", "qualifying_at", "redundant_yes", "redundant_no"]
CRAFTED = 8          # slots behind the random keyframes that the families fill


class Scene:
    """a store's entries and octaves (dense, by slot), the set bytes, the pool's bad bytes"""

    def __init__(self, kfcap, stride, pool_cap, rng):
        self.kfcap, self.stride, self.pool_cap, self.rng = kfcap, stride, pool_cap, rng
        self.entries = np.full((kfcap, stride), -1, np.int32)
        self.octaves = np.zeros((kfcap, stride), np.uint8)
        self.kf_flags = np.zeros(kfcap, np.uint8)
        self.pt_bad = np.zeros(pool_cap, np.uint8)
        self.next_pt = 0

    def set_slots(self):
        return np.flatnonzero(self.kf_flags & KF_SET).astype(np.int32)

    def fresh(self, n=1):
        """n pool ids nothing holds yet"""
        assert self.next_pt + n <= self.pool_cap, "the scene's pool is too small"
        ids = np.arange(self.next_pt, self.next_pt + n, dtype=np.int32)
        self.next_pt += n
        return ids

    def put(self, k, pt, octave=None, no_vote=False):
        """point pt into a free match slot of keyframe k (chosen at random)"""
        free = np.flatnonzero(self.entries[k] == -1)
        assert len(free), "keyframe %d is full" % k
        i = int(free[self.rng.integers(len(free))])
        self.kf_flags[k] |= KF_SET
        self.entries[k, i] = int(pt) | (NO_VOTE if no_vote else 0)
        self.octaves[k, i] = self.rng.integers(0, 8) if octave is None else octave
        return i

    def share(self, k, others, n, octave=None):
        """n fresh points, each in keyframe k and in every keyframe of `others`"""
        ids = self.fresh(n)
        for pt in ids:
            self.put(k, pt, octave)
            for j in others:
                self.put(j, pt, octave)
        return ids

    def records(self, slots=None):
        """the arguments of KeyFrameStore.set for `slots` (default: every set slot); a row's entries up to its last used slot"""
        slots = self.set_slots() if slots is None else np.asarray(slots, np.int32)
        ent = []
        for k in slots:
            used = np.flatnonzero(self.entries[k] != -1)
            ent.append(self.entries[k, :used[-1] + 1 if len(used) else 0])
        none = [np.zeros(0, np.int32)] * len(slots)
        return slots, self.kf_flags[slots] & KF_BAD, ent, none, np.full(len(slots), -1, np.int32), none


def random_scene(rng, nkf=40, stride=64, npts=600, kfcap=None, pool_extra=400, fill=0.7, p_unset=0.1, p_pt_bad=0.05, p_no_vote=0.1, spread=1.5,
                 crafted=CRAFTED, octave_255=True):
    """keyframe k of the first nkf slots sees a window of the point range around k, so neighbours share about th points and
    far keyframes none; some slots stay unset, one row is empty and one full; `crafted` empty slots follow"""
    kfcap = nkf + crafted if kfcap is None else kfcap
    s = Scene(kfcap, stride, npts + pool_extra, rng)
    s.next_pt = npts
    s.pt_bad[:npts] = rng.random(npts) < p_pt_bad
    w = max(int(spread * npts / max(nkf, 1)), stride)
    special = rng.permutation(nkf)[:2] if nkf >= 4 else []
    for k in range(nkf):
        if nkf > 2 and k not in special and rng.random() < p_unset:
            continue
        s.kf_flags[k] = KF_SET | (KF_BAD if rng.random() < 0.1 else 0)
        n_k = int(rng.integers(0, stride + 1)) if rng.random() < 0.2 else int(fill * stride)
        if len(special) and k == special[0]:
            n_k = 0
        if len(special) and k == special[1]:
            n_k = stride
        c = int((k + 0.5) * npts / nkf)
        lo = min(max(c - w, 0), max(npts - 2 * w, 0))
        cand = np.arange(lo, min(lo + 2 * w, npts))
        pts = rng.permutation(cand)[:min(n_k, len(cand))].astype(np.int32)
        if len(pts) < n_k and len(pts):                         # (a full row of a wide stride: points repeat)
            pts = np.concatenate([pts, pts[rng.integers(0, len(pts), n_k - len(pts))]])
        pos = np.sort(rng.permutation(stride)[:len(pts)])
        s.entries[k, pos] = np.where(rng.random(len(pts)) < p_no_vote, pts | NO_VOTE, pts)
        s.octaves[k, pos] = rng.integers(0, 8, len(pts))
        holes = np.flatnonzero(s.entries[k] == -1)
        if len(holes) and len(pts) and rng.random() < 0.5:       # a point twice in one keyframe
            h = holes[rng.integers(len(holes))]
            s.entries[k, h] = pts[rng.integers(len(pts))]
            s.octaves[k, h] = rng.integers(0, 8)
    used = np.argwhere(s.entries >= 0)
    if octave_255 and len(used):
        k, i = used[rng.integers(len(used))]
        s.octaves[k, i] = 255
    return s


# family -> the branch counters that must be non-zero in it over seeds 1..10; what else a family must show is asserted by
# name in test_covis_cpu.py
FAMILIES = {
    "random": ["self_skipped", "bad_point_skipped", "no_vote_target_slot", "duplicate_entry", "redundant_no"],
    "weights_14_and_15": [],
    "two_at_the_maximum": ["tie_at_max", "ordered_ties"],
    "three_at_one_weight": ["ordered_ties"],
    "none_at_th": ["fallback_to_max", "tie_at_max"],
    "no_observed_point": ["empty_counter"],
    "duplicates_no_vote_bad": ["duplicate_entry", "no_vote_target_slot", "bad_point_skipped", "self_skipped"],
    "observations_at_th": ["obs_at_th", "obs_at_th_plus_1"],
    "octave_edges": ["octave_plus_1", "octave_plus_2"],
    "qualifying_edges": ["qualifying_below", "qualifying_at"],
    "ratio_edges": ["redundant_yes", "redundant_no"],
    "own_slots_no_vote": ["no_vote_target_slot", "redundant_yes"],
}
T0 = 40              # the first crafted slot of a family scene: the keyframe the family is about


def family_scene(family, seed):
    """the random scene of 40 keyframes by stride 64 with the family's keyframes in slots T0 .. T0 + 7, on points of their own"""
    rng = np.random.default_rng(1000 * (sorted(FAMILIES).index(family) + 1) + seed)
    s = random_scene(rng)
    a = T0
    if family == "random":
        pass
    elif family == "weights_14_and_15":           # one below th, th, one above
        s.share(a, [a + 1], 14)
        s.share(a, [a + 2], 15)
        s.share(a, [a + 3], 16)
    elif family == "two_at_the_maximum":
        s.share(a, [a + 2], 20)
        s.share(a, [a + 1], 20)
        s.share(a, [a + 3], 17)
    elif family == "three_at_one_weight":
        for j in (3, 1, 2):
            s.share(a, [a + j], 16)
        s.share(a, [a + 4], 15)
    elif family == "none_at_th":                  # the largest weight is below th, and two keyframes have it
        s.share(a, [a + 1], 5)
        s.share(a, [a + 3], 9)
        s.share(a, [a + 2], 9)
    elif family == "no_observed_point":           # points nobody else sees; a keyframe without entries; one whose slots are NO_VOTE only
        for pt in s.fresh(10):
            s.put(a, pt)
        s.kf_flags[a + 1] |= KF_SET
        for pt in s.fresh(6):
            s.put(a + 2, pt, no_vote=True)
    elif family == "duplicates_no_vote_bad":
        (d,) = s.fresh()                          # twice in the target, once in a + 1, twice in a + 2: weights 2 and 4
        for k in (a, a, a + 1, a + 2, a + 2):
            s.put(k, d)
        (q,) = s.fresh()                          # in the target's match slot without the observation: still a point of it
        s.put(a, q, no_vote=True)
        s.put(a + 1, q)
        (r,) = s.fresh()                          # a bad point the target shares
        s.pt_bad[r] = 1
        s.put(a, r)
        s.put(a + 1, r)
        s.share(a, [a + 3], 16)
    elif family == "observations_at_th":          # Observations() == th_obs: not looked at; th_obs + 1: looked at, and redundant
        s.share(a, [a + 1, a + 2], 3, octave=2)
        s.share(a, [a + 1, a + 2, a + 3], 3, octave=2)
    elif family == "octave_edges":                # the target at octave 2; others at 3 (counts), 4 (does not), 3, 3
        for pt in s.fresh(4):
            s.put(a, pt, 2)
            for j, o in ((1, 3), (2, 4), (3, 3), (4, 3)):
                s.put(a + j, pt, o)
    elif family == "qualifying_edges":
        for pt in s.fresh(3):                     # th_obs - 1 qualifying others, two that do not qualify
            s.put(a, pt, 1)
            for j, o in ((1, 0), (2, 2), (3, 3), (4, 7)):
                s.put(a + j, pt, o)
        for pt in s.fresh(3):                     # exactly th_obs qualifying others
            s.put(a, pt, 1)
            for j, o in ((1, 0), (2, 2), (3, 1), (4, 7)):
                s.put(a + j, pt, o)
    elif family == "ratio_edges":                 # 9 of 10 redundant: 9 > 9.0 is false; 10 of 10 and 19 of 20: true
        s.share(a, [a + 3, a + 4, a + 5], 9, octave=1)
        s.share(a, [], 1, octave=1)
        s.share(a + 1, [a + 3, a + 4, a + 5], 10, octave=1)
        s.share(a + 2, [a + 3, a + 4, a + 5], 19, octave=1)
        s.share(a + 2, [], 1, octave=1)
    elif family == "own_slots_no_vote":           # every slot of the target is NO_VOTE: nothing of its own to leave out
        for pt in s.fresh(12):
            s.put(a, pt, 3, no_vote=True)
            for j in (1, 2, 3, 4):
                s.put(a + j, pt, 3)
    else:
        raise KeyError(family)
    return s


# ---- the restatement
class RefStore(C.Structure):
    _fields_ = [("kfcap", C.c_int), ("stride", C.c_int), ("entries", C.c_void_p), ("kfFlags", C.c_void_p), ("octaves", C.c_void_p), ("ptBad", C.c_void_p),
                ("poolCap", C.c_int)]


def _declare(L):
    L.cov_open.restype = C.c_void_p
    L.cov_open.argtypes = [C.c_void_p]
    L.cov_close.argtypes = [C.c_void_p]
    L.cov_connections.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_void_p]
    L.cov_culling.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.cov_culling.restype = None


def shim():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("covis_ref", _declare)


class Ref:
    """the restatement over a scene as it is NOW (the observation index is built here): connections(targets), culling(targets)"""

    def __init__(self, s, count_branches=True):
        self._keep = [np.ascontiguousarray(a) for a in (s.entries, s.kf_flags, s.octaves, s.pt_bad)]
        self._st = RefStore(s.kfcap, s.stride, *[p(a) for a in self._keep], s.pool_cap)
        self._h = shim().cov_open(C.byref(self._st))
        self.kfcap = s.kfcap
        self.branches = np.zeros(len(BRANCHES), np.int32) if count_branches else None   # (None: the walk alone, for tools/covis_bench.py)

    def __del__(self):
        if getattr(self, "_h", None):
            shim().cov_close(self._h)
            self._h = None

    def connections(self, targets, th=TH):
        tg = np.ascontiguousarray(targets, np.int32)
        K, cap = len(tg), max(len(tg) * self.kfcap, 1)
        o = {"status": np.zeros(K, np.int32), "kf_max": np.zeros(K, np.int32), "n_max": np.zeros(K, np.int32), "cnt_start": np.zeros(K + 1, np.int32),
             "cnt_kf": np.zeros(cap, np.int32), "cnt_w": np.zeros(cap, np.int32), "ord_start": np.zeros(K + 1, np.int32),
             "ord_kf": np.zeros(cap, np.int32), "ord_w": np.zeros(cap, np.int32)}
        rc = shim().cov_connections(self._h, p(tg), K, th, *[p(o[n]) for n in ("status", "kf_max", "n_max", "cnt_start", "cnt_kf", "cnt_w", "ord_start",
                                                                                  "ord_kf", "ord_w")], cap, p(self.branches))
        assert rc == 0
        for n in ("cnt_kf", "cnt_w"):
            o[n] = o[n][:o["cnt_start"][-1]].copy()
        for n in ("ord_kf", "ord_w"):
            o[n] = o[n][:o["ord_start"][-1]].copy()
        return o

    def culling(self, targets, th_obs=TH_OBS):
        tg = np.ascontiguousarray(targets, np.int32)
        K = len(tg)
        o = {"n_mps": np.zeros(K, np.int32), "n_redundant": np.zeros(K, np.int32), "redundant": np.zeros(K, np.uint8)}
        shim().cov_culling(self._h, p(tg), K, th_obs, p(o["n_mps"]), p(o["n_redundant"]), p(o["redundant"]), p(self.branches))
        return o

    def seen(self):
        return dict(zip(BRANCHES, [int(x) for x in self.branches]))


def row(o, t, which="cnt"):
    a, b = o[which + "_start"][t], o[which + "_start"][t + 1]
    return o[which + "_kf"][a:b], o[which + "_w"][a:b]
