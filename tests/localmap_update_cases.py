"""Scenes for Tracking::UpdateLocalMap over a keyframe store (orbu_*), shared by test_localmap_update_cpu.py and
test_gpu_localmap_update.py: seeded random covisibility graphs, each family named after the branch of Tracking.cc:1289-1397 /
:1263-1286 it forces, and the restatement (tools/localmap_update_ref.hpp) behind tests/ref_shim.py."""
import ctypes as C

import numpy as np

from ref_shim import cached_shim, p

NO_VOTE = 1 << 30
KF_BAD, KF_SET = 1, 2
BRANCHES = ["neighbour_taken", "neighbour_skipped_bad", "neighbour_skipped_included", "neighbours_exhausted", "child_taken", "child_skipped_bad",
            "parent_taken", "parent_bad_taken", "size_break", "steps_run"]


class Scene:
    """a store's arrays (dense, by slot), the pool's bad bytes, one frame"""

    def __init__(self, kfcap, stride, maxc, pool_cap, max_keyframes=80):
        self.kfcap, self.stride, self.maxc, self.pool_cap, self.max_keyframes = kfcap, stride, maxc, pool_cap, max_keyframes
        self.entries = np.full((kfcap, stride), -1, np.int32)
        self.kf_flags = np.zeros(kfcap, np.uint8)
        self.neigh = np.full((kfcap, 10), -1, np.int32)
        self.parent = np.full(kfcap, -1, np.int32)
        self.nchildren = np.zeros(kfcap, np.int32)
        self.children = np.full((kfcap, max(maxc, 1)), -1, np.int32)
        self.pt_bad = np.zeros(pool_cap, np.uint8)
        self.frame_ids = np.zeros(0, np.int32)

    def set_slots(self):
        return np.flatnonzero(self.kf_flags & KF_SET).astype(np.int32)

    def set_children(self, k, ch):
        ch = list(ch)
        assert len(ch) <= self.maxc
        self.nchildren[k] = len(ch)
        self.children[k, :] = -1
        self.children[k, :len(ch)] = ch

    def records(self, slots=None):
        """the arguments of KeyFrameStore.set for `slots` (default: every set slot); a row's entries up to its last used slot"""
        slots = self.set_slots() if slots is None else np.asarray(slots, np.int32)
        ent = []
        for k in slots:
            used = np.flatnonzero(self.entries[k] != -1)
            ent.append(self.entries[k, :used[-1] + 1 if len(used) else 0])
        return (slots, self.kf_flags[slots] & KF_BAD, ent, [self.neigh[k] for k in slots], self.parent[slots],
                [self.children[k, :self.nchildren[k]] for k in slots])

    def votes(self):
        """numpy, for building scenes only: votes per slot"""
        cnt = np.zeros(self.pool_cap, np.int64)
        ids = self.frame_ids[self.frame_ids >= 0]
        np.add.at(cnt, ids[self.pt_bad[ids] == 0], 1)
        e = self.entries
        ok = (e >= 0) & ((e & NO_VOTE) == 0)
        v = np.where(ok, cnt[np.where(ok, e, 0)], 0).sum(axis=1)
        return np.where(self.kf_flags & KF_SET, v, 0)

    def group(self):
        v = self.votes()
        return np.flatnonzero((v > 0) & ((self.kf_flags & KF_BAD) == 0))

    def free(self, bad=False):
        """set keyframes without a vote that are (not) bad"""
        v = self.votes()
        return np.flatnonzero((v == 0) & ((self.kf_flags & KF_SET) != 0) & (((self.kf_flags & KF_BAD) != 0) == bad))


def base_scene(rng, nkf=40, kfcap=None, stride=64, maxc=4, npts=600, nframe=120, fill=0.7, p_unset=0.1, p_kf_bad=0.1, p_pt_bad=0.05,
               p_no_vote=0.1, max_keyframes=80, spread=3.0):
    """keyframe k sees a window of the point range around k; the frame sees a window around a random centre: a band of keyframes
    is voted, the rest is there for the expansion.  The last 16 pool ids are in no keyframe."""
    kfcap = nkf if kfcap is None else kfcap
    s = Scene(kfcap, stride, maxc, npts + 16, max_keyframes)
    s.pt_bad[:npts] = rng.random(npts) < p_pt_bad
    slots = np.sort(rng.permutation(kfcap)[:nkf])
    w = max(int(spread * npts / max(nkf, 1)), stride)
    for j, k in enumerate(slots):
        if rng.random() < p_unset:
            continue
        s.kf_flags[k] = KF_SET | (KF_BAD if rng.random() < p_kf_bad else 0)
        n_k = int(rng.integers(0, stride + 1)) if rng.random() < 0.2 else int(fill * stride)
        c = int((j + 0.5) * npts / nkf)
        lo = min(max(c - w, 0), max(npts - 2 * w, 0))
        cand = np.arange(lo, min(lo + 2 * w, npts))
        pts = rng.permutation(cand)[:min(n_k, len(cand))].astype(np.int32)
        pos = np.sort(rng.permutation(stride)[:len(pts)])
        pts = np.where(rng.random(len(pts)) < p_no_vote, pts | NO_VOTE, pts)
        s.entries[k, pos] = pts
        holes = np.flatnonzero(s.entries[k] == -1)
        if len(holes) and len(pts) and rng.random() < 0.5:   # a point twice in one keyframe
            s.entries[k, holes[rng.integers(len(holes))]] = pts[rng.integers(len(pts))]
    live = s.set_slots()
    for k in live:
        others = live[live != k]
        if len(others):
            near = others[np.argsort(np.abs(others - k) + rng.random(len(others)) * 6)]
            s.neigh[k, :min(10, len(near))] = near[:10]
            if rng.random() < 0.3:
                s.neigh[k, rng.integers(10)] = -1
            s.set_children(k, rng.permutation(others)[:rng.integers(0, maxc + 1)] if maxc else [])
    centre = int(rng.integers(0, npts))
    lo = min(max(centre - w, 0), max(npts - 2 * w, 0))
    ids = rng.integers(lo, min(lo + 2 * w, npts), nframe).astype(np.int32)
    ids[rng.random(nframe) < 0.2] = -1
    s.frame_ids = ids
    # the parent of a voted keyframe is in the group (or none): the break of :1386 is for the families that ask for it
    g = s.group()
    for k in live:
        lower = g[g < k]
        s.parent[k] = lower[-1] if len(lower) and rng.random() < 0.8 else -1
    return s


def _need(cond):
    assert cond, "the scene generator did not reach the shape the family needs"


def _group_of(nkf, g, rng, stride=64, max_keyframes=80, kfcap=None):
    """exactly g keyframes hold point 0, which the frame holds: a voted group of g with free neighbours and children around"""
    s = base_scene(rng, nkf=nkf, kfcap=kfcap, stride=stride, npts=20 * nkf, p_kf_bad=0.0, p_unset=0.0, max_keyframes=max_keyframes)
    s.entries[s.entries == 0] = -1
    s.entries[(s.entries & ~NO_VOTE) == 0] = -1
    s.pt_bad[0] = 0
    live = s.set_slots()
    chosen = np.sort(rng.permutation(live)[:g])
    for k in chosen:
        s.entries[k, rng.integers(stride)] = 0
    s.frame_ids = np.array([0, -1, 0], np.int32)
    s.parent[:] = -1
    _need(len(s.group()) == g)
    return s


def family_scene(family, seed):
    rng = np.random.default_rng(1000 * (sorted(FAMILIES).index(family) + 1) + seed)
    if family == "random":
        return base_scene(rng)
    if family == "random_wide":
        return base_scene(rng, nkf=150, kfcap=200, stride=65, maxc=3, npts=1500, nframe=300, spread=20.0)
    if family == "no_expansion":          # the voted group is larger than max_keyframes: :1343 breaks before the first step
        return _group_of(60, 30, rng, max_keyframes=20)
    if family == "group_at_limit":        # size() == max_keyframes: a step runs, the next one breaks
        return _group_of(60, 20, rng, max_keyframes=20)
    for _ in range(100):                  # (seeded: the same draws every time) until the band leaves room for every family's rewiring
        s = base_scene(rng, p_kf_bad=0.15, spread=5.0)
        g, free, freebad = s.group(), s.free(), s.free(bad=True)
        if len(g) >= 12 and len(free) >= 2 and len(freebad) >= 1:
            break
    _need(len(g) >= 12 and len(free) >= 2 and len(freebad) >= 1)
    if family == "neighbour_first_included":
        _need(len(free) >= 1)
        for i, k in enumerate(g):
            s.neigh[k, :] = -1
            s.neigh[k, :2] = [g[(i + 1) % len(g)], free[i % len(free)]]
    elif family == "neighbour_bad":
        _need(len(free) >= 1 and len(freebad) >= 1)
        for i, k in enumerate(g):
            s.neigh[k, :3] = [freebad[i % len(freebad)], -1, free[i % len(free)]]
    elif family == "neighbours_all_included":
        for i, k in enumerate(g):
            s.neigh[k, :] = [g[(i + 1 + j) % len(g)] for j in range(10)]
    elif family == "child_bad":
        _need(len(free) >= 1 and len(freebad) >= 1)
        for i, k in enumerate(g):
            s.set_children(k, [freebad[i % len(freebad)], free[(i * 7) % len(free)]])
    elif family == "children_full":
        _need(len(free) >= 1)
        for i, k in enumerate(g):
            s.set_children(k, [g[(i + 1 + j) % len(g)] for j in range(s.maxc - 1)] + [free[(i * 3) % len(free)]])
    elif family == "parent_bad_taken":
        _need(len(freebad) >= 1)
        s.parent[g[0]] = freebad[0]
    elif family == "parent_break":        # the third member's parent is free: the loop ends after three steps
        _need(len(free) >= 1)
        s.parent[g[:2]] = -1
        s.parent[g[2]] = free[-1]
        for k in g[:3]:                   # (nothing takes it before the parent test does)
            s.neigh[k][s.neigh[k] == free[-1]] = -1
            s.set_children(k, [c for c in s.children[k, :s.nchildren[k]] if c != free[-1]])
    elif family == "all_voted_bad":
        s.kf_flags[g] |= KF_BAD
    elif family == "no_votes":            # the frame holds points no keyframe lists, bad points, NO_VOTE-only points and holes
        lone = np.arange(s.pool_cap - 16, s.pool_cap, dtype=np.int32)
        bad = np.flatnonzero(s.pt_bad)[:8].astype(np.int32)
        nv = int(s.entries[g[0]][s.entries[g[0]] >= 0][0] & ~NO_VOTE)
        s.entries[(s.entries & ~NO_VOTE) == nv] = nv | NO_VOTE
        s.pt_bad[nv] = 0
        s.frame_ids = np.concatenate([lone, bad, [nv, -1, nv]]).astype(np.int32)
    elif family == "point_twice_in_frame":
        ok = s.frame_ids[s.frame_ids >= 0]
        s.frame_ids = np.concatenate([s.frame_ids, ok[:10], ok[:5]]).astype(np.int32)
    elif family == "point_in_many_keyframes":   # one point in every keyframe at a random slot: its place in L is the first keyframe's
        pt = s.pool_cap - 1
        for k in s.set_slots():
            s.entries[k, rng.integers(s.stride)] = pt | (NO_VOTE if rng.random() < 0.5 else 0)
    elif family == "bad_points":
        s.pt_bad[:s.pool_cap - 16] = rng.random(s.pool_cap - 16) < 0.4
    else:
        raise KeyError(family)
    return s


# family -> the branch counters that must be non-zero in it (seeds 1..10), or a property checked by name in the tests
FAMILIES = {
    "random": ["neighbour_taken", "child_taken", "steps_run"],
    "random_wide": ["neighbour_taken", "steps_run"],
    "no_expansion": ["size_break"],
    "group_at_limit": ["size_break", "steps_run"],
    "neighbour_first_included": ["neighbour_skipped_included", "neighbour_taken"],
    "neighbour_bad": ["neighbour_skipped_bad", "neighbour_taken"],
    "neighbours_all_included": ["neighbours_exhausted"],
    "child_bad": ["child_skipped_bad", "child_taken"],
    "children_full": ["child_taken"],
    "parent_bad_taken": ["parent_bad_taken"],
    "parent_break": ["parent_taken"],
    "all_voted_bad": [],
    "no_votes": [],
    "point_twice_in_frame": [],
    "point_in_many_keyframes": [],
    "bad_points": [],
}


# ---- the restatement
class RefStore(C.Structure):
    _fields_ = [("kfcap", C.c_int), ("stride", C.c_int), ("maxc", C.c_int), ("entries", C.c_void_p), ("kfFlags", C.c_void_p), ("neigh", C.c_void_p),
                ("parent", C.c_void_p), ("nchildren", C.c_void_p), ("children", C.c_void_p), ("ptBad", C.c_void_p), ("poolCap", C.c_int)]


def _declare(L):
    L.lmu_keyframes.restype = None
    L.lmu_points.restype = None
    L.lmu_keyframes_obs.restype = None


def shim():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("localmap_update_ref", _declare)


def _ref_store(s):
    arrs = [np.ascontiguousarray(a) for a in (s.entries, s.kf_flags, s.neigh, s.parent, s.nchildren, s.children, s.pt_bad)]
    st = RefStore(s.kfcap, s.stride, s.children.shape[1], *[p(a) for a in arrs[:6]], p(arrs[6]), s.pool_cap)
    return st, arrs


def ref_keyframes(s, frame_ids=None, max_keyframes=None):
    st, keep = _ref_store(s)
    ids = np.ascontiguousarray(s.frame_ids if frame_ids is None else frame_ids, np.int32)
    hdr, votes, lst = np.zeros(16, np.int32), np.zeros(s.kfcap, np.int32), np.zeros(s.kfcap, np.int32)
    shim().lmu_keyframes(C.byref(st), p(ids), len(ids), int(s.max_keyframes if max_keyframes is None else max_keyframes), p(hdr), p(votes), p(lst))
    return {"no_votes": bool(hdr[0]), "kf_max": int(hdr[1]), "kf": lst[:hdr[2]].copy(), "votes": votes,
            "branches": dict(zip(BRANCHES, [int(x) for x in hdr[3:13]]))}


def observations(s):
    """per pool id, the keyframes whose entries list it with a vote, one per entry (CSR): MapPoint::mObservations over arrays"""
    e = s.entries
    k, _ = np.nonzero((e >= 0) & ((e & NO_VOTE) == 0) & ((s.kf_flags & KF_SET) != 0)[:, None])
    ids = e[(e >= 0) & ((e & NO_VOTE) == 0) & ((s.kf_flags & KF_SET) != 0)[:, None]]
    order = np.argsort(ids, kind="stable")
    start = np.zeros(s.pool_cap + 1, np.int32)
    np.cumsum(np.bincount(ids, minlength=s.pool_cap), out=start[1:])
    return start, np.ascontiguousarray(k[order].astype(np.int32))


def ref_keyframes_from_observations(s, obs, frame_ids=None, max_keyframes=None, store=None):
    st, keep = store or _ref_store(s)
    ids = np.ascontiguousarray(s.frame_ids if frame_ids is None else frame_ids, np.int32)
    hdr, votes, lst = np.zeros(16, np.int32), np.zeros(s.kfcap, np.int32), np.zeros(s.kfcap, np.int32)
    shim().lmu_keyframes_obs(C.byref(st), p(obs[0]), p(obs[1]), p(ids), len(ids), int(s.max_keyframes if max_keyframes is None else max_keyframes),
                             p(hdr), p(votes), p(lst))
    return {"no_votes": bool(hdr[0]), "kf_max": int(hdr[1]), "kf": lst[:hdr[2]].copy(), "votes": votes}


def ref_points(s, kf_list, frame_ids=None):
    st, keep = _ref_store(s)
    ids = np.ascontiguousarray(s.frame_ids if frame_ids is None else frame_ids, np.int32)
    kf = np.ascontiguousarray(kf_list, np.int32)
    cap = s.kfcap * s.stride
    n, L, seen, S = np.zeros(2, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
    shim().lmu_points(C.byref(st), p(kf), len(kf), p(ids), len(ids), cap, p(n), p(L), p(seen), p(S))
    return {"L": L[:n[0]].copy(), "seen": seen[:n[0]].copy(), "S": S[:n[1]].copy()}


def ref_update(s, frame_ids=None, max_keyframes=None):
    """both functions, as orbu_update_local_map returns them"""
    r = ref_keyframes(s, frame_ids, max_keyframes)
    if not r["no_votes"]:
        r.update(ref_points(s, r["kf"], frame_ids))
    return r
