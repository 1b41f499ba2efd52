"""Scene families for orbq_track_pose (tests/test_trackpose_cpu.py, tests/test_gpu_trackpose.py,
tools/trackpose_bench.py): a frame of keypoints on a jittered lattice with random descriptors, one MapPoint per keypoint that the
search view sees within half a pixel of it at the keypoint's octave, a query list and the frame's ids before the search per family;
the restatement (tools/trackpose_ref.hpp through tests/cpp/trackpose_ref_capi.cpp) and an independent numpy model of the merge, the
edge order and both loops written here.  Every family is named after the branch it forces; BRANCH says which counter of the
restatement must be positive (or which relation must hold) on it."""
import ctypes as C
import functools

import numpy as np

import localmap_cases as lc
import poseopt_cases as pc
from orbslamm_amd._lib import KP_DTYPE
from ref_shim import cached_shim, p

NLEVELS = lc.NLEVELS
FLAG_BAD, FLAG_OBSERVED = lc.FLAG_BAD, lc.FLAG_OBSERVED
REF_KEY = np.dtype([("u", "<f4"), ("v", "<f4"), ("octave", "<i4")])
REF_RESULT = np.dtype([("opt", pc.REF_RESULT), ("n_matches", "<i4"), ("n_matches_map", "<i4")])
BRANCH_NAMES = ("nFromBase", "nFromSearch", "nOverwritten", "nNull", "nRepeatedId", "nBadFlagEdge", "nEdges", "nOutlierDiscarded", "nOutlierKept",
                "nInlierObserved", "nInlierUnobserved")
FAMILIES = ("base_only", "search_only", "search_overwrites_base", "same_id_twice", "no_edges", "edges_2", "edges_3", "edges_9", "edges_10",
            "gross_outliers", "unobserved_inliers", "bad_flag_edge")
SEEDS = (1, 2)


def sigma2():
    return pc.inv_level_sigma2(NLEVELS)


def lattice_keys(rng, n):
    """n keypoints on a 15-pixel lattice inside the image, each moved by up to 2 pixels, in random order, octaves 0 .. 3; above
    1 160 keypoints an 11-pixel lattice moved by up to a pixel (2 240 places)"""
    cols, rows, pitch, x0, move = (40, 29, 15.0, 25.0, 2.0) if n <= 40 * 29 else (56, 40, 11.0, 12.0, 1.0)
    assert n <= cols * rows
    cell = rng.permutation(cols * rows)[:n]
    keys = np.zeros(n, KP_DTYPE)
    keys["x"] = x0 + pitch * (cell % cols) + rng.uniform(-move, move, n)
    keys["y"] = x0 + pitch * (cell // cols) + rng.uniform(-move, move, n)
    keys["octave"] = rng.integers(0, 4, n)
    keys["size"], keys["angle"], keys["response"], keys["class_id"] = 31.0, rng.uniform(0, 360, n), 50.0, -1
    return keys


def make_scene(seed, n):
    """the part of a case that the families share: keys, descriptors, the search view, the start pose, a pool of n + 8 slots in
    which feature t's own MapPoint lies at own[t] (every record observed and good, pixel noise 0.4)"""
    rng = np.random.default_rng([seed, n])
    keys = lattice_keys(rng, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    R, t = lc.rot_axis_angle([0.2, 1.0, 0.1], 0.05 + 0.01 * seed), np.array([0.1, -0.05, 0.2])
    view = lc.make_view(R, t)
    pts = lc.points_from_keys(rng, view, keys, lc.SF, desc, jitter=0.4)
    pts["flags"] = FLAG_OBSERVED
    cap = n + 8
    own = rng.permutation(cap)[:n].astype(np.int32)
    pool = np.zeros(cap, lc.POINT_DTYPE)
    pool["flags"] = FLAG_OBSERVED
    pool["max_distance"], pool["min_distance"] = 1.0, 0.1
    pool[own] = pts
    # the start pose: the search view turned by 0.2 degrees and moved by a centimetre
    Rs = lc.rot_axis_angle(rng.normal(size=3), np.deg2rad(0.2)) @ R
    Tcw = pc.tcw_of(Rs, t + 0.01 * rng.normal(size=3) / np.sqrt(3))
    return dict(seed=seed, n=n, keys=keys, desc=desc, view=view, Tcw=Tcw, K=lc.K_A.copy(), pool=pool, own=own, rng=rng)


def with_lists(s, family, base_feat=(), base_of=None, query_feat=()):
    """base ids own[base_of[t]] (or own[t]) at the features base_feat, a shuffled query list of the own points of query_feat; the
    table an exact search returns for it"""
    n, own, rng = s["n"], s["own"], s["rng"]
    base = None
    if len(base_feat) or base_of is not None:
        base = np.full(n, -1, np.int32)
        bf = np.asarray(base_feat, np.int64)
        base[bf] = own[bf]
        for t, src in (base_of or {}).items():
            base[t] = own[src]
    qf = np.asarray(query_feat, np.int64)
    qf = qf[rng.permutation(len(qf))] if len(qf) else qf
    ids = own[qf].astype(np.int32) if len(qf) else np.zeros(0, np.int32)
    assign = None
    if len(qf):
        assign = np.full(n, -1, np.int32)
        assign[qf] = np.arange(len(qf), dtype=np.int32)
    c = dict(s)
    del c["rng"]
    c.update(family=family, base_ids=base, ids=ids, assign=assign)
    return c


def make_case(family, seed, n=120):
    s = make_scene(seed * 100 + FAMILIES.index(family), n)
    rng = s["rng"]
    feat = rng.permutation(n)
    if family == "base_only":
        return with_lists(s, family, base_feat=feat[:80])
    if family == "search_only":
        return with_lists(s, family, query_feat=feat[:80])
    if family == "search_overwrites_base":
        # twenty features hold ANOTHER feature's point before the search and are matched to their own by it
        wrong = {int(t): int(feat[(k + 7) % 20 + 60]) for k, t in enumerate(feat[:20])}
        return with_lists(s, family, base_feat=feat[60:80], base_of=wrong, query_feat=feat[:60])
    if family == "same_id_twice":
        twice = {int(feat[40 + k]): int(feat[k]) for k in range(6)}       # six features hold the point of a feature that holds it too
        return with_lists(s, family, base_feat=feat[:40], base_of=twice)
    if family == "no_edges":
        return with_lists(s, family, base_of={})
    if family.startswith("edges_"):
        k = int(family.split("_")[1])
        return with_lists(s, family, base_feat=feat[:k - k // 2], query_feat=feat[40:40 + k // 2])
    if family == "gross_outliers":
        wrong = {int(t): int(feat[(k + 3) % 25 + 90]) for k, t in enumerate(feat[:25])}      # 25 wrong points among 85
        return with_lists(s, family, base_feat=feat[25:50], base_of=wrong, query_feat=feat[50:85])
    if family == "unobserved_inliers":
        s["pool"]["flags"][s["own"][feat[:15]]] = 0                       # given through the base: the search is not asked about them
        return with_lists(s, family, base_feat=feat[:40], query_feat=feat[40:80])
    if family == "bad_flag_edge":
        s["pool"]["flags"][s["own"][feat[:10]]] |= FLAG_BAD
        return with_lists(s, family, base_feat=feat[:40], query_feat=feat[40:80])
    raise KeyError(family)


def placement_case(seed, n, features):
    """base ids alone at the given features of an n-feature frame: the carries of the ordered compaction"""
    s = make_scene(seed, n)
    return with_lists(s, "placement", base_feat=np.asarray(features, np.int64), base_of={})


@functools.lru_cache(maxsize=None)
def family_cases(family):
    return tuple(make_case(family, seed) for seed in SEEDS)


# what a family must show in the restatement's branch counters (both discard modes are run on every case)
BRANCH = {
    "base_only": lambda b0, b1, r0, r1: b0["nFromBase"] == 80 and b0["nFromSearch"] == 0,
    "search_only": lambda b0, b1, r0, r1: b0["nFromSearch"] > 60 and b0["nFromBase"] == 0,
    "search_overwrites_base": lambda b0, b1, r0, r1: b0["nOverwritten"] >= 15 and b0["nFromBase"] >= 15,
    "same_id_twice": lambda b0, b1, r0, r1: b0["nRepeatedId"] == 6,
    "no_edges": lambda b0, b1, r0, r1: b0["nEdges"] == 0 and r0["opt"]["rounds"] == 0 and r0["n_matches"] == 0,
    "edges_2": lambda b0, b1, r0, r1: b0["nEdges"] == 2 and r0["opt"]["rounds"] == 0 and r0["n_matches"] == 2,
    "edges_3": lambda b0, b1, r0, r1: b0["nEdges"] == 3 and r0["opt"]["rounds"] == 1,
    "edges_9": lambda b0, b1, r0, r1: b0["nEdges"] == 9 and r0["opt"]["rounds"] == 1,
    "edges_10": lambda b0, b1, r0, r1: b0["nEdges"] == 10 and r0["opt"]["rounds"] == 4,
    "gross_outliers": lambda b0, b1, r0, r1: b1["nOutlierDiscarded"] >= 20 and b0["nOutlierKept"] == b1["nOutlierDiscarded"],
    "unobserved_inliers": lambda b0, b1, r0, r1: b0["nInlierUnobserved"] >= 10 and r0["n_matches"] != r0["n_matches_map"],
    "bad_flag_edge": lambda b0, b1, r0, r1: b0["nBadFlagEdge"] == 10,
}


# ------------------------------------------------------------------ the restatement
def _declare(L):
    assert [L.trackposeref_sizes(i) for i in range(3)] == [REF_KEY.itemsize, REF_RESULT.itemsize, 4 * len(BRANCH_NAMES)]
    vp = C.c_void_p
    L.trackposeref_run.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.trackposeref_motion_model_verdict.argtypes = [C.c_int, C.c_int, C.c_int, vp]
    L.trackposeref_local_map_verdict.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("trackpose_ref", _declare)


def ref_keys(keys):
    k = np.zeros(len(keys), REF_KEY)
    k["u"], k["v"], k["octave"] = keys["x"], keys["y"], keys["octave"]
    return k


def ref_run(case, discard, assign="case", ids=None, base_ids="case", n=None, pool=None, Tcw=None, sig=None, nlevels=None):
    """the restatement on a case (assign / ids / base_ids / n / pool / Tcw override the case's): (rc, result REF_RESULT[1], ids_out,
    outlier_out, branches dict)"""
    L = ref_lib()
    n = case["n"] if n is None else n
    assign = case["assign"] if isinstance(assign, str) else assign
    ids = case["ids"] if ids is None else ids
    base = case["base_ids"] if isinstance(base_ids, str) else base_ids
    pool = case["pool"] if pool is None else pool
    keys = ref_keys(case["keys"])
    a = None if assign is None else np.ascontiguousarray(assign[:n], np.int32)
    i = np.ascontiguousarray(ids, np.int32)
    b = None if base is None else np.ascontiguousarray(base[:n], np.int32)
    pos = np.ascontiguousarray(pool["pos"], np.float32)
    fl = np.ascontiguousarray(pool["flags"], np.uint8)
    T = np.ascontiguousarray(case["Tcw"] if Tcw is None else Tcw, np.float32).reshape(16)
    K = np.ascontiguousarray(case["K"], np.float32)
    sig = sigma2() if sig is None else np.ascontiguousarray(sig, np.float32)
    out = np.zeros(1, REF_RESULT)
    ids_out, outl = np.full(max(n, 1), -2, np.int32), np.zeros(max(n, 1), np.uint8)
    br = np.zeros(len(BRANCH_NAMES), np.int32)
    rc = L.trackposeref_run(p(keys), n, p(a), p(i), i.shape[0], p(b), int(discard), p(T), p(K), p(pos), p(fl), pool.shape[0], p(sig),
                            sig.shape[0] if nlevels is None else nlevels, p(out), p(ids_out), p(outl), p(br))
    return rc, out, ids_out[:n], outl[:n], dict(zip(BRANCH_NAMES, (int(v) for v in br)))


# ------------------------------------------------------------------ the model: numpy, written without looking at the restatement's code
def model_merge(case, assign="case", n=None):
    """(merged ids, the features that become edges in ascending order)"""
    n = case["n"] if n is None else n
    assign = case["assign"] if isinstance(assign, str) else assign
    merged = np.full(n, -1, np.int64) if case["base_ids"] is None else case["base_ids"][:n].astype(np.int64)
    if assign is not None:
        a = np.asarray(assign[:n], np.int64)
        merged = np.where(a >= 0, case["ids"].astype(np.int64)[np.maximum(a, 0)] if len(case["ids"]) else -1, merged)
    return merged, np.flatnonzero(merged >= 0)


def model_run(case, discard, assign="case", n=None):
    """dict(opt REF_RESULT record, ids_out, outlier_out, n_matches, n_matches_map): the solve is poseopt_cases.ref_run (DEFINED) on the
    model's own edge list"""
    merged, feat = model_merge(case, assign, n)
    n = len(merged)
    po = dict(n=len(feat), Tcw=case["Tcw"], K=case["K"], keys_un=case["keys"], feature=feat.astype(np.int32),
              Xw=case["pool"]["pos"][merged[feat]].astype(np.float32).reshape(-1, 3))
    out, per, _, _ = pc.ref_run(pc.DEFINED, [po])
    outlier = np.zeros(n, np.uint8)
    outlier[feat] = per[0]
    ids_out = merged.copy()
    if discard:
        ids_out[outlier != 0] = -1
    alive = (merged >= 0) & (outlier == 0)
    observed = np.zeros(n, bool)
    observed[feat] = (case["pool"]["flags"][merged[feat]] & FLAG_OBSERVED) != 0
    return dict(opt=out[0], ids_out=ids_out.astype(np.int32), outlier_out=outlier, n_matches=int(alive.sum()), n_matches_map=int((alive & observed).sum()))


# ------------------------------------------------------------------ the device side: what tests/test_gpu_trackpose.py and
# tests/one_handle_cases.py share
W, H, NF = lc.W, lc.H, 500
D0 = [0, 0, 0, 0, 0]
CAP = 320                      # the custom frame sets' cap: five chunks of 64 features


class Rig:
    """a matcher; an extractor (device memory for custom frames, and three real 640 x 480 frames of about 500 features in the four
    slots of `fs`); two frame sets of four slots of CAP features for frames made of given keys"""

    def __init__(self):
        from orbslamm_amd import ORBextractor, ORBmatcher, level_breaks, make_grid, synth
        self.gex = ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=3, device=0)
        self.sf = np.array(self.gex.GetScaleFactors(), np.float32)
        self.m = ORBmatcher(0.8, True, device=0)
        self.grid = make_grid(0.0, 0.0, float(W), float(H))
        self.fs = self.m.frame_set(4, self.gex.max_keypoints, lc.K_A, D0, self.grid, list(lc.BOUNDS), self.sf)
        self.gex.extract_batch_device(*self.gex.upload_frames(synth.make_frames(W, H, 3, stream=17)))
        self.fs.build_from_extractor(0, self.gex)
        self.host = [self.gex.download(f) for f in range(3)]
        self.breaks = level_breaks(lc.LOG_SF, lc.NLEVELS)
        self.sig = sigma2()
        self.cfs = [self.new_set(), self.new_set()]
        self._dev = []

    def new_set(self, cap=CAP):
        return self.m.frame_set(4, cap, lc.K_A, D0, self.grid, list(lc.BOUNDS), self.sf)

    def _up(self, a):
        L, d = self.gex._L, C.c_void_p()
        a = np.ascontiguousarray(a)
        from orbslamm_amd._lib import check, ptr
        check(L.orbx_device_alloc(self.gex._h, C.c_size_t(max(a.nbytes, 4)), C.byref(d)))
        if a.nbytes:
            check(L.orbx_upload(self.gex._h, d, ptr(a), C.c_size_t(a.nbytes)))
        self._dev.append(d)
        return d.value

    def put(self, fs, slot, keys, desc, resident=False):
        """a frame of the given keys into `slot` (no distortion: mvKeysUn is keys); resident: also as an opaque frame for orbo_*"""
        dk, dd, dn = self._up(keys), self._up(desc), self._up(np.array([len(keys)], np.int32))
        fs.build(slot, 1, dk, dd, dn, len(keys))
        fs.sync()
        got, _ = fs.download(slot)
        assert len(got) == len(keys) and all(got[f].tobytes() == keys[f].tobytes() for f in ("x", "y", "octave"))
        return self.m.frame_from_device(dk, dd, len(keys), lc.K_A, D0, self.grid) if resident else None


def new_pool(rig, records):
    from orbslamm_amd import MapPool
    pool = MapPool(rig.m, len(records))
    pool.set(np.arange(len(records)), records)
    return pool


def job(fs, slot, case, back, discard, n=None, base="case", Tcw=None):
    return dict(fs=fs, slot=slot, back=back, base_ids=case["base_ids"] if isinstance(base, str) else base, n=case["n"] if n is None else n, discard=discard,
                Tcw=case["Tcw"] if Tcw is None else Tcw, K=case["K"])


def call(rig, pool, jobs, sig=None, nlevels=None, fill=None):
    from orbslamm_amd.track_pose import pack_jobs, track_pose_raw
    rec, keep = pack_jobs(jobs)
    return track_pose_raw(rig.m._h, pool._h, rec, rig.sig if sig is None else sig, nlevels=nlevels, fill=fill)
