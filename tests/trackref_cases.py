"""Scene families for orbq_track_reference (tests/test_trackref_cpu.py, tests/test_gpu_trackref.py,
tools/trackref_bench.py): a keyframe of random descriptors whose feature q holds a MapPoint of the pool, and a current frame whose
features are noisy copies of the keyframe's, permuted, with angles within a few degrees, each seeing its MapPoint within half a
pixel (tests/trackpose_cases.py's scene); a 6-node vocabulary; the keyframe's match list per family.  The restatement
(tools/trackref_ref.hpp through tests/cpp/trackref_ref_capi.cpp), the oracle's SearchByBoW with the validity array, and an
independent numpy model of the validity rule, the masked merge, the gate and the loop (no code shared with the restatement).  Every family is named after
the branch it forces; BRANCH says which counter of the restatement must be positive on it."""
import ctypes as C
import functools

import numpy as np

import localmap_cases as lc
import trackpose_cases as tc
from matcher_cases import noisy_copies
from orbslamm_amd import synth
from ref_shim import cached_shim, p

FLAG_BAD, FLAG_OBSERVED = tc.FLAG_BAD, tc.FLAG_OBSERVED
NO_VOTE = 1 << 30
TRACKED, TOO_FEW, SEARCH_ONLY = 0, 1, 2
REF_RESULT = np.dtype([("track", tc.REF_RESULT), ("n_bow", "<i4"), ("status", "<i4")])
BRANCH_NAMES = ("nNull", "nBad", "nNoVote", "nBeyondStride", "nValid", "gateTaken", "nDiscarded", "nInlierObserved", "nInlierUnobserved", "nRepeatedId")
FAMILIES = ("all_valid", "null_entries", "bad_points", "no_vote", "short_stride", "same_id_twice", "gross_outliers", "unobserved_inliers", "empty_kf")
VOC_K, VOC_L, LEVELSUP = 6, 3, 2      # FeatureVector nodes at level 1: six of them
N = 300                               # about 50 features a node: the register path of the set search


@functools.lru_cache(maxsize=None)
def vocabulary(k=VOC_K, L=VOC_L):
    return synth.make_vocabulary(k, L)


def oracle_voc(oracle, k=VOC_K, L=VOC_L):
    v = vocabulary(k, L)
    return oracle.Vocabulary(k, L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"])


def make_case(family, seed, n=N, nflip=6):
    """keys / desc: the current frame; kkeys / kdesc: the keyframe; src[t]: the keyframe feature that frame feature t copies;
    entries: the keyframe's match list (entries[src[t]] = own[t] before the family's changes); stride: the store's"""
    s = tc.make_scene(seed * 100 + 50 + (FAMILIES.index(family) if family in FAMILIES else 40), n)
    rng = s["rng"]
    kdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kang = rng.uniform(0, 360, n).astype(np.float32)
    src = rng.permutation(n)
    desc = noisy_copies(rng, kdesc, nflip)[src]
    keys = s["keys"].copy()
    keys["angle"] = np.mod(kang[src] + rng.uniform(-3, 3, n).astype(np.float32), np.float32(360.0)).astype(np.float32)
    kkeys = tc.lattice_keys(rng, n)
    kkeys["angle"] = kang
    entries = np.full(n, -1, np.int32)
    entries[src] = s["own"]
    stride = n
    pool = s["pool"]
    pick = rng.permutation(n)
    if family == "null_entries":
        entries[pick[:n // 5]] = -1
    elif family == "bad_points":
        pool["flags"][entries[pick[:n // 5]]] |= FLAG_BAD
    elif family == "no_vote":
        entries[pick[:n // 3]] |= NO_VOTE
    elif family == "short_stride":
        stride = n - 50
        entries = entries[:stride].copy()
    elif family == "same_id_twice":
        entries[pick[6:12]] = entries[pick[:6]]
    elif family == "gross_outliers":
        entries[pick[:25]] = np.roll(entries[pick[:25]], 3)
    elif family == "unobserved_inliers":
        pool["flags"][entries[pick[:40]]] &= ~np.uint8(FLAG_OBSERVED)
    elif family == "empty_kf":
        entries = np.zeros(0, np.int32)
    elif family == "mixed":     # the issue's check: 80 % of the keyframe's features valid, by both causes
        entries[pick[:n // 10]] = -1
        pool["flags"][entries[pick[n // 10:n // 5]]] |= FLAG_BAD
    elif family == "ratio_ori":
        # ten keyframe features whose best frame feature lies at distance 29 and whose second best at 40: 29 < 0.75 * 40 but not
        # < 0.7 * 40 (ORBmatcher.cc:220); ten frame features turned by 90 degrees: pruned by the rotation check alone (:268-287)
        entries[pick[:n // 10]] = -1
        for k in range(10):
            t, t2, t3 = pick[n - 1 - 3 * k], pick[n - 2 - 3 * k], pick[n - 3 - 3 * k]
            bits = rng.permutation(256)
            for tt, sel in ((t, bits[:29]), (t2, bits[29:69])):
                d = kdesc[src[t]].copy()
                for bit in sel:
                    d[bit // 8] ^= np.uint8(1 << (bit % 8))
                desc[tt] = d
            keys["angle"][t2] = keys["angle"][t]
            keys["angle"][t3] = np.mod(keys["angle"][t3] + np.float32(90.0), np.float32(360.0))
    c = dict(s)
    del c["rng"]
    c.update(family=family, keys=keys, desc=desc, kkeys=kkeys, kdesc=kdesc, src=src, entries=entries, stride=stride, nk=n)
    return c


@functools.lru_cache(maxsize=None)
def family_case(family):
    return make_case(family, 1)


# what a family must show in the restatement's counters (b) and result (r)
BRANCH = {
    "all_valid": lambda b, r: b["nValid"] == N and b["nNull"] == b["nBad"] == b["nNoVote"] == b["nBeyondStride"] == 0 and r["status"] == TRACKED,
    "null_entries": lambda b, r: b["nNull"] == N // 5 and b["nBad"] == 0,
    "bad_points": lambda b, r: b["nBad"] == N // 5 and b["nNull"] == 0,
    "no_vote": lambda b, r: b["nNoVote"] == N // 3 and b["nValid"] == N,
    "short_stride": lambda b, r: b["nBeyondStride"] == 50 and b["nValid"] == N - 50,
    "same_id_twice": lambda b, r: b["nRepeatedId"] >= 3,
    "gross_outliers": lambda b, r: b["nDiscarded"] >= 15,
    "unobserved_inliers": lambda b, r: b["nInlierUnobserved"] >= 20 and r["track"]["n_matches"] != r["track"]["n_matches_map"],
    "empty_kf": lambda b, r: b["nNull"] == N and b["gateTaken"] == 1 and r["status"] == TOO_FEW and r["n_bow"] == 0,
}


# ------------------------------------------------------------------ the restatement
def _declare(L):
    assert [L.trackrefref_sizes(i) for i in range(3)] == [tc.REF_KEY.itemsize, REF_RESULT.itemsize, 4 * len(BRANCH_NAMES)]
    vp, ci = C.c_void_p, C.c_int
    L.trackrefref_validity.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp]
    L.trackrefref_validity.restype = None
    L.trackrefref_run.argtypes = [vp, ci, ci, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp]
    L.trackrefref_verdict.argtypes = [ci, ci]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("trackref_ref", _declare)


def _pool_arrays(case, pool):
    pool = case["pool"] if pool is None else pool
    return np.ascontiguousarray(pool["pos"], np.float32), np.ascontiguousarray(pool["flags"], np.uint8), pool.shape[0]


def ref_validity(case, pool=None, entries=None, br=None):
    """(valid[nk], the counters array the call added to)"""
    L = ref_lib()
    pos, fl, cap = _pool_arrays(case, pool)
    ent = np.ascontiguousarray(case["entries"] if entries is None else entries, np.int32)
    valid = np.zeros(max(case["nk"], 1), np.uint8)
    br = np.zeros(len(BRANCH_NAMES), np.int32) if br is None else br
    L.trackrefref_validity(p(ent), ent.shape[0], case["stride"], case["nk"], p(fl), cap, p(valid), p(br))
    return valid[:case["nk"]], br


def ref_run(case, match, solve=1, min_matches=15, pool=None, entries=None, n=None, Tcw=None, sig=None, nlevels=None, br=None):
    """the restatement behind the search: (rc, result REF_RESULT[1], ids_out, outlier_out, counters dict)"""
    L = ref_lib()
    n = case["n"] if n is None else n
    pos, fl, cap = _pool_arrays(case, pool)
    ent = np.ascontiguousarray(case["entries"] if entries is None else entries, np.int32)
    keys = tc.ref_keys(case["keys"])
    m = np.ascontiguousarray(match[:n], np.int32)
    T = np.ascontiguousarray(case["Tcw"] if Tcw is None else Tcw, np.float32).reshape(16)
    K = np.ascontiguousarray(case["K"], np.float32)
    sig = tc.sigma2() if sig is None else np.ascontiguousarray(sig, np.float32)
    out = np.zeros(1, REF_RESULT)
    ids_out, outl = np.full(max(n, 1), -2, np.int32), np.zeros(max(n, 1), np.uint8)
    br = np.zeros(len(BRANCH_NAMES), np.int32) if br is None else br
    rc = L.trackrefref_run(p(ent), ent.shape[0], case["stride"], case["nk"], p(m), p(keys), n, int(solve), int(min_matches), p(T), p(K), p(pos), p(fl), cap,
                           p(sig), sig.shape[0] if nlevels is None else nlevels, p(out), p(ids_out), p(outl), p(br))
    return rc, out, ids_out[:n], outl[:n], dict(zip(BRANCH_NAMES, (int(v) for v in br)))


# ------------------------------------------------------------------ the oracle's search
def oracle_search(oracle, case, valid, nnratio=0.7, check_ori=True, voc=None):
    """SearchByBoW(pKF, F) of the oracle with the validity array (None: all valid): (match over the frame's features, count)"""
    O = voc or oracle_voc(oracle)
    fvq, fvt = O.transform(case["kdesc"], LEVELSUP)[1], O.transform(case["desc"], LEVELSUP)[1]
    m, n = oracle.search_by_bow(case["kdesc"], case["kkeys"]["angle"], valid, fvq, case["desc"], case["keys"]["angle"], None, fvt, nnratio, check_ori, True)
    return m.copy(), int(n)


def ref_whole(oracle, case, solve=1, min_matches=15, nnratio=0.7, check_ori=True, pool=None, entries=None, voc=None):
    """validity -> the oracle's search -> the restatement behind it: (match, n_bow, ref_run's tuple, valid)"""
    valid, br = ref_validity(case, pool=pool, entries=entries)
    match, nb = oracle_search(oracle, case, valid, nnratio, check_ori, voc)
    r = ref_run(case, match, solve, min_matches, pool=pool, entries=entries, br=br)
    assert r[0] == 0 and int(r[1]["n_bow"][0]) == nb
    return match, nb, r, valid


# ------------------------------------------------------------------ the model: numpy; it shares no code with tools/trackref_ref.hpp
def model_validity(case, pool=None, entries=None):
    pool = case["pool"] if pool is None else pool
    ent = np.asarray(case["entries"] if entries is None else entries, np.int64)
    row = np.full(case["nk"], -1, np.int64)
    k = min(len(ent), case["stride"], case["nk"])
    row[:k] = ent[:k]
    ids = np.where(row >= 0, row & ~np.int64(NO_VOTE), -1)
    bad = (pool["flags"][np.maximum(ids, 0)] & FLAG_BAD) != 0
    return ((ids >= 0) & ~bad).astype(np.uint8), ids


def model_run(case, match, solve=1, min_matches=15, pool=None, entries=None):
    """dict(status, n_bow, opt REF_RESULT record or None, ids_out, outlier_out, n_matches, n_matches_map)"""
    pool = case["pool"] if pool is None else pool
    _, ids = model_validity(case, pool, entries)
    n = case["n"]
    match = np.asarray(match[:n], np.int64)
    merged = np.where(match >= 0, ids[np.maximum(match, 0)], -1)
    nb = int((match >= 0).sum())
    if nb < min_matches or not solve:
        return dict(status=TOO_FEW if nb < min_matches else SEARCH_ONLY, n_bow=nb, opt=None, ids_out=merged.astype(np.int32), outlier_out=np.zeros(n, np.uint8),
                    n_matches=nb, n_matches_map=0)
    c = dict(case, pool=pool, base_ids=None, ids=ids.astype(np.int32), assign=match.astype(np.int32))
    m = tc.model_run(c, 1)
    return dict(status=TRACKED, n_bow=nb, opt=m["opt"], ids_out=m["ids_out"], outlier_out=m["outlier_out"], n_matches=m["n_matches"], n_matches_map=m["n_matches_map"])


# ------------------------------------------------------------------ the device side: what tests/test_gpu_trackref.py and
# tests/one_handle_cases.py share
W, H = lc.W, lc.H
D0 = [0, 0, 0, 0, 0]
CAP = 320


class Rig:
    """a matcher, the 6-node vocabulary on both sides, an extractor (device memory for frames made of given keys), two frame sets of
    four slots of CAP features"""

    def __init__(self, oracle):
        from orbslamm_amd import ORBextractor, ORBmatcher, ORBVocabulary, make_grid
        self.oracle = oracle
        self.gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=1, device=0)
        self.sf = np.array(self.gex.GetScaleFactors(), np.float32)
        self.m = ORBmatcher(0.7, True, device=0)
        self.grid = make_grid(0.0, 0.0, float(W), float(H))
        v = vocabulary()
        self.G = ORBVocabulary(VOC_K, VOC_L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)
        self.O = oracle_voc(oracle)
        self.sig = tc.sigma2()
        self.cfs = [self.new_set(), self.new_set()]
        self._dev = []

    def new_set(self, cap=CAP):
        return self.m.frame_set(4, cap, lc.K_A, D0, self.grid, list(lc.BOUNDS), self.sf)

    def _up(self, a):
        from orbslamm_amd._lib import check, ptr
        L, d = self.gex._L, C.c_void_p()
        a = np.ascontiguousarray(a)
        check(L.orbx_device_alloc(self.gex._h, C.c_size_t(max(a.nbytes, 4)), C.byref(d)))
        if a.nbytes:
            check(L.orbx_upload(self.gex._h, d, ptr(a), C.c_size_t(a.nbytes)))
        self._dev.append(d)
        return d.value

    def put(self, fs, slot, keys, desc, resident=False):
        dk, dd, dn = self._up(keys), self._up(desc), self._up(np.array([len(keys)], np.int32))
        fs.build(slot, 1, dk, dd, dn, len(keys))
        fs.sync()
        return self.m.frame_from_device(dk, dd, len(keys), lc.K_A, D0, self.grid) if resident else None

    def put_pair(self, fs, kf_slot, slot, case, resident=False):
        """the case's keyframe and frame into two slots, their BoW computed"""
        self.put(fs, kf_slot, case["kkeys"], case["kdesc"])
        frame = self.put(fs, slot, case["keys"], case["desc"], resident)
        for s in (kf_slot, slot):
            fs.compute_bow(self.G, s, 1, LEVELSUP)
        return frame


def new_world(rig, pool_records, rows, stride, kfcap=4):
    """(pool, store): the records at ids 0 .., keyframe k of the store holding rows[k]"""
    from orbslamm_amd import MapPool
    from orbslamm_amd.map_pool import KeyFrameStore
    pool = MapPool(rig.m, len(pool_records))
    pool.set(np.arange(len(pool_records)), pool_records)
    store = KeyFrameStore(pool, kfcap, stride, 0, 16)
    k = len(rows)
    store.set(np.arange(k), np.zeros(k, np.uint8), [np.asarray(r, np.int32) for r in rows], [[] for _ in range(k)], [-1] * k, [[] for _ in range(k)])
    return pool, store


def job(fs, kf_slot, slot, kf, case, solve=1, n=None, Tcw=None):
    return dict(fs=fs, kf_slot=kf_slot, slot=slot, kf=kf, n=case["n"] if n is None else n, solve=solve, Tcw=case["Tcw"] if Tcw is None else Tcw, K=case["K"])


def call(rig, pool, store, jobs, nnratio=0.7, check_ori=True, min_matches=15, sig=None, nlevels=None, fill=None, want_match=True, m=None):
    from orbslamm_amd.track_pose import pack_ref_jobs, track_reference_raw
    return track_reference_raw((m or rig.m)._h, pool._h, store._h, pack_ref_jobs(jobs), nnratio, check_ori, min_matches, rig.sig if sig is None else sig,
                               nlevels=nlevels, fill=fill, want_match=want_match)
