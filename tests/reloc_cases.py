"""Scene families for orbq_relocalize (tests/test_reloc_cpu.py, tests/test_gpu_reloc.py): a lost frame of keypoints
on a jittered lattice, each seeing its own MapPoint of the pool within half a pixel (tests/trackpose_cases.py's scene); a candidate
keyframe whose row entry q holds the point of frame feature src[q], with angles within a few degrees of the frame's; the ids a PnP
iterate returned, per family.  A family is built from counts: how many of the row's points PnP hands over at their own feature
(true), how many at a feature that is none of the row's (wrong: solve 1 discards them, the wide search skips them as found, the
narrow search may find them), how many more the row holds untouched (add) or moved by some pixels in the image (off), and nothing
else in the row.  The restatement (tools/reloc_ref.hpp through tests/cpp/reloc_ref_capi.cpp) and an independent Python model of the
chain.  Every family is named after the exit or branch it forces; BRANCH says what the restatement's counters and result must show."""
import ctypes as C
import functools

import numpy as np

import localmap_cases as lc
import poseopt_cases as pc
import trackpose_cases as tc
from orbslamm_amd._lib import OrbmGrid
from ref_shim import cached_shim, p

f32 = np.float32
W, H = lc.W, lc.H
N, NK = 300, 250
NO_VOTE = 1 << 30
FLAG_BAD = tc.FLAG_BAD
KEEP = 0xff
REJECTED, FIRST, WIDE_SHORT, SECOND, NARROW_SHORT, THIRD = range(6)
ST_NOT_RUN, ST_NO_POINT, ST_BAD, ST_FOUND, ST_OUT_OF_IMAGE, ST_DISTANCE, ST_LEVEL_RANGE, ST_IN_VIEW = range(8)
REF_KEY = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
REF_RESULT = np.dtype([("opt", pc.REF_RESULT, (3,)), ("Tcw", "<f4", (16,)), ("exit", "<i4"), ("n_good", "<i4", (3,)), ("n_additional", "<i4", (2,))])
BRANCH_NAMES = ("exit0", "exit1", "exit2", "exit3", "exit4", "exit5",
                "below3Edges", "secondAbove", "secondBelow", "thirdSucceeds", "thirdFails", "nDiscarded1", "nDiscarded3", "nKeptOutlier2",
                "nNull", "nBeyondStride", "nBeyondRow", "nNoVote", "nBad", "nFound", "nBehindCamera", "nOutU", "nOutV", "nDistLow", "nDistHigh",
                "nLevelBelow", "nLevelAbove", "nInView",
                "nEmptyWindow", "nOccupiedSkipped", "nNoneFree", "nBestAboveDistWide", "nBestAboveDistNarrow", "nBestAtDistWide", "nBestAtDistNarrow", "nContended", "nMatched", "nRotPruned", "nBeyondN")
SEEDS = range(1, 11)

# family -> (true, wrong, add, off, pixels the off points are moved by, pixels the wrong points are moved by)
EXIT_FAMILIES = {
    "rejected": (4, 8, 0, 0, 0.0, 0.0),              # 12 ids, 8 gross mismatches
    "first": (60, 0, 0, 0, 0.0, 0.0),                # 60 true correspondences
    "wide_short": (20, 0, 20, 0, 0.0, 0.0),          # 20 true, too few projectable
    "second_high": (20, 0, 45, 0, 0.0, 0.0),         # the wide search's additions carry solve 2 past 50
    "second_low": (20, 0, 0, 35, 6.0, 0.0),          # the added matches sit where chi-square rejects them
    "narrow_short": (20, 0, 15, 20, 6.0, 0.0),       # solve 2 leaves 31..49 and the narrow search adds too few
    "third_succeeds": (20, 20, 20, 14, 6.0, 0.0),    # the narrow search's additions are true correspondences
    "third_fails": (20, 20, 20, 14, 6.0, 2.3),       # additions inside the 3 px window (2.3 px on both axes) but beyond sqrt(5.991 * sigma2)
}
EXIT_OF = {"rejected": REJECTED, "first": FIRST, "wide_short": WIDE_SHORT, "second_high": SECOND, "second_low": SECOND, "narrow_short": NARROW_SHORT,
           "third_succeeds": THIRD, "third_fails": THIRD}
GATE_FAMILIES = ("bad_point", "already_found", "behind_camera", "outside_u", "outside_v", "distance_low", "distance_high", "level_below", "level_above",
                 "empty_window", "contention", "dist_101_100", "dist_65_64", "rotation_pruned", "no_vote", "short_row", "fewer_device_keys")
FAMILIES = tuple(EXIT_FAMILIES) + GATE_FAMILIES


def sigma2():
    return tc.sigma2()


def breaks(log_sf=lc.LOG_SF):
    from orbslamm_amd import level_breaks
    return level_breaks(log_sf, lc.NLEVELS)


def grid():
    from orbslamm_amd import make_grid
    return make_grid(0.0, 0.0, float(W), float(H))


def _camera(view):
    R, t, _ = lc.camera_of(view)
    return R, t, view[0]["K"].astype(np.float64)


def move_in_image(pool, pid, view, du, dv):
    """the point moved so that `view` sees it (du, dv) pixels from where it saw it, at the same depth"""
    R, t, K = _camera(view)
    Xc = R @ pool["pos"][pid].astype(np.float64) + t
    z = Xc[2]
    u, v = K[0] * Xc[0] / z + K[2] + du, K[1] * Xc[1] / z + K[3] + dv
    pool["pos"][pid] = (R.T @ (np.array([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z]) - t)).astype(f32)


def place_at(pool, pid, view, u, v, z, level=0):
    """the point put where `view` sees it at (u, v) and depth z, with distance bounds that predict `level`"""
    R, t, K = _camera(view)
    Xc = np.array([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z])
    Xw = R.T @ (Xc - t)
    pool["pos"][pid] = Xw.astype(f32)
    dist = np.linalg.norm(Xw - view[0]["Ow"].astype(np.float64))
    pool["max_distance"][pid] = f32(0.95 * dist * float(lc.SF[level]))
    pool["min_distance"][pid] = pool["max_distance"][pid] / lc.SF[-1]


def flip_bits(rng, d, k):
    d = d.copy()
    for bit in rng.permutation(256)[:k]:
        d[bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def make_case(family, seed, n=N, nk=NK, counts=None):
    """keys / desc: the lost frame; kang: the keyframe's angles; entries: its row; ids: what PnP hands over; pool; Tcw: PnP's pose"""
    s = tc.make_scene(seed * 100 + 70 + FAMILIES.index(family), n)
    rng = s["rng"]
    keys, desc, pool, own, view = s["keys"], s["desc"], s["pool"], s["own"], s["view"]
    src = rng.permutation(n)[:nk]                      # row entry q holds the point of frame feature src[q]
    extra = np.setdiff1d(np.arange(n), src)            # features whose own point is none of the row's
    kang = rng.uniform(0, 360, nk).astype(f32)
    keys["angle"][src] = np.mod(kang + rng.uniform(-3, 3, nk).astype(f32), f32(360.0)).astype(f32)
    base = "narrow_short" if family in GATE_FAMILIES else family
    if family == "dist_65_64":
        base = "third_succeeds"
    true, wrong, add, off, off_px, wrong_px = counts or EXIT_FAMILIES[base]
    scale = nk / NK if counts is None else 1.0
    true, wrong, add, off = (int(round(c * scale)) for c in (true, wrong, add, off))
    if family == "third_fails":
        keys["octave"][src] = 0                        # the 3 px window and sqrt(5.991) = 2.45 px are level 0's
        for t in src:
            place_at(pool, own[t], view, float(keys["x"][t]), float(keys["y"][t]), 6.0, 0)
            move_in_image(pool, own[t], view, *rng.normal(0, 0.3, 2))
    q = rng.permutation(nk)
    g_true, g_wrong, g_add, g_off, g_none = np.split(q, np.cumsum([true, wrong, add, off]))
    entries = np.full(nk, -1, np.int32)
    kept = np.concatenate([g_true, g_wrong, g_add, g_off])
    entries[kept] = own[src[kept]]
    ids = np.full(n, -1, np.int32)
    ids[src[g_true]] = own[src[g_true]]
    ids[extra[:wrong]] = own[src[g_wrong]]
    for k in g_off:
        a = rng.uniform(0, 2 * np.pi)
        move_in_image(pool, own[src[k]], view, off_px * np.cos(a), off_px * np.sin(a))
    for k in g_wrong:
        if wrong_px:
            move_in_image(pool, own[src[k]], view, wrong_px * rng.choice([-1, 1]), wrong_px * rng.choice([-1, 1]))
    stride, n_dev, log_sf, gone_q = nk, n, lc.LOG_SF, np.zeros(0, np.int64)
    spare = list(g_none)                               # row entries that hold nothing yet, for the gate families' own points
    free_ids = np.setdiff1d(np.arange(len(pool)), own)  # pool slots no feature owns

    def new_point(u, v, z, level=0, like=None):
        """a row entry of its own: a fresh pool slot seen at (u, v); returns (row index, pool id)"""
        k, pid = spare.pop(), int(free_ids[len(spare) % len(free_ids)])
        pool[pid] = pool[own[src[like]]] if like is not None else pool[own[0]]
        pool["desc"][pid] = rng.integers(0, 256, 32, dtype=np.uint8)
        place_at(pool, pid, view, u, v, z, level)
        entries[k] = pid
        return k, pid
    if family == "bad_point":
        pool["flags"][entries[g_add[:5]]] |= FLAG_BAD
    elif family == "behind_camera":
        new_point(300.0, 200.0, -5.0)
    elif family == "outside_u":
        new_point(W + 40.0, 200.0, 5.0)
    elif family == "outside_v":
        new_point(300.0, -40.0, 5.0)
    elif family in ("distance_low", "distance_high", "level_below", "level_above"):
        for k in g_add[:3]:
            pid = entries[k]
            dist = float(np.linalg.norm(pool["pos"][pid].astype(np.float64) - view[0]["Ow"]))
            if family == "distance_low":               # dist < 0.8 min
                pool["min_distance"][pid], pool["max_distance"][pid] = f32(2.0 * dist), f32(8.0 * dist)
            elif family == "distance_high":            # dist > 1.2 max
                pool["min_distance"][pid], pool["max_distance"][pid] = f32(dist / 8.0), f32(dist / 2.0)
            elif family == "level_below":              # ratio 0.84: inside 1.2 max, below level 0 under the 1.1 table
                pool["min_distance"][pid], pool["max_distance"][pid] = f32(dist / 8.0), f32(dist * 0.84)
            else:                                      # ratio 1.2 ** 7.5: level 8
                pool["min_distance"][pid], pool["max_distance"][pid] = f32(dist / 1.1), f32(dist * 1.2 ** 7.5)
        if family == "level_below":
            log_sf = f32(np.log(f32(1.1)))
    elif family == "empty_window":
        new_point(W - 8.0, H - 8.0, 5.0)               # the lattice ends 25 pixels inside the image
    elif family == "contention":
        # row entries qa < qb see the same place: feature ta, whose descriptor is 5 bits from both points'.  qa takes ta; qb's next
        # candidate is tb, a feature put 6 pixels beside ta at ta's octave, 40 bits away, whose own point is none of the row's
        qa, qb = sorted(spare[-2:])
        del spare[-2:]
        ta, tb = int(src[g_add[0]]), int(extra[-1])
        entries[g_add[0]] = -1
        keys["x"][tb], keys["y"][tb], keys["octave"][tb] = keys["x"][ta] + f32(6.0), keys["y"][ta], keys["octave"][ta]
        for k, qq in enumerate((qa, qb)):
            pid = int(free_ids[k])
            pool[pid] = pool[own[ta]]
            pool["desc"][pid] = flip_bits(rng, desc[ta], 5)
            entries[qq] = pid
        desc[tb] = flip_bits(rng, pool["desc"][int(free_ids[1])], 40)
    elif family == "dist_101_100":
        for k, bits in zip(g_add[:2], (101, 100)):
            pool["desc"][entries[k]] = flip_bits(rng, desc[src[k]], bits)
    elif family == "dist_65_64":
        for k, bits in zip(g_wrong[:2], (65, 64)):
            pool["desc"][entries[k]] = flip_bits(rng, desc[src[k]], bits)
    elif family == "rotation_pruned":
        for j, k in enumerate(g_add[:4]):
            keys["angle"][src[k]] = np.mod(keys["angle"][src[k]] + f32(90.0 + 60.0 * j), f32(360.0))
    elif family == "no_vote":
        entries[g_add[:8]] |= NO_VOTE
    elif family == "short_row":
        last = int(np.flatnonzero(entries >= 0).max())
        entries = entries[:min(last + 1, nk - 10)].copy()
    elif family == "fewer_device_keys":
        # the frame's last 20 features are not on the device: none of them holds a point, and none is anybody's match
        tail = np.arange(n - 20, n)
        gone = np.isin(src, tail)
        gone_q = np.flatnonzero(gone & ~np.isin(np.arange(nk), g_true))[:4]   # kept: their own feature is not there to be found
        entries[gone] = -1
        entries[gone_q] = own[src[gone_q]]
        ids[tail] = -1
        n_dev = n - 20
    c = dict(s)
    del c["rng"]
    c.update(family=family, keys=keys, desc=desc, kang=kang, src=src, entries=entries, ids=ids, stride=stride, nk=nk, n_dev=n_dev, log_sf=log_sf,
             groups=dict(true=g_true, wrong=g_wrong, add=g_add, off=g_off), gone_q=gone_q)
    return c


@functools.lru_cache(maxsize=None)
def family_case(family, seed=1):
    return make_case(family, seed)


# what a family must show in the restatement's counters (b) and result record (r)
BRANCH = {
    "rejected": lambda b, r: b["exit0"] == 1 and r["n_good"][0] < 10,
    "first": lambda b, r: b["exit1"] == 1 and r["n_good"][0] >= 50,
    "wide_short": lambda b, r: b["exit2"] == 1 and 0 < r["n_additional"][0] and r["n_additional"][0] + r["n_good"][0] < 50,
    "second_high": lambda b, r: b["exit3"] == 1 and b["secondAbove"] == 1 and r["n_good"][1] >= 50,
    "second_low": lambda b, r: b["exit3"] == 1 and b["secondBelow"] == 1 and r["n_good"][1] <= 30 and b["nKeptOutlier2"] >= 20,
    "narrow_short": lambda b, r: b["exit4"] == 1 and 30 < r["n_good"][1] < 50 and r["n_good"][1] + r["n_additional"][1] < 50,
    "third_succeeds": lambda b, r: b["exit5"] == 1 and b["thirdSucceeds"] == 1 and r["n_additional"][1] >= 10 and r["n_good"][2] >= 50 and b["nDiscarded1"] >= 15,
    "third_fails": lambda b, r: b["exit5"] == 1 and b["thirdFails"] == 1 and r["n_additional"][1] >= 10 and r["n_good"][2] < 50 and b["nDiscarded3"] >= 20,
    "bad_point": lambda b, r: b["nBad"] >= 5,
    "already_found": lambda b, r: b["nFound"] >= 20,
    "behind_camera": lambda b, r: b["nBehindCamera"] >= 1,
    "outside_u": lambda b, r: b["nOutU"] >= 1,
    "outside_v": lambda b, r: b["nOutV"] >= 1,
    "distance_low": lambda b, r: b["nDistLow"] >= 3,
    "distance_high": lambda b, r: b["nDistHigh"] >= 3,
    "level_below": lambda b, r: b["nLevelBelow"] >= 3,
    "level_above": lambda b, r: b["nLevelAbove"] >= 3,
    "empty_window": lambda b, r: b["nEmptyWindow"] >= 1,
    "contention": lambda b, r: b["nContended"] >= 1,
    "dist_101_100": lambda b, r: b["nBestAboveDistWide"] >= 1 and b["nBestAtDistWide"] >= 1,
    "dist_65_64": lambda b, r: b["exit5"] == 1 and b["nBestAboveDistNarrow"] >= 1 and b["nBestAtDistNarrow"] >= 1,
    "rotation_pruned": lambda b, r: b["nRotPruned"] >= 3,
    "no_vote": lambda b, r: b["nNoVote"] >= 8,
    "short_row": lambda b, r: b["nBeyondRow"] >= 10,
    "fewer_device_keys": lambda b, r: r["exit"] != REJECTED,
}


# ------------------------------------------------------------------ the restatement
class RelocRefArgs(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("minD", C.c_void_p), ("maxD", C.c_void_p), ("flags", C.c_void_p), ("pdesc", C.c_void_p), ("cap", C.c_int32),
                ("keys", C.c_void_p), ("desc", C.c_void_p), ("nKeys", C.c_int32),
                ("grid", OrbmGrid), ("bounds", C.c_float * 4),
                ("entries", C.c_void_p), ("nEntries", C.c_int32), ("stride", C.c_int32), ("angles", C.c_void_p), ("nAngles", C.c_int32),
                ("invSigma2", C.c_void_p), ("sf", C.c_void_p), ("breaks", C.c_void_p), ("nlevels", C.c_int32),
                ("ids", C.c_void_p), ("n", C.c_int32),
                ("Tcw", C.c_float * 16), ("K", C.c_float * 4), ("checkOri", C.c_int32)]


def _declare(L):
    assert [L.relocref_sizes(i) for i in range(4)] == [REF_KEY.itemsize, REF_RESULT.itemsize, 4 * len(BRANCH_NAMES), C.sizeof(RelocRefArgs)]
    vp = C.c_void_p
    L.relocref_run.argtypes = [vp, vp, vp, vp, vp, vp]
    L.relocref_n_good.argtypes = [vp]
    L.relocref_verdict.argtypes = [vp]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("reloc_ref", _declare)


def ref_keys(keys):
    k = np.zeros(len(keys), REF_KEY)
    k["x"], k["y"], k["octave"], k["angle"] = keys["x"], keys["y"], keys["octave"], keys["angle"]
    return k


def ref_run(case, check_ori=True, pool=None, ids=None, Tcw=None, n=None, entries=None, kang=None, sig=None, nlevels=None, br=None):
    """the restatement on a case: (rc, result REF_RESULT[1], ids_out, outlier_out, status (2, stride), counters dict)"""
    L = ref_lib()
    pool = case["pool"] if pool is None else pool
    n = case["n"] if n is None else n
    keep = dict(pos=np.ascontiguousarray(pool["pos"], f32), minD=np.ascontiguousarray(pool["min_distance"], f32), maxD=np.ascontiguousarray(pool["max_distance"], f32),
                flags=np.ascontiguousarray(pool["flags"], np.uint8), pdesc=np.ascontiguousarray(pool["desc"], np.uint8),
                keys=ref_keys(case["keys"][:case["n_dev"]]), desc=np.ascontiguousarray(case["desc"][:case["n_dev"]], np.uint8),
                entries=np.ascontiguousarray(case["entries"] if entries is None else entries, np.int32),
                angles=np.ascontiguousarray(case["kang"] if kang is None else kang, f32),
                invSigma2=sigma2() if sig is None else np.ascontiguousarray(sig, f32), sf=np.ascontiguousarray(lc.SF, f32), breaks=breaks(case["log_sf"]),
                ids=np.ascontiguousarray((case["ids"] if ids is None else ids)[:n], np.int32))
    a = RelocRefArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.cap, a.nKeys, a.nEntries, a.stride, a.nAngles = len(pool), case["n_dev"], len(keep["entries"]), case["stride"], len(keep["angles"])
    a.nlevels = len(keep["invSigma2"]) if nlevels is None else nlevels
    a.n, a.checkOri = n, int(bool(check_ori))
    a.grid = grid()
    a.bounds[:] = [f32(x) for x in lc.BOUNDS]
    a.Tcw[:] = np.asarray(case["Tcw"] if Tcw is None else Tcw, f32).reshape(16)
    a.K[:] = np.asarray(case["K"], f32)
    out = np.zeros(1, REF_RESULT)
    ids_out, outl, status = np.full(max(n, 1), -2, np.int32), np.zeros(max(n, 1), np.uint8), np.zeros((2, max(case["stride"], 1)), np.uint8)
    br = np.zeros(len(BRANCH_NAMES), np.int32) if br is None else br
    rc = L.relocref_run(C.byref(a), p(out), p(ids_out), p(outl), p(status), p(br))
    return rc, out, ids_out[:n], outl[:n], status[:, :case["stride"]], dict(zip(BRANCH_NAMES, (int(v) for v in br)))


def ref_n_good(rec):
    return ref_lib().relocref_n_good(p(np.ascontiguousarray(rec)))


# ------------------------------------------------------------------ the model: numpy float32 scalars and Python floats for the gates,
# the oracle's mode-5 search, and for the solve poseopt_cases' DEFINED restatement (tools/poseopt_ref.hpp, which tools/reloc_ref.hpp includes too:
# as in trackpose_cases the solve is shared) on the model's own edge list.  The id list, the gates, sFound, the search and the exits share no code
# with tools/reloc_ref.hpp
def model_project(case, pool, Tcw, K, found, th, brk):
    """the gates of ORBmatcher.cc:1490-1530 per row entry: (status, uvr, lvl, ids)"""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    stride, ent = case["stride"], np.asarray(case["entries"], np.int64)
    status, uvr, lvl, ids = np.full(stride, ST_NO_POINT, np.uint8), np.zeros((stride, 3), f32), np.zeros((stride, 2), np.int8), np.full(stride, -1, np.int64)
    Ow = [f32(-1.0 * sum(float(T[k, i]) * float(T[k, 3]) for k in range(3))) for i in range(3)]
    mn_x, mx_x, mn_y, mx_y = (f32(b) for b in lc.BOUNDS)
    fx, fy, cx, cy = (f32(k) for k in K)
    for q in range(min(stride, len(ent))):
        e = int(ent[q])
        pid = e & ~NO_VOTE
        if e < 0 or pid >= len(pool):
            continue
        ids[q] = pid
        lvl[q] = (-2, 0)
        if pool["flags"][pid] & FLAG_BAD:
            status[q] = ST_BAD
            continue
        if pid in found:
            status[q] = ST_FOUND
            continue
        X = pool["pos"][pid]
        pc3 = []
        for i in range(3):
            t = T[i, 0] * X[0] + T[i, 1] * X[1] + T[i, 2] * X[2]          # float32 scalars: every product and sum rounds
            pc3.append(f32(float(t) * 1.0 + float(T[i, 3]) * 1.0))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            invz = f32(np.float64(1.0) / np.float64(pc3[2]))
            u, v = fx * pc3[0] * invz + cx, fy * pc3[1] * invz + cy
        uvr[q, 0], uvr[q, 1] = u, v
        if not (mn_x <= u <= mx_x and mn_y <= v <= mx_y):
            status[q] = ST_OUT_OF_IMAGE
            continue
        PO = [X[i] - Ow[i] for i in range(3)]
        dist = f32(np.sqrt(sum(float(c) * float(c) for c in PO)))
        mx, mn = pool["max_distance"][pid], pool["min_distance"][pid]
        if dist < f32(0.8) * mn or dist > f32(1.2) * mx:
            status[q] = ST_DISTANCE
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            level = int((f32(mx) / dist > brk).sum()) - 1
        lvl[q] = (level - 1, level + 1)
        if level < 0 or level >= lc.NLEVELS:
            status[q] = ST_LEVEL_RANGE
            continue
        status[q] = ST_IN_VIEW
        uvr[q, 2] = f32(th) * lc.SF[level]
    return status, uvr, lvl, ids


def model_run(oracle, case, check_ori=True, pool=None):
    """dict(exit, n_good, n_additional, opt [records reached], Tcw, ids_out, outlier_out, status (2, stride))"""
    pool = case["pool"] if pool is None else pool
    n, nd, stride = case["n"], case["n_dev"], case["stride"]
    keys, desc = case["keys"][:nd], case["desc"][:nd]
    cur = np.asarray(case["ids"][:n], np.int64).copy()
    outl = np.full(n, KEEP, np.uint8)
    status = np.zeros((2, stride), np.uint8)
    brk = breaks(case["log_sf"])
    gp = oracle.make_grid_params(0.0, 0.0, float(W), float(H))
    start, idx = oracle.grid_build(gp, keys)
    kang = np.zeros(stride, f32)
    kang[:min(stride, len(case["kang"]))] = case["kang"][:stride]
    res = dict(n_good=[0, 0, 0], n_additional=[0, 0], opt=[], Tcw=np.asarray(case["Tcw"], f32).reshape(16).copy())

    def solve():
        feat = np.flatnonzero(cur >= 0)
        po = dict(n=len(feat), Tcw=res["Tcw"].reshape(4, 4), K=case["K"], keys_un=case["keys"], feature=feat.astype(np.int32),
                  Xw=pool["pos"][cur[feat]].astype(f32).reshape(-1, 3))
        out, per, _, _ = pc.ref_run(pc.DEFINED, [po])
        outl[feat] = per[0]
        res["opt"].append(out[0].copy())
        res["Tcw"] = out[0]["Tcw"].copy()
        res["n_good"][len(res["opt"]) - 1] = int(out[0]["n_good"])
        return int(out[0]["n_good"])

    def search(k, found, th, orb_dist):
        st, uvr, lvl, ids = model_project(case, pool, res["Tcw"], case["K"], found, th, brk)
        status[k] = st
        occ = np.ones(nd, np.uint8)
        m = min(n, nd)
        occ[:m] = cur[:m] >= 0
        qdesc = pool["desc"][np.maximum(ids, 0)]
        assign, _, nm = oracle.search_by_projection(5, 0.0, check_ori, orb_dist, uvr, lvl, qdesc, kang, (st == ST_IN_VIEW).astype(np.uint8), None,
                                                    gp, keys, start, idx, desc, occ, np.full(nd, -1, np.int32))
        hit = np.flatnonzero(assign[:m] >= 0)
        cur[hit] = ids[assign[hit]]
        res["n_additional"][k] = int(nm)
        return int(nm)

    def leave(exit):
        res.update(exit=exit, ids_out=cur.astype(np.int32), outlier_out=outl, status=status)
        return res
    found = set(int(i) for i in cur[cur >= 0])
    good = solve()
    if good < 10:
        return leave(REJECTED)
    cur[outl == 1] = -1
    if good >= 50:
        return leave(FIRST)
    if search(0, found, 10.0, 100) + good < 50:
        return leave(WIDE_SHORT)
    good = solve()
    if good >= 50 or good <= 30:
        return leave(SECOND)
    if good + search(1, set(int(i) for i in cur[cur >= 0]), 3.0, 64) < 50:
        return leave(NARROW_SHORT)
    solve()
    cur[(cur >= 0) & (outl == 1)] = -1
    return leave(THIRD)


# ------------------------------------------------------------------ the device side: what tests/test_gpu_reloc.py and tools/reloc_bench.py share
D0 = [0, 0, 0, 0, 0]
CAP = 320


class Rig:
    """a matcher, an extractor (device memory for frames made of given keys), two frame sets of four slots of CAP features"""

    def __init__(self):
        from orbslamm_amd import ORBextractor, ORBmatcher
        self.gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=1, device=0)
        self.m = ORBmatcher(0.9, True, device=0)
        self.grid = grid()
        self.sig = sigma2()
        self.cfs = [self.new_set(), self.new_set()]
        self._dev = []

    def new_set(self, cap=CAP):
        return self.m.frame_set(4, cap, lc.K_A, D0, self.grid, list(lc.BOUNDS), lc.SF)

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

    def put_case(self, fs, kf_slot, slot, case, resident=False):
        """the case's keyframe (its angles are all that is read) and its frame into two slots"""
        self.put(fs, kf_slot, kf_keys(case), np.zeros((case["nk"], 32), np.uint8))
        return self.put(fs, slot, case["keys"][:case["n_dev"]], case["desc"][:case["n_dev"]], resident)


def kf_keys(case):
    rng = np.random.default_rng(case["nk"])
    k = tc.lattice_keys(rng, case["nk"])
    k["angle"] = case["kang"]
    return k


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


def job(fs, kf_slot, slot, kf, case, n=None, ids=None, Tcw=None):
    return dict(fs=fs, kf_slot=kf_slot, slot=slot, kf=kf, n=case["n"] if n is None else n, ids=case["ids"] if ids is None else ids,
                Tcw=case["Tcw"] if Tcw is None else Tcw, K=case["K"])


def call(rig, pool, store, jobs, check_ori=True, sig=None, nlevels=None, fill=None, want_status=True, m=None, log_sf=lc.LOG_SF, brk=None):
    from orbslamm_amd.track_pose import pack_reloc_jobs, relocalize_raw
    rec, keep = pack_reloc_jobs(jobs)
    return relocalize_raw((m or rig.m)._h, pool._h, store._h, rec, check_ori, rig.sig if sig is None else sig, lc.SF, breaks(log_sf) if brk is None else brk,
                          store.stride, nlevels=nlevels, fill=fill, want_status=want_status)


def assert_job_equals_ref(got, j, ref, tag):
    """ref: reloc_cases.ref_run's tuple"""
    rcode, out, ids, flags, status = got
    rrc, rout, rids, routl, rstatus, br = ref
    assert rcode == 0 and rrc == 0, (tag, rcode, rrc)
    assert out["exit"][j] == rout["exit"][0] and np.array_equal(out["n_good"][j], rout["n_good"][0]) and np.array_equal(out["n_additional"][j], rout["n_additional"][0]), \
        (tag, "exit", out["exit"][j], out["n_good"][j], out["n_additional"][j], rout["exit"][0], rout["n_good"][0], rout["n_additional"][0])
    assert status[j].tobytes() == rstatus.tobytes(), (tag, "status", np.argwhere(status[j] != rstatus)[:8])
    assert ids[j].tobytes() == rids.tobytes(), (tag, "ids_out", np.flatnonzero(ids[j] != rids)[:8])
    assert flags[j].tobytes() == routl.tobytes(), (tag, "outlier_out", np.flatnonzero(flags[j] != routl)[:8])
    assert out[j].tobytes() == rout[0].tobytes(), (tag, "OrbqRelocResult", out[j], rout[0])


def same_call(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and all(x.tobytes() == y.tobytes() for k in (2, 3, 4) for x, y in zip(a[k], b[k]))
