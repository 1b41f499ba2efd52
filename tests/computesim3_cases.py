"""Scene families for orby_compute_sim3 (tests/test_computesim3_cpu.py, tests/test_gpu_computesim3.py,
tools/computesim3_bench.py): two keyframes of N features that see one synthetic scene from two maps related by a known similarity
(P1c = s R P2c + t).  Keyframe 1's feature i holds MapPoint A_i (its own descriptor, its position in map 1), keyframe 2's feature
true2[i] is a noisy copy of it within half a pixel of A_i's image under the similarity and holds MapPoint B (position in map 2); the
Sim3 handed to the search is the truth turned by 0.2 degrees and moved by a centimetre.  The restatement (tools/computesim3_ref.hpp
through tests/cpp/computesim3_ref_capi.cpp) and an independent numpy model of the marks, the gates, the agreement, the walk and the
epilogue (no code shared with the restatement; its two searches are the oracle's window_best, its solve sim3opt_ref.hpp on the model's
own correspondence list).  Every family is named after the branch it forces; BRANCH says what the restatement's counters must show."""
import ctypes as C
import functools

import numpy as np

import localmap_cases as lc
import sim3opt_cases as sc
import trackpose_cases as tc
from matcher_cases import noisy_copies
from orbslamm_amd._lib import KP_DTYPE
from poseopt_cases import inv_level_sigma2
from ref_shim import cached_shim, p

f32 = np.float32
N = 300
NLEVELS = lc.NLEVELS
W, H = lc.W, lc.H
FLAG_BAD, FLAG_OBSERVED = lc.FLAG_BAD, lc.FLAG_OBSERVED
NO_VOTE = 1 << 30
TH, TH_HIGH = 7.5, 100
(ST_NO_POINT, ST_MARKED, ST_BAD, ST_DEPTH, ST_OUTSIDE_IMAGE, ST_DISTANCE, ST_LEVEL_RANGE, ST_NO_CANDIDATE, ST_FOUND) = range(9)
REF_KEY = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])
REF_GRID = np.dtype([("minX", "<f4"), ("minY", "<f4"), ("invW", "<f4"), ("invH", "<f4"), ("cols", "<i4"), ("rows", "<i4")])
REF_RESULT = np.dtype([("opt", sc.REF_RESULT), ("n_found", "<i4"), ("n_corr", "<i4")])
BRANCH_NAMES = ("nMarked1", "nMarked2", "nSharedIdx2", "nNull", "nBad", "nBeyondStride", "nDepth", "nOutside", "nDistLow", "nDistHigh", "nLevelOut",
                "nNoCandidate", "nFound12", "nFound21", "nOneWay", "nNew", "nEntering", "nWalkNull1", "nWalkBad", "nWalkNoIndex", "nNoVoteNew", "nRemoved1",
                "nRemoved2", "earlyReturn", "maxIt10", "nNoVoteSearched")
FAMILIES = ("all_new", "inliers_in", "idx2_shared", "null_entries", "bad_points", "no_vote", "short_stride", "behind_camera", "outside_image",
            "distance_range_half", "distance_range_double", "level_out_of_table", "one_way_only", "gross_outliers", "below_ten", "fix_scale", "empty")
DEGENERATE = ("distance_range_half", "distance_range_double", "below_ten", "empty")


def breaks():
    from orbslamm_amd import level_breaks
    return level_breaks(lc.LOG_SF, NLEVELS)


def sigma2():
    return inv_level_sigma2(NLEVELS)


def grid_record():
    """the 64 x 48 grid over the image as the frame set and the oracle hold it"""
    g = np.zeros(1, REF_GRID)
    g["minX"], g["minY"] = 0.0, 0.0
    g["invW"], g["invH"] = f32(64) / f32(f32(W) - f32(0)), f32(48) / f32(f32(H) - f32(0))
    g["cols"], g["rows"] = 64, 48
    return g


def _project(K, P):
    return np.stack([K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]], axis=1)


def make_case(family, seed, n=N):
    rng = np.random.default_rng([seed, n, FAMILIES.index(family) if family in FAMILIES else 90])
    K = lc.K_A.copy()
    Kd = K.astype(np.float64)
    wide = family.startswith("distance_range")
    keys1 = tc.lattice_keys(rng, n)
    if wide:
        keys1["octave"] = rng.integers(0, NLEVELS, n)
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    R1w, t1w = lc.rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 0.6)).astype(f32), rng.uniform(-1.0, 1.0, 3).astype(f32)
    R2w, t2w = lc.rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 0.6)).astype(f32), rng.uniform(-1.0, 1.0, 3).astype(f32)
    Rt, tt, st = lc.rot_axis_angle([0.3, 1.0, 0.2], np.deg2rad(2.0)), np.array([0.05, -0.03, 0.02]), 1.04
    z = rng.uniform(2.0, 15.0, n)
    u = keys1["x"].astype(np.float64) + rng.normal(0, 0.4, n)
    v = keys1["y"].astype(np.float64) + rng.normal(0, 0.4, n)
    P1c = np.stack([(u - Kd[2]) / Kd[0] * z, (v - Kd[3]) / Kd[1] * z, z], axis=1)
    X1w = ((P1c - t1w.astype(np.float64)) @ R1w.astype(np.float64)).astype(f32)
    P1c = X1w.astype(np.float64) @ R1w.astype(np.float64).T + t1w
    P2c = (P1c - tt) @ Rt / st
    X2w = ((P2c - t2w.astype(np.float64)) @ R2w.astype(np.float64)).astype(f32)
    P2c = X2w.astype(np.float64) @ R2w.astype(np.float64).T + t2w
    src2 = rng.permutation(n)                    # keyframe 2's feature j copies keyframe 1's feature src2[j]
    true2 = np.empty(n, np.int64)
    true2[src2] = np.arange(n)
    obs2 = _project(Kd, P2c) + rng.normal(0, 0.4, (n, 2))
    keys2 = np.zeros(n, KP_DTYPE)
    keys2["x"], keys2["y"] = obs2[src2, 0], obs2[src2, 1]
    keys2["octave"] = keys1["octave"][src2]
    keys2["size"], keys2["angle"], keys2["response"], keys2["class_id"] = 31.0, keys1["angle"][src2], 50.0, -1
    desc2 = noisy_copies(rng, desc1, 6)[src2]
    cap = 2 * n + 8
    ids = rng.permutation(cap)
    idA, idB = ids[:n].astype(np.int32), ids[n:2 * n].astype(np.int32)
    pool = np.zeros(cap, lc.POINT_DTYPE)
    pool["flags"] = FLAG_OBSERVED
    pool["max_distance"], pool["min_distance"] = 1.0, 0.1
    sf = lc.SF.astype(np.float64)
    pool["pos"][idA] = X1w
    pool["max_distance"][idA] = (0.95 * np.linalg.norm(P1c, axis=1) * sf[keys1["octave"]]).astype(f32)
    pool["desc"][idA] = desc1
    pool["pos"][idB] = X2w[src2]
    pool["max_distance"][idB] = (0.95 * np.linalg.norm(P2c[src2], axis=1) * sf[keys2["octave"]]).astype(f32)
    pool["desc"][idB] = desc2
    pool["min_distance"] = (pool["max_distance"] / lc.SF[-1]).astype(f32)
    entries1, entries2, stride = idA.copy(), idB.copy(), n
    # the Sim3 the solver hands over
    d = rng.normal(size=3)
    Rs, ts, ss = lc.rot_axis_angle(rng.normal(size=3), np.deg2rad(0.2)) @ Rt, tt + 0.01 * d / np.linalg.norm(d), st * 1.005
    if family == "distance_range_half":
        ss *= 0.5
    elif family == "distance_range_double":
        ss *= 2.0
    R12, t12, s12 = Rs.astype(f32), ts.astype(f32), f32(ss)
    m12_id = m12_idx2 = None
    fix_scale = 0
    pick, pick2 = rng.permutation(n), rng.permutation(n)

    def enter(feat, idx2):
        nonlocal m12_id, m12_idx2
        if m12_id is None:
            m12_id, m12_idx2 = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        m12_id[feat], m12_idx2[feat] = idB[idx2], idx2

    def behind(idx, Pc, Rw, tw):
        Pb = Pc[idx].copy()
        Pb[:, 2] *= -1
        return ((Pb - tw.astype(np.float64)) @ Rw.astype(np.float64)).astype(f32)
    if family in ("inliers_in", "idx2_shared", "gross_outliers"):
        enter(pick[:40], true2[pick[:40]])
    if family == "idx2_shared":
        enter(pick[40:42], true2[[pick[40], pick[40]]])
    elif family == "gross_outliers":
        enter(pick[40:65], true2[np.roll(pick[40:65], 3)])
    elif family == "null_entries":
        entries1[pick[:n // 5]] = -1
        entries2[pick2[:n // 5]] = -1
    elif family == "bad_points":
        pool["flags"][idA[pick[:n // 5]]] |= FLAG_BAD
        pool["flags"][idB[pick2[:n // 5]]] |= FLAG_BAD
    elif family == "no_vote":
        entries1[pick[:n // 6]] |= NO_VOTE
        entries2[pick2[:n // 3]] |= NO_VOTE
    elif family == "short_stride":
        stride = n - 50
        entries1, entries2 = entries1[:stride].copy(), entries2[:stride].copy()
    elif family == "behind_camera":
        pool["pos"][idA[pick[:20]]] = behind(pick[:20], P1c, R1w, t1w)
        pool["pos"][idB[pick2[:20]]] = behind(src2[pick2[:20]], P2c, R2w, t2w)
    elif family == "outside_image":
        Po = P1c[pick[:20]].copy()
        Po[:, 0] = (W + 200.0 - Kd[2]) / Kd[0] * Po[:, 2]
        pool["pos"][idA[pick[:20]]] = ((Po - t1w.astype(np.float64)) @ R1w.astype(np.float64)).astype(f32)
    elif family == "level_out_of_table":
        pool["max_distance"][idA[pick[:20]]] *= f32(5.0)
    elif family == "one_way_only":
        pool["desc"][idB[true2[pick[:20]]]] = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    elif family == "below_ten":
        entries1[pick[8:]] = -1
    elif family == "fix_scale":
        fix_scale = 1
    elif family == "empty":
        entries1[:], entries2[:] = -1, -1
    return dict(family=family, seed=seed, n1=n, n2=n, K=K, keys1=keys1, desc1=desc1, keys2=keys2, desc2=desc2, pool=pool, entries1=entries1,
                entries2=entries2, stride=stride, R1w=R1w.reshape(9), t1w=t1w, R2w=R2w.reshape(9), t2w=t2w, R12=R12.reshape(9), t12=t12, s12=s12,
                q=sc.quat_of(R12.astype(np.float64)), t=t12.astype(np.float64), s=float(s12), m12_id=m12_id, m12_idx2=m12_idx2, fix_scale=fix_scale,
                th=f32(TH), th2=f32(sc.TH2), true2=true2, idA=idA, idB=idB, bounds=np.array(lc.BOUNDS, f32))


@functools.lru_cache(maxsize=None)
def family_case(family):
    return make_case(family, 1)


# what a family must show in the restatement's counters (b) and result record (r)
BRANCH = {
    "all_new": lambda b, r: b["nEntering"] == b["nMarked1"] == b["nMarked2"] == 0 and b["nNew"] == r["n_found"],
    "inliers_in": lambda b, r: b["nMarked1"] == b["nMarked2"] == b["nEntering"] == 40,
    "idx2_shared": lambda b, r: b["nSharedIdx2"] == 1 and b["nMarked1"] == 42 and b["nMarked2"] == 41,
    "null_entries": lambda b, r: b["nNull"] == 2 * (N // 5) and b["nBad"] == 0,
    "bad_points": lambda b, r: b["nBad"] == 2 * (N // 5) and b["nNull"] == 0,
    "no_vote": lambda b, r: b["nNoVoteNew"] >= 20 and b["nWalkNoIndex"] == b["nNoVoteNew"] and b["nNoVoteSearched"] == N // 6 + N // 3,
    "short_stride": lambda b, r: b["nBeyondStride"] == 100,
    "behind_camera": lambda b, r: b["nDepth"] >= 30,
    "outside_image": lambda b, r: b["nOutside"] >= 20,
    "distance_range_half": lambda b, r: b["nDistLow"] >= 10 and b["nDistHigh"] >= 10,
    "distance_range_double": lambda b, r: b["nDistLow"] >= 10 and b["nDistHigh"] >= 10,
    "level_out_of_table": lambda b, r: b["nLevelOut"] >= 20,
    "one_way_only": lambda b, r: b["nOneWay"] >= 15,
    "gross_outliers": lambda b, r: b["nRemoved1"] >= 15 and b["maxIt10"] == 1,
    "below_ten": lambda b, r: b["earlyReturn"] == 1 and r["opt"]["written"] == 0 and r["opt"]["n_in"] == 0 and 0 < r["n_corr"] < 10,
    "fix_scale": lambda b, r: r["opt"]["written"] == 1 and r["opt"]["s"] == np.float64(family_case("fix_scale")["s12"]),
    "empty": lambda b, r: r["n_corr"] == 0 and r["n_found"] == 0 and b["nNull"] == 2 * N and r["opt"]["written"] == 0,
}


# ------------------------------------------------------------------ the restatement
def _declare(L):
    assert [L.computesim3ref_sizes(i) for i in range(5)] == [REF_KEY.itemsize, REF_GRID.itemsize, sc.REF_PROBLEM.itemsize, REF_RESULT.itemsize, 4 * len(BRANCH_NAMES)]
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.computesim3ref_run.argtypes = ([vp] * 5 + [ci] + [vp, vp, ci, vp, ci, vp] * 2 + [vp] * 6 + [ci] + [vp] * 4 + [cf, cf] + [vp] * 9)
    L.computesim3ref_run.restype = None
    L.computesim3ref_verdict.argtypes = [ci]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("computesim3_ref", _declare)


def ref_keys(keys):
    k = np.zeros(len(keys), REF_KEY)
    k["x"], k["y"], k["octave"] = keys["x"], keys["y"], keys["octave"]
    return k


def problem_of(case):
    r = np.zeros(1, sc.REF_PROBLEM)
    for k in ("q", "t", "s", "R1w", "t1w", "R2w", "t2w", "th2", "fix_scale"):
        r[k][0] = case[k]
    r["K1"][0] = r["K2"][0] = case["K"]
    return r


def ref_run(case, pool=None, br=None):
    """the restatement on one case: dict(res REF_RESULT record, match, ids, removed, status, vn, br)"""
    L = ref_lib()
    pool = case["pool"] if pool is None else pool
    n1, n2 = case["n1"], case["n2"]
    c = lambda a, dt: np.ascontiguousarray(a, dt)   # noqa: E731
    pos, mind, maxd = c(pool["pos"], f32), c(pool["min_distance"], f32), c(pool["max_distance"], f32)
    fl, pdesc = c(pool["flags"], np.uint8), c(pool["desc"], np.uint8)
    k1, k2 = ref_keys(case["keys1"]), ref_keys(case["keys2"])
    d1, d2 = c(case["desc1"], np.uint8), c(case["desc2"], np.uint8)
    e1, e2 = c(case["entries1"], np.int32), c(case["entries2"], np.int32)
    b = c(case["bounds"], f32)
    sf, brk, sig = c(lc.SF, f32), c(breaks(), f32), c(sigma2(), f32)
    grid, prob = grid_record(), problem_of(case)
    R12, t12 = c(case["R12"], f32), c(case["t12"], f32)
    mid = None if case["m12_id"] is None else c(case["m12_id"], np.int32)
    midx = None if case["m12_idx2"] is None else c(case["m12_idx2"], np.int32)
    res = np.zeros(1, REF_RESULT)
    match, ids, removed = np.full(max(n1, 1), -2, np.int32), np.full(max(n1, 1), -2, np.int32), np.zeros(max(n1, 1), np.uint8)
    status, vn = np.zeros(max(n1 + n2, 1), np.uint8), np.full(max(n1 + n2, 1), -2, np.int32)
    br = np.zeros(len(BRANCH_NAMES), np.int32) if br is None else br
    L.computesim3ref_run(p(pos), p(mind), p(maxd), p(fl), p(pdesc), pool.shape[0],
                         p(k1), p(d1), n1, p(e1), min(e1.shape[0], case["stride"]), p(b), p(k2), p(d2), n2, p(e2), min(e2.shape[0], case["stride"]), p(b),
                         p(sf), p(sf), p(brk), p(brk), p(sig), p(sig), NLEVELS, p(grid), p(prob), p(R12), p(t12), C.c_float(case["s12"]), C.c_float(case["th"]),
                         p(mid), p(midx), p(res), p(match), p(ids), p(removed), p(status), p(vn), p(br))
    return dict(res=res, match=match[:n1], ids=ids[:n1], removed=removed[:n1], status=status[:n1 + n2], vn=vn[:n1 + n2],
                br=dict(zip(BRANCH_NAMES, (int(x) for x in br))))


@functools.lru_cache(maxsize=None)
def family_ref(family):
    """the restatement on family_case(family), computed once and shared (treat as read-only)"""
    return ref_run(family_case(family))


# ------------------------------------------------------------------ the model: numpy; it shares no code with tools/computesim3_ref.hpp
def _gemm(A, X, c):
    """cv::Mat A*x + c on CV_32F: float products summed left to right, then (float)((double)t + (double)c); X: (n, 3)"""
    A = np.asarray(A, f32).reshape(3, 3)
    t = (A[:, 0][None, :] * X[:, 0][:, None] + A[:, 1][None, :] * X[:, 1][:, None]) + A[:, 2][None, :] * X[:, 2][:, None]
    return (t.astype(np.float64) + np.asarray(c, f32).astype(np.float64)[None, :]).astype(f32)


def model_sim3_pair(case):
    R12, t12, s12 = case["R12"].reshape(3, 3), case["t12"], case["s12"]
    sR12 = (R12.astype(np.float64) * np.float64(s12)).astype(f32)
    sR21 = (R12.T.astype(np.float64) * (1.0 / np.float64(s12))).astype(f32)
    m = (sR21[:, 0] * t12[0] + sR21[:, 1] * t12[1]) + sR21[:, 2] * t12[2]
    return sR12, sR21, (m.astype(np.float64) * -1.0).astype(f32)


def model_ids(case, which, n):
    """(entries as the store holds them over n features, pool ids or -1)"""
    ent = np.full(n, -1, np.int64)
    e = np.asarray(case["entries%d" % which], np.int64)
    k = min(len(e), case["stride"], n)
    ent[:k] = e[:k]
    return ent, np.where(ent >= 0, ent & ~np.int64(NO_VOTE), -1)


def model_pass(oracle, case, pool, frm, already, search=None):
    """one direction: (vnMatch, status) over the features of keyframe `frm` (1 or 2).  search(to, uvr, level, qdesc) -> (bestIdx, bestDist): another
    window search than the oracle's (the device's resident window_best of the existing path)"""
    to = 3 - frm
    n = case["n%d" % frm]
    _, ids = model_ids(case, frm, n)
    sR12, sR21, t21 = model_sim3_pair(case)
    sR, t = (sR21, t21) if frm == 1 else (sR12, case["t12"])
    status = np.full(n, ST_NO_POINT, np.uint8)
    vn = np.full(n, -1, np.int32)
    has = ids >= 0
    status[has] = ST_MARKED
    live = has & ~already.astype(bool)
    rec = pool[np.maximum(ids, 0)]
    status[live] = ST_BAD
    live &= (rec["flags"] & FLAG_BAD) == 0
    pf = _gemm(case["R%dw" % frm], rec["pos"], case["t%dw" % frm])
    pt = _gemm(sR, pf, t)
    status[live] = ST_DEPTH
    live &= ~(pt[:, 2] < 0)
    with np.errstate(all="ignore"):
        invz = (1.0 / pt[:, 2].astype(np.float64)).astype(f32)
        K = case["K"]
        u, v = K[0] * (pt[:, 0] * invz) + K[2], K[1] * (pt[:, 1] * invz) + K[3]
        b = case["bounds"]
        status[live] = ST_OUTSIDE_IMAGE
        live &= (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        dist = np.sqrt((pt.astype(np.float64) ** 2).sum(1)).astype(f32)
        status[live] = ST_DISTANCE
        live &= ~((dist < f32(0.8) * rec["min_distance"]) | (dist > f32(1.2) * rec["max_distance"]))
        ratio = rec["max_distance"] / dist
        level = (ratio[:, None] > breaks()[None, :NLEVELS + 1]).sum(1) - 1
    status[live] = ST_LEVEL_RANGE
    live &= (level >= 0) & (level < NLEVELS)
    q = np.flatnonzero(live)
    if len(q):
        tkeys = case["keys%d" % to]
        uvr = np.stack([u[q], v[q], f32(case["th"]) * lc.SF[level[q]]], axis=1).astype(f32)
        if search is None:
            gp = oracle.make_grid_params(0.0, 0.0, float(W), float(H))
            start, idx = oracle.grid_build(gp, tkeys)
            bi, bd = oracle.window_best(uvr, level[q].astype(np.int8), rec["desc"][q], None, gp, tkeys, start, idx, case["desc%d" % to])
        else:
            bi, bd = search(to, uvr, level[q].astype(np.int8), rec["desc"][q])
        ok = bd <= TH_HIGH
        status[q] = np.where(ok, ST_FOUND, ST_NO_CANDIDATE)
        vn[q[ok]] = bi[ok]
    return vn, status


def model_run(oracle, case, pool=None, search=None, solve=True):
    """dict(n_found, n_corr, match, ids, removed, status, vn, res: the solve's REF_RESULT record, corr: the model's correspondence list as
    (i, i2, id1, id2) rows)"""
    pool = case["pool"] if pool is None else pool
    n1, n2 = case["n1"], case["n2"]
    mid = np.full(n1, -1, np.int64) if case["m12_id"] is None else np.asarray(case["m12_id"], np.int64)
    midx = np.full(n1, -1, np.int64) if case["m12_idx2"] is None else np.asarray(case["m12_idx2"], np.int64)
    already1 = mid >= 0
    already2 = np.zeros(n2, bool)
    sel = already1 & (midx >= 0) & (midx < n2)
    already2[midx[sel]] = True
    vn1, st1 = model_pass(oracle, case, pool, 1, already1, search)
    vn2, st2 = model_pass(oracle, case, pool, 2, already2, search)
    ent2, ids2 = model_ids(case, 2, n2)
    _, ids1 = model_ids(case, 1, n1)
    i1 = np.arange(n1)
    new = (vn1 >= 0) & (vn2[np.maximum(vn1, 0)] == i1)
    match = np.where(new, vn1, np.where(already1, midx, -1))
    id2 = np.where(new, ids2[np.maximum(vn1, 0)], np.where(already1, mid, -1))
    i2 = np.where(new, np.where((ent2[np.maximum(vn1, 0)] & NO_VOTE) != 0, -1, vn1), np.where(already1, midx, -1))
    bad = lambda ids: (pool["flags"][np.maximum(ids, 0)] & FLAG_BAD) != 0   # noqa: E731
    edge = (id2 >= 0) & (ids1 >= 0) & ~bad(ids1) & ~bad(id2) & (i2 >= 0)
    feat = np.flatnonzero(edge)
    k1, k2 = case["keys1"][feat], case["keys2"][i2[feat]]
    item = dict(case, n=len(feat), obs1=np.stack([k1["x"], k1["y"]], 1), oct1=k1["octave"], obs2=np.stack([k2["x"], k2["y"]], 1), oct2=k2["octave"],
                X1w=pool["pos"][ids1[feat]], X2w=pool["pos"][id2[feat]], K1=case["K"], K2=case["K"], S12=(case["q"], case["t"], case["s"]), idx1=feat.astype(np.int32))
    if not solve:   # the searches, the agreement and the walk alone: the correspondence list for another solver (tools/computesim3_bench.py)
        return dict(n_found=int(new.sum()), n_corr=len(feat), item=item, match_in=match, vn=np.concatenate([vn1, vn2]))
    out, rem, _, _ = sc.ref_run(sc.DEFINED_CACHED, [item], sig1=sigma2(), sig2=sigma2())
    gone = feat[rem[0] != 0]
    match_out, ids_out = match.copy(), id2.copy()
    match_out[gone], ids_out[gone] = -1, -1
    removed = np.zeros(n1, np.uint8)
    removed[:len(feat)] = rem[0]
    return dict(n_found=int(new.sum()), n_corr=len(feat), match=match_out.astype(np.int32), ids=ids_out.astype(np.int32), removed=removed,
                status=np.concatenate([st1, st2]), vn=np.concatenate([vn1, vn2]), res=out[0], new=new, feat=feat, i2=i2, id1=ids1, id2=id2, match_in=match, item=item)


# ------------------------------------------------------------------ the device side: what tests/test_gpu_computesim3.py and
# tests/one_handle_cases.py share
D0 = [0, 0, 0, 0, 0]
CAP = 320


class Rig:
    """a matcher, an extractor (device memory for frames made of given keys), two frame sets of four slots of CAP features"""

    def __init__(self, oracle):
        from orbslamm_amd import ORBextractor, ORBmatcher, make_grid
        self.oracle = oracle
        self.gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=1, device=0)
        self.sf = np.array(self.gex.GetScaleFactors(), np.float32)
        assert np.array_equal(self.sf, lc.SF)
        self.m = ORBmatcher(0.7, True, device=0)
        self.grid = make_grid(0.0, 0.0, float(W), float(H))
        self.sig, self.breaks = sigma2(), breaks()
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

    def put_pair(self, fs, slot1, slot2, case, resident=False):
        return self.put(fs, slot1, case["keys1"], case["desc1"], resident), self.put(fs, slot2, case["keys2"], case["desc2"], resident)


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


def job(fs, slot1, slot2, kf1, kf2, case, **kw):
    j = dict(fs=fs, slot1=slot1, slot2=slot2, kf1=kf1, kf2=kf2, n1=case["n1"], n2=case["n2"], R12=case["R12"], t12=case["t12"], s12=case["s12"],
             S12=(case["q"], case["t"], case["s"]), R1w=case["R1w"], t1w=case["t1w"], R2w=case["R2w"], t2w=case["t2w"], K1=case["K"], K2=case["K"],
             bounds1=case["bounds"], bounds2=case["bounds"], th=case["th"], th2=case["th2"], fix_scale=case["fix_scale"], m12_id=case["m12_id"],
             m12_idx2=case["m12_idx2"])
    j.update(kw)
    return j


def call(rig, pool, store, jobs, sig=None, nlevels=None, fill=None, m=None, debug=True):
    from orbslamm_amd.compute_sim3 import compute_sim3_raw, pack_jobs
    rec, keep = pack_jobs(jobs)
    sig = rig.sig if sig is None else sig
    return compute_sim3_raw((m or rig.m)._h, pool._h, store._h, rec, rig.sf, rig.sf, rig.breaks, rig.breaks, sig, sig, nlevels=nlevels, fill=fill, debug=debug)
