"""Scene families for orbq_track_motion_model (tests/test_motionmodel_cpu.py, tests/test_gpu_motionmodel.py,
tools/motionmodel_bench.py): a current frame of keypoints on a jittered lattice, each seeing its own MapPoint of the pool within
half a pixel under the pose the motion model predicts (tests/trackpose_cases.py's scene); a last frame whose feature i holds the
point of current feature src[i], with that feature's octave, an angle within a few degrees of it and its descriptor with a few bits
flipped; a velocity and a last pose, both with a real rotation, whose float product is the predicted pose.  A family is built from
counts: how many of the last frame's points stay where they are seen (true), how many are moved 22 .. 28 scaled pixels away (far:
only the search with 2 * th finds them) or 6 scaled pixels (gross: inside the first window, beyond chi-square), and nothing else in
the last frame.  The restatement (tools/motionmodel_ref.hpp through tests/cpp/motionmodel_ref_capi.cpp) and an independent model of
the chain.  Every family is named after the exit or branch it forces; BRANCH says what the restatement's counters and result must
show."""
import ctypes as C
import functools

import numpy as np

import localmap_cases as lc
import reloc_cases as rc
import trackpose_cases as tc
from orbslamm_amd._lib import KP_DTYPE, OrbmGrid
from ref_shim import cached_shim, p

f32 = np.float32
W, H = lc.W, lc.H
N, NQ = 300, 250
TH, MIN_MATCHES = 15.0, 20
FLAG_OBSERVED = tc.FLAG_OBSERVED
TRACKED, TOO_FEW = 0, 1
ST_NOT_RUN = 0xff
REF_KEY = rc.REF_KEY
REF_RESULT = np.dtype([("track", tc.REF_RESULT), ("Tcw_pred", "<f4", (16,)), ("n_search", "<i4", (2,)), ("wide", "<i4"), ("status", "<i4")])
BRANCH_NAMES = ("exit0", "exit1", "retried", "nNoPoint", "nBehindCamera", "nOutU", "nOutV", "nInView", "nEmptyWindow", "nObservedSkipped", "nOverwritten",
                "nContended", "nNoneFree", "nBestAboveDist", "nBestAtDist", "nMatched", "nRotPruned", "nBeyondN", "nDiscarded")
SEEDS = range(1, 6)

# family -> (true, far, gross, how many of the true points are observed, or None: all)
EXIT_FAMILIES = {
    "first_enough": (80, 0, 0, None),
    "first_19_second_enough": (19, 10, 0, None),
    "first_20": (20, 10, 0, None),
    "wide_rescues": (12, 30, 0, None),
    "too_few": (10, 5, 0, None),
    "second_19": (19, 0, 0, None),
    "map_9": (40, 0, 0, 9),
    "map_10": (40, 0, 0, 10),
    "outliers_discarded": (50, 0, 12, None),
}
GATE_FAMILIES = ("no_point", "behind_camera", "outside_u", "outside_v", "empty_window", "contention", "observed_skip", "dist_101_100", "rotation_pruned",
                 "fewer_device_keys", "velocity_rotation")
FAMILIES = tuple(EXIT_FAMILIES) + GATE_FAMILIES


def sigma2():
    return tc.sigma2()


def grid():
    return rc.grid()


def case_grid(case):
    from orbslamm_amd import make_grid
    w, h = case.get("wh", (W, H))
    return make_grid(0.0, 0.0, float(w), float(h))


def pose44(view):
    R, t, _ = lc.camera_of(view)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_case(family, seed, n=N, nq=NQ, counts=None):
    """keys / desc: the current frame; lkeys / ldesc: the last frame; last_ids; pool; velocity, last_Tcw: float32 4 x 4"""
    return build_case(tc.make_scene(seed * 100 + 40 + FAMILIES.index(family), n), family, seed, nq, counts)


BIG_W, BIG_H, BIG_N = 1241, 376, 2000
BIG_K = np.array([718.856, 718.856, 607.1928, 185.2157], dtype=f32)


def big_case(seed=1, true=1000, far=500):
    """one pair of 2 000-feature frames on a 1241 x 376 image: 100 x 20 places on a 12-pixel lattice, each moved by up to a pixel"""
    n = BIG_N
    rng = np.random.default_rng([seed, n, BIG_W])
    cell = rng.permutation(100 * 20)[:n]
    keys = np.zeros(n, KP_DTYPE)
    keys["x"] = 20.0 + 12.0 * (cell % 100) + rng.uniform(-1, 1, n)
    keys["y"] = 20.0 + 12.0 * (cell // 100) + rng.uniform(-1, 1, n)
    keys["octave"] = rng.integers(0, 4, n)
    keys["size"], keys["angle"], keys["response"], keys["class_id"] = 31.0, rng.uniform(0, 360, n), 50.0, -1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    bounds = (0.0, float(BIG_W), 0.0, float(BIG_H))
    view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.05), np.array([0.1, -0.05, 0.2]), K=BIG_K, bounds=bounds)
    pts = lc.points_from_keys(rng, view, keys, lc.SF, desc, jitter=0.4)
    pts["flags"] = FLAG_OBSERVED
    own = rng.permutation(n + 8)[:n].astype(np.int32)
    pool = np.zeros(n + 8, lc.POINT_DTYPE)
    pool["flags"] = FLAG_OBSERVED
    pool["max_distance"], pool["min_distance"] = 1.0, 0.1
    pool[own] = pts
    s = dict(seed=seed, n=n, keys=keys, desc=desc, view=view, K=BIG_K.copy(), pool=pool, own=own, rng=rng, wh=(BIG_W, BIG_H), bounds=bounds)
    return build_case(s, "big", seed, n, (true, far, 0, None))


def build_case(s, family, seed, nq, counts):
    n = s["n"]
    rng = s["rng"]
    keys, desc, pool, own, view = s["keys"], s["desc"], s["pool"], s["own"], s["view"]
    src = rng.permutation(n)[:nq]                      # last feature i holds the point of current feature src[i]
    lkeys = keys[src].copy()                           # (only the octaves and the angles of the last frame's keys are read)
    lkeys["octave"] = keys["octave"][src]
    lkeys["angle"] = np.mod(keys["angle"][src] + rng.uniform(-3, 3, nq).astype(f32), f32(360.0)).astype(f32)
    ldesc = np.stack([rc.flip_bits(rng, desc[t], int(rng.integers(0, 11))) for t in src])
    true, far, gross, observed = counts or EXIT_FAMILIES.get(family, (40, 0, 0, None))
    q = rng.permutation(nq)
    g_true, g_far, g_gross, g_none = np.split(q, np.cumsum([true, far, gross]))
    last_ids = np.full(nq, -1, np.int32)
    kept = np.concatenate([g_true, g_far, g_gross])
    last_ids[kept] = own[src[kept]]
    for group, lo, hi in ((g_far, 22.0, 28.0), (g_gross, 6.0, 6.0)):
        for k in group:
            a, d = rng.uniform(0, 2 * np.pi), rng.uniform(lo, hi) * float(lc.SF[keys["octave"][src[k]]])
            rc.move_in_image(pool, own[src[k]], view, d * np.cos(a), d * np.sin(a))
    if observed is not None:
        pool["flags"][own[src[g_true[observed:]]]] = 0
    n_dev = n
    spare = list(g_none)
    free_ids = np.setdiff1d(np.arange(len(pool)), own)

    def new_point(u, v, z, octave=0):
        """a last-frame feature of its own: a fresh pool slot seen at (u, v); returns (last feature, pool id)"""
        k, pid = spare.pop(), int(free_ids[len(spare) % len(free_ids)])
        pool[pid] = pool[own[0]]
        rc.place_at(pool, pid, view, u, v, z, octave)
        last_ids[k] = pid
        lkeys["octave"][k] = octave
        return k, pid
    if family == "behind_camera":
        new_point(300.0, 200.0, -5.0)
    elif family == "outside_u":
        new_point(W + 40.0, 200.0, 5.0)
    elif family == "outside_v":
        new_point(300.0, -40.0, 5.0)
    elif family == "empty_window":
        new_point(W - 8.0, H - 8.0, 5.0)               # the lattice ends 25 pixels inside the image; octave 0: a window of 15 pixels
    elif family in ("contention", "observed_skip"):
        # last features qa < qb see the same place: current feature ta, whose descriptor is 5 bits from both rows.  qa takes ta.  When
        # qa's point is observed qb skips ta (ORBmatcher.cc:1405-1407) and takes tb, a feature put 6 pixels beside ta at ta's octave,
        # 40 bits away; when it is not, qb takes ta over
        qa, qb = sorted(spare[-2:])
        del spare[-2:]
        ta = int(src[g_true[0]])
        tb = int(np.setdiff1d(np.arange(n), src)[-1])
        last_ids[g_true[0]] = -1
        keys["x"][tb], keys["y"][tb], keys["octave"][tb] = keys["x"][ta] + f32(6.0), keys["y"][ta], keys["octave"][ta]
        for k, qq in enumerate((qa, qb)):
            pid = int(free_ids[k])
            pool[pid] = pool[own[ta]]
            pool["flags"][pid] = FLAG_OBSERVED if family == "observed_skip" else 0
            last_ids[qq] = pid
            lkeys["octave"][qq] = keys["octave"][ta]
            lkeys["angle"][qq] = keys["angle"][ta]
            ldesc[qq] = rc.flip_bits(rng, desc[ta], 5)
        keys["angle"][tb] = keys["angle"][ta]
        desc[tb] = rc.flip_bits(rng, ldesc[qb], 40)
    elif family == "dist_101_100":
        for k, bits in zip(g_true[:2], (101, 100)):
            ldesc[k] = rc.flip_bits(rng, desc[src[k]], bits)
    elif family == "rotation_pruned":
        for j, k in enumerate(g_true[:4]):
            lkeys["angle"][k] = np.mod(lkeys["angle"][k] + f32(90.0 + 60.0 * j), f32(360.0))
    elif family == "fewer_device_keys":
        # the current frame's last 20 features are not on the device: the points of the last frame that are theirs find nobody
        tail = np.arange(n - 20, n)
        gone = np.flatnonzero(np.isin(src, tail))[:4]
        last_ids[gone] = own[src[gone]]
        n_dev = n - 20
    # the predicted pose is the scene's view: mVelocity = D, mLastFrame.mTcw = D^-1 * view, both with a rotation of their own
    D = np.eye(4)
    big = family == "velocity_rotation"
    D[:3, :3] = lc.rot_axis_angle(rng.normal(size=3), 0.5 if big else 0.02 + 0.01 * seed)
    D[:3, 3] = rng.normal(size=3) * (0.5 if big else 0.05)
    velocity, last_Tcw = D.astype(f32), (np.linalg.inv(D) @ pose44(view)).astype(f32)
    c = dict(s)
    del c["rng"]
    c.update(family=family, keys=keys, desc=desc, lkeys=lkeys, ldesc=ldesc, src=src, last_ids=last_ids, nq=nq, n_dev=n_dev, velocity=velocity,
             last_Tcw=last_Tcw, groups=dict(true=g_true, far=g_far, gross=g_gross))
    return c


@functools.lru_cache(maxsize=None)
def family_case(family, seed=1):
    return make_case(family, seed)


# what a family must show in the restatement's counters (b) and result record (r)
BRANCH = {
    "first_enough": lambda b, r: b["exit0"] == 1 and b["retried"] == 0 and r["n_search"][0] >= 70 and r["wide"] == 0 and r["n_search"][1] == -1,
    "first_19_second_enough": lambda b, r: b["exit0"] == 1 and b["retried"] == 1 and r["n_search"][0] == 19 and r["n_search"][1] >= 20 and r["wide"] == 1,
    "first_20": lambda b, r: b["exit0"] == 1 and b["retried"] == 0 and r["n_search"][0] == 20 and r["wide"] == 0,
    "wide_rescues": lambda b, r: b["exit0"] == 1 and b["retried"] == 1 and r["n_search"][0] < 20 and r["n_search"][1] >= 35,
    "too_few": lambda b, r: b["exit1"] == 1 and b["retried"] == 1 and r["n_search"][1] < 19 and r["track"]["n_matches"] == r["n_search"][1],
    "second_19": lambda b, r: b["exit1"] == 1 and b["retried"] == 1 and r["n_search"][0] == 19 and r["n_search"][1] == 19,
    "map_9": lambda b, r: b["exit0"] == 1 and r["track"]["n_matches_map"] == 9 and r["track"]["n_matches"] > 20,
    "map_10": lambda b, r: b["exit0"] == 1 and r["track"]["n_matches_map"] == 10 and r["track"]["n_matches"] > 20,
    "outliers_discarded": lambda b, r: b["exit0"] == 1 and b["nDiscarded"] >= 10,
    "no_point": lambda b, r: b["nNoPoint"] >= 100,
    "behind_camera": lambda b, r: b["nBehindCamera"] >= 1,
    "outside_u": lambda b, r: b["nOutU"] >= 1,
    "outside_v": lambda b, r: b["nOutV"] >= 1,
    "empty_window": lambda b, r: b["nEmptyWindow"] >= 1,
    # (a window may hold a neighbour that an observed point took earlier: nObservedSkipped alone does not tell the two families apart)
    "contention": lambda b, r: b["nOverwritten"] >= 1 and b["nContended"] == 0,
    "observed_skip": lambda b, r: b["nObservedSkipped"] >= 1 and b["nContended"] >= 1 and b["nOverwritten"] == 0,
    "dist_101_100": lambda b, r: b["nBestAboveDist"] >= 1 and b["nBestAtDist"] >= 1,
    "rotation_pruned": lambda b, r: b["nRotPruned"] >= 3,
    "fewer_device_keys": lambda b, r: b["exit0"] == 1,
    "velocity_rotation": lambda b, r: b["exit0"] == 1 and r["n_search"][0] >= 35,
}


# ------------------------------------------------------------------ the restatement
class MotionRefArgs(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("flags", C.c_void_p), ("cap", C.c_int32),
                ("keys", C.c_void_p), ("desc", C.c_void_p), ("nKeys", C.c_int32),
                ("grid", OrbmGrid), ("bounds", C.c_float * 4),
                ("lastKeys", C.c_void_p), ("lastDesc", C.c_void_p), ("nLastKeys", C.c_int32),
                ("invSigma2", C.c_void_p), ("sf", C.c_void_p), ("nlevels", C.c_int32),
                ("lastIds", C.c_void_p), ("nq", C.c_int32), ("n", C.c_int32),
                ("velocity", C.c_float * 16), ("lastTcw", C.c_float * 16), ("K", C.c_float * 4),
                ("th", C.c_float), ("minMatches", C.c_int32), ("checkOri", C.c_int32)]


def _declare(L):
    assert [L.motionref_sizes(i) for i in range(4)] == [REF_KEY.itemsize, REF_RESULT.itemsize, 4 * len(BRANCH_NAMES), C.sizeof(MotionRefArgs)]
    vp = C.c_void_p
    L.motionref_run.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.motionref_pose_product.argtypes = [vp, vp, vp]
    L.motionref_pose_product.restype = None


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("motionmodel_ref", _declare)


def ref_run(case, th=TH, min_matches=MIN_MATCHES, check_ori=True, pool=None, last_ids=None, n=None, sig=None, nlevels=None, br=None):
    """the restatement on a case: (rc, result REF_RESULT[1], ids_out, outlier_out, assign_out, status (2, nq), counters dict)"""
    L = ref_lib()
    pool = case["pool"] if pool is None else pool
    n = case["n"] if n is None else n
    nq = case["nq"]
    keep = dict(pos=np.ascontiguousarray(pool["pos"], f32), flags=np.ascontiguousarray(pool["flags"], np.uint8),
                keys=rc.ref_keys(case["keys"][:case["n_dev"]]), desc=np.ascontiguousarray(case["desc"][:case["n_dev"]], np.uint8),
                lastKeys=rc.ref_keys(case["lkeys"]), lastDesc=np.ascontiguousarray(case["ldesc"], np.uint8),
                invSigma2=sigma2() if sig is None else np.ascontiguousarray(sig, f32), sf=np.ascontiguousarray(lc.SF, f32),
                lastIds=np.ascontiguousarray(case["last_ids"] if last_ids is None else last_ids, np.int32))
    a = MotionRefArgs()
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    a.cap, a.nKeys, a.nLastKeys, a.nq, a.n = len(pool), case["n_dev"], len(case["lkeys"]), nq, n
    a.nlevels = len(keep["invSigma2"]) if nlevels is None else nlevels
    a.grid = case_grid(case)
    a.bounds[:] = [f32(x) for x in case.get("bounds", lc.BOUNDS)]
    a.velocity[:] = np.asarray(case["velocity"], f32).reshape(16)
    a.lastTcw[:] = np.asarray(case["last_Tcw"], f32).reshape(16)
    a.K[:] = np.asarray(case["K"], f32)
    a.th, a.minMatches, a.checkOri = th, min_matches, int(bool(check_ori))
    out = np.zeros(1, REF_RESULT)
    ids_out, outl, asg = np.full(max(n, 1), -2, np.int32), np.zeros(max(n, 1), np.uint8), np.full(max(n, 1), -2, np.int32)
    status = np.zeros((2, max(nq, 1)), np.uint8)
    br = np.zeros(len(BRANCH_NAMES), np.int32) if br is None else br
    code = L.motionref_run(C.byref(a), p(out), p(ids_out), p(outl), p(asg), p(status), p(br))
    return code, out, ids_out[:n], outl[:n], asg[:n], status.reshape(-1)[:2 * nq].reshape(2, nq), dict(zip(BRANCH_NAMES, (int(v) for v in br)))


# ------------------------------------------------------------------ the model: the pose product in numpy float32 scalars summed left to
# right, the frame/frame gates of tools/frustum_ref.hpp (localmap_cases.ref_frame), the oracle's mode-4 search, and trackpose_cases'
# restatement (tools/trackpose_ref.hpp) for the merge, the solve and the loop.  The product, the gates, the search, the retry and the
# gate of :944 share no code with tools/motionmodel_ref.hpp
def model_pose_product(V, T):
    V, T = np.asarray(V, f32).reshape(4, 4), np.asarray(T, f32).reshape(4, 4)
    out = np.zeros((4, 4), f32)
    for r in range(4):
        for c in range(4):
            s = V[r, 0] * T[0, c]
            for k in range(1, 4):
                s = f32(s + V[r, k] * T[k, c])
            out[r, c] = f32(np.float64(s) * 1.0)
    return out


def view_of_pose(T, K, bounds=lc.BOUNDS):
    """the OrbwView record of a 4 x 4 float32 pose as the frame holds it (Ow is not read by the frame/frame gates)"""
    v = lc.make_view(K=np.asarray(K, f32), bounds=bounds)
    v["Rcw"], v["tcw"] = np.asarray(T, f32)[:3, :3].reshape(9), np.asarray(T, f32)[:3, 3]
    return v


def model_run(oracle, case, th=TH, min_matches=MIN_MATCHES, check_ori=True, pool=None):
    """dict(status, wide, n_search, Tcw_pred, track (tc.REF_RESULT record), ids_out, outlier_out, assign, search_status (2, nq))"""
    pool = case["pool"] if pool is None else pool
    n, nd, nq = case["n"], case["n_dev"], case["nq"]
    keys, desc = case["keys"][:nd], case["desc"][:nd]
    T = model_pose_product(case["velocity"], case["last_Tcw"])
    view = view_of_pose(T, case["K"])
    gp = oracle.make_grid_params(0.0, 0.0, float(W), float(H))
    start, idx = oracle.grid_build(gp, keys)
    status = np.full((2, nq), ST_NOT_RUN, np.uint8)
    ids = np.asarray(case["last_ids"], np.int32)

    def search(k, thx):
        ref = lc.ref_frame(view, pool, ids, case["lkeys"]["octave"], thx)
        status[k] = ref["status"]
        occ = np.zeros(nd, np.uint8)
        occ[n:] = 1
        assign, _, nm = oracle.search_by_projection(4, 0.9, check_ori, 100, ref["uvr"], ref["lvl"], case["ldesc"], case["lkeys"]["angle"], ref["valid"], ref["obs"],
                                                    gp, keys, start, idx, desc, occ, np.full(nd, -1, np.int32))
        full = np.full(n, -1, np.int32)
        full[:min(n, nd)] = assign[:min(n, nd)]
        return full, int(nm)
    assign, nm = search(0, f32(th))
    n_search, wide = [nm, -1], 0
    if nm < min_matches:
        assign, nm = search(1, f32(2.0) * f32(th))
        n_search[1], wide = nm, 1
    res = dict(wide=wide, n_search=n_search, Tcw_pred=T.reshape(16), assign=assign, search_status=status)
    merged = np.where(assign >= 0, ids[np.maximum(assign, 0)], -1).astype(np.int32)
    if nm < min_matches:
        track = np.zeros(1, tc.REF_RESULT)
        track["opt"]["Tcw"][0] = T.reshape(16)
        track["n_matches"][0] = nm
        res.update(status=TOO_FEW, track=track[0], ids_out=merged, outlier_out=np.zeros(n, np.uint8))
        return res
    code, out, ids_out, outl, _ = tc.ref_run(dict(case, base_ids=None), 1, assign=assign, ids=ids, n=n, pool=pool, Tcw=T)
    assert code == 0
    res.update(status=TRACKED, track=out[0], ids_out=ids_out, outlier_out=outl)
    return res


# ------------------------------------------------------------------ the device side: what tests/test_gpu_motionmodel.py and
# tools/motionmodel_bench.py share
CAP = 320


class Rig(rc.Rig):
    """reloc_cases' rig: a matcher, device memory for frames made of given keys, two frame sets of four slots of CAP features"""

    def put_case(self, fs, last_slot, cur_slot, case):
        """the case's last frame and its current frame into two slots"""
        self.put(fs, last_slot, case["lkeys"], case["ldesc"])
        self.put(fs, cur_slot, case["keys"][:case["n_dev"]], case["desc"][:case["n_dev"]])


def new_pool(rig, records):
    from orbslamm_amd import MapPool
    pool = MapPool(rig.m, len(records))
    pool.set(np.arange(len(records)), records)
    return pool


def job(fs, last_slot, cur_slot, case, n=None, last_ids=None):
    return dict(fs=fs, cur_slot=cur_slot, last_slot=last_slot, n=case["n"] if n is None else n, last_ids=case["last_ids"] if last_ids is None else last_ids,
                velocity=case["velocity"], last_Tcw=case["last_Tcw"], K=case["K"])


def call(rig, pool, jobs, th=TH, min_matches=MIN_MATCHES, check_ori=True, sig=None, nlevels=None, fill=None, want_tables=True, m=None):
    from orbslamm_amd.track_pose import pack_motion_jobs, track_motion_model_raw
    rec, keep = pack_motion_jobs(jobs)
    return track_motion_model_raw((m or rig.m)._h, pool._h, rec, th, min_matches, check_ori, rig.sig if sig is None else sig, lc.SF, nlevels=nlevels, fill=fill,
                                  want_tables=want_tables)


def assert_job_equals_ref(got, j, ref, tag):
    """ref: motionmodel_cases.ref_run's tuple"""
    code, out, ids, flags, assign, status = got
    rcode, rout, rids, routl, rasg, rstatus, br = ref
    assert code == 0 and rcode == 0, (tag, code, rcode)
    assert out["status"][j] == rout["status"][0] and out["wide"][j] == rout["wide"][0] and np.array_equal(out["n_search"][j], rout["n_search"][0]), \
        (tag, "exit", out["status"][j], out["wide"][j], out["n_search"][j], rout["status"][0], rout["wide"][0], rout["n_search"][0])
    assert out["Tcw_pred"][j].tobytes() == rout["Tcw_pred"][0].tobytes(), (tag, "Tcw_pred")
    assert status[j].tobytes() == rstatus.tobytes(), (tag, "status", np.argwhere(status[j] != rstatus)[:8])
    assert assign[j].tobytes() == rasg.tobytes(), (tag, "assign_out", np.flatnonzero(assign[j] != rasg)[:8])
    assert ids[j].tobytes() == rids.tobytes(), (tag, "ids_out", np.flatnonzero(ids[j] != rids)[:8])
    assert flags[j].tobytes() == routl.tobytes(), (tag, "outlier_out", np.flatnonzero(flags[j] != routl)[:8])
    assert out[j].tobytes() == rout[0].tobytes(), (tag, "OrbqMotionResult", out[j], rout[0])


def same_call(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and all(x.tobytes() == y.tobytes() for k in (2, 3, 4, 5) for x, y in zip(a[k], b[k]))
