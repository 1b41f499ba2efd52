"""Scene families for OptimizeSim3 (tests/test_sim3opt_cpu.py, tests/test_gpu_sim3opt.py, tools/sim3opt_bench.py): two synthetic
keyframes whose camera frames are related by a ground-truth Sim3 (P1c = s R P2c + t), points seen by both, projected with
TUM-like intrinsics plus Gaussian pixel noise, a perturbed start Sim3; and the restatement (tools/sim3opt_ref.hpp through
tests/cpp/sim3opt_ref_capi.cpp) run on them."""
import ctypes as C
import functools

import numpy as np

from poseopt_cases import K_TUM, inv_level_sigma2, rot_axis_angle
from ref_shim import cached_shim, p

W, H = 640.0, 480.0
NLEVELS = 8
TH2 = 10.0                                   # both call sites (LoopClosing::ComputeSim3, MultiMapper::Run) pass 10
FAMILIES = ("clean", "gross_30", "scale_off", "far_start", "mixed_octaves", "few_left", "behind", "all_wrong")
INTEGER_ONLY = ("few_left", "behind", "all_wrong")   # Serial against Defined: compared on the integer outputs only
# 32 correspondences are 64 edges, the border of the partials; 9 / 10 the early-return border; 1 000 puts 32 edges on a lane
COUNTS = (0, 1, 9, 10, 31, 32, 33, 150, 1000)
SEEDS = (1, 2, 3)                            # the device tests: every family x these x both fix_scale x COUNTS
# OPEN_SEEDS: the first ten seeds, NOT chosen by how the two restatement modes compare (tests/test_sim3opt_cpu.py)
OPEN_SEEDS = tuple(range(1, 11))
OPEN_COUNTS = (1, 9, 10, 31, 32, 33, 150)

REF_PROBLEM = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("R1w", "<f4", (9,)), ("t1w", "<f4", (3,)), ("K1", "<f4", (4,)),
                        ("R2w", "<f4", (9,)), ("t2w", "<f4", (3,)), ("K2", "<f4", (4,)), ("th2", "<f4"), ("fix_scale", "<i4")])
REF_CORR = np.dtype([("obs1", "<f4", (2,)), ("invSigma2_1", "<f4"), ("obs2", "<f4", (2,)), ("invSigma2_2", "<f4"), ("X1w", "<f4", (3,)),
                     ("X2w", "<f4", (3,))])
REF_RESULT = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("written", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"),
                       ("n_in", "<i4"), ("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("lambda_", "<f8", (2,)), ("chi2", "<f8", (2,))])


def quat_of(R):
    """Eigen's Quaterniond(R) through the restatement (x y z w)"""
    q = np.zeros(4)
    ref_lib().sim3optref_quat(p(np.ascontiguousarray(R, dtype=np.float64)), p(q))
    return q


def make_case(family, n, seed, fix_scale=0, K2=None):
    """One problem: dict(q, t, s: the start g2oS12; R1w t1w K1 R2w t2w K2; th2, fix_scale; idx1, obs1, oct1, obs2, oct2, X1w, X2w per
    correspondence; truth=(R, t, s); inlier (bool per correspondence: neither observation was displaced))"""
    rng = np.random.default_rng([seed, n, FAMILIES.index(family)])
    K1 = K_TUM.copy()
    K2 = K_TUM.copy() if K2 is None else np.asarray(K2, dtype=np.float32)
    behind = family == "behind"
    if behind:
        Rt, tt, st = rot_axis_angle([0.3, 1.0, 0.2], np.deg2rad(3.0)), np.array([0.05, -0.03, 0.02]), 1.0
        Rs, ts, ss = np.eye(3), np.zeros(3), 1.0                  # the identity: S12.map(P2c) is P2c exactly
        R2w, t2w = np.eye(3), np.array([0.0, 0.0, 0.25])          # P2c.z = X2w.z + 0.25 exactly
    else:
        Rt, tt, st = rot_axis_angle(rng.normal(size=3), rng.uniform(0.02, 0.25)), rng.uniform(-0.4, 0.4, 3), 1.0
        ang, off, sc = {"far_start": (np.deg2rad(10.0), 0.3, 1.1), "scale_off": (np.deg2rad(1.0), 0.02, 1.3)}.get(family, (np.deg2rad(1.0), 0.02, 1.02))
        d = rng.normal(size=3)
        Rs, ts, ss = rot_axis_angle(rng.normal(size=3), ang) @ Rt, tt + off * d / np.linalg.norm(d), st * sc
        R2w, t2w = rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 0.6)), rng.uniform(-1.0, 1.0, 3)
    R1w, t1w = rot_axis_angle(rng.normal(size=3), rng.uniform(0.1, 0.6)), rng.uniform(-1.0, 1.0, 3)
    R1w, R2w = R1w.astype(np.float32), R2w.astype(np.float32)
    t1w, t2w = t1w.astype(np.float32), t2w.astype(np.float32)
    u0, v0 = rng.uniform(60, W - 60, n), rng.uniform(60, H - 60, n)
    depth = rng.uniform(3.0, 8.0, n)
    P1c = np.stack([(u0 - K1[2]) / K1[0] * depth, (v0 - K1[3]) / K1[1] * depth, depth], axis=1)
    P2c = (P1c - tt) @ Rt / st                                    # R^T (P1c - t) / s
    X1w = ((P1c - t1w.astype(np.float64)) @ R1w.astype(np.float64)).astype(np.float32)
    X2w = ((P2c - t2w.astype(np.float64)) @ R2w.astype(np.float64)).astype(np.float32)
    if behind and n >= 3:
        k = min(4, n - 2)
        X2w[:k, 2] = np.float32(-0.25) - rng.uniform(0.5, 2.0, k).astype(np.float32)   # behind camera 2
        X2w[0, 2] = np.float32(-0.25)                                                  # exactly on its plane
    P1c = X1w.astype(np.float64) @ R1w.astype(np.float64).T + t1w                      # (of the float positions)
    P2c = X2w.astype(np.float64) @ R2w.astype(np.float64).T + t2w
    mixed = family == "mixed_octaves"
    oct1 = rng.integers(0, NLEVELS, n) if mixed else np.zeros(n, dtype=np.int64)
    oct2 = rng.integers(0, NLEVELS, n) if mixed else np.zeros(n, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        obs1 = np.stack([K1[0] * P1c[:, 0] / P1c[:, 2] + K1[2], K1[1] * P1c[:, 1] / P1c[:, 2] + K1[3]], axis=1)
        obs2 = np.stack([K2[0] * P2c[:, 0] / P2c[:, 2] + K2[2], K2[1] * P2c[:, 1] / P2c[:, 2] + K2[3]], axis=1)
    obs2 = np.where(np.isfinite(obs2), obs2, 0.0)
    obs1 = obs1 + rng.normal(size=(n, 2)) * (0.5 * 1.2 ** oct1)[:, None]
    obs2 = obs2 + rng.normal(size=(n, 2)) * (0.5 * 1.2 ** oct2)[:, None]
    inlier = np.ones(n, dtype=bool)
    if family == "gross_30":
        inlier = ~(rng.random(n) < 0.30)
    elif family == "few_left":
        inlier = np.arange(n) < 6                                 # at most six right: fewer than 10 survive the first check
    elif family == "all_wrong":
        inlier[:] = False
    elif behind and n >= 3:
        inlier[:min(4, n - 2)] = False
    wrong = ~inlier
    if family in ("gross_30",):
        disp = rng.uniform(20.0, 60.0, n)
        th = rng.uniform(0, 2 * np.pi, n)
        side = rng.random(n) < 0.5
        dv = np.stack([disp * np.cos(th), disp * np.sin(th)], axis=1)
        obs1 = obs1 + dv * (wrong & side)[:, None]
        obs2 = obs2 + dv * (wrong & ~side)[:, None]
    elif family in ("few_left", "all_wrong"):
        rnd = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)
        obs1 = np.where(wrong[:, None], rnd, obs1)
    idx1 = np.sort(rng.choice(n + n // 3 + 2, size=n, replace=False)).astype(np.int32)
    return dict(family=family, n=n, seed=seed, q=quat_of(Rs), t=np.asarray(ts, dtype=np.float64), s=float(ss), R1w=R1w.reshape(9), t1w=t1w, K1=K1,
                R2w=R2w.reshape(9), t2w=t2w, K2=K2, th2=np.float32(TH2), fix_scale=int(fix_scale), idx1=idx1, obs1=obs1.astype(np.float32),
                oct1=oct1.astype(np.int32), obs2=obs2.astype(np.float32), oct2=oct2.astype(np.int32), X1w=X1w, X2w=X2w, truth=(Rt, tt, st),
                inlier=inlier)


@functools.lru_cache(maxsize=None)
def family_cases(family):
    """every count x seed x fix_scale of a family, made once"""
    return tuple(make_case(family, n, s, fs) for s in SEEDS for fs in (0, 1) for n in COUNTS)


@functools.lru_cache(maxsize=None)
def open_cases(family):
    """OPEN_COUNTS x OPEN_SEEDS x fix_scale of a family, made once"""
    return tuple(make_case(family, n, s, fs) for s in OPEN_SEEDS for fs in (0, 1) for n in OPEN_COUNTS)


def sim3_distance(a, b):
    """(rotation angle in radians, translation distance, |scale difference|) between two (q, t, s); q x y z w, need not be unit"""
    qa, qb = np.asarray(a[0], np.float64), np.asarray(b[0], np.float64)
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    # the vector part of qa^-1 qb: its norm is sin(angle / 2), exactly 0 for equal quaternions
    v = qa[3] * qb[:3] - qb[3] * qa[:3] - np.cross(qa[:3], qb[:3])
    ang = 2.0 * float(np.arcsin(min(np.linalg.norm(v), 1.0)))
    return ang, float(np.linalg.norm(np.asarray(a[1], np.float64) - np.asarray(b[1], np.float64))), abs(float(a[2]) - float(b[2]))


# ------------------------------------------------------------------ the restatement
def _declare(L):
    assert [L.sim3optref_sizes(i) for i in range(3)] == [REF_PROBLEM.itemsize, REF_CORR.itemsize, REF_RESULT.itemsize]
    L.sim3optref_run.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.sim3optref_run.restype = None
    L.sim3optref_exp.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.sim3optref_quat.argtypes = [C.c_void_p, C.c_void_p]
    L.sim3optref_exp_sweep.argtypes = [C.c_double, C.c_double, C.c_int64, C.c_void_p, C.c_void_p]


def ref_lib():
    """the restatement as a shared object (built once per process)"""
    return cached_shim("sim3opt_ref", _declare)


SERIAL, DEFINED, DEFINED_CACHED = 0, 1, 2


def ref_problem(c):
    r = np.zeros(1, dtype=REF_PROBLEM)
    for k in ("q", "t", "s", "R1w", "t1w", "K1", "R2w", "t2w", "K2", "th2", "fix_scale"):
        r[k][0] = c[k]
    return r


def ref_corrs(c, sig1=None, sig2=None):
    sig1 = inv_level_sigma2() if sig1 is None else sig1
    sig2 = inv_level_sigma2() if sig2 is None else sig2
    e = np.zeros(c["n"], dtype=REF_CORR)
    e["obs1"], e["invSigma2_1"], e["obs2"], e["invSigma2_2"], e["X1w"], e["X2w"] = c["obs1"], sig1[c["oct1"]], c["obs2"], sig2[c["oct2"]], c["X1w"], c["X2w"]
    return e


def ref_run(mode, cases, want_chi2=False, sig1=None, sig2=None):
    """the restatement on a list of cases: (results REF_RESULT array, [removed bytes per case], last_rejected (n, 2),
    [check chi2 (2 passes, 2 n) per case] or None)"""
    L = ref_lib()
    nprob = len(cases)
    probs = np.concatenate([ref_problem(c) for c in cases]) if cases else np.zeros(0, dtype=REF_PROBLEM)
    corrs = [ref_corrs(c, sig1, sig2) for c in cases]
    start = np.concatenate([[0], np.cumsum([c["n"] for c in cases])]).astype(np.int32)
    allc = np.concatenate(corrs) if corrs else np.zeros(0, dtype=REF_CORR)
    out = np.zeros(max(nprob, 1), dtype=REF_RESULT)
    flags = np.zeros(max(int(start[-1]), 1), dtype=np.uint8)
    rej = np.zeros((max(nprob, 1), 2), dtype=np.int32)
    chi = np.zeros(max(4 * int(start[-1]), 1), dtype=np.float64) if want_chi2 else None
    L.sim3optref_run(mode, p(probs), nprob, p(start), p(allc), p(out), p(flags), p(rej), p(chi))
    per = [flags[start[i]:start[i + 1]].copy() for i in range(nprob)]
    chis = [chi[4 * start[i]:4 * start[i + 1]].reshape(2, -1).copy() for i in range(nprob)] if want_chi2 else None
    return out[:nprob], per, rej[:nprob], chis


@functools.lru_cache(maxsize=None)
def family_ref(family, mode):
    """the restatement over family_cases(family), computed once and shared (treat as read-only)"""
    return ref_run(mode, list(family_cases(family)), want_chi2=(mode == SERIAL))


@functools.lru_cache(maxsize=None)
def open_ref(family, mode):
    """the restatement over open_cases(family), computed once and shared (treat as read-only)"""
    return ref_run(mode, list(open_cases(family)), want_chi2=(mode == SERIAL))
