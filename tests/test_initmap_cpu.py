"""The initial map on the host, no GPU: the ABI of include/orbslamm_initmap.h, the drop-in against the mock, the refusals that
need no GPU, and the restatement (tools/initmap_ref.hpp) against itself and against numpy: its Defined mode against its Serial
mode over every family of initmap_cases.py, its Serial mode against a dense Gauss-Newton written here, the Huber precondition
and the branches its diagnostics must show.

Figures measured on x86-64 / glibc (recorded in DESIGN.md §8aa) and asserted here at 10x:
  Defined against Serial over all 16 families x their sizes x seeds 1 .. 10 (1 370 problems): the verdict and n_points are equal
    everywhere; the outputs are float32 and the two modes' runs end within a float32 step of each other: pose entries (Tcw, Ow,
    scene units) differ by at most 7.5e-9, positions by at most 7.3e-11 of the problem's largest coordinate, the median depth
    in no problem.  Iteration or trial counts differ in 130 of the problems; they are printed, not asserted: rounding decides a
    converged run's last solver calls.
  Serial (robust off) against the Gauss-Newton, the scale gauge fixed through the baseline: see GN_MEASURED below."""
import importlib
import os

import numpy as np
import pytest

import dropin
import initmap_cases as ic
import ref_shim
from orbslamm_amd._lib import KP_DTYPE, ORBX_E_INVALID, ORBX_E_UNSUPPORTED

im = importlib.import_module("orbslamm_amd.initial_map")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured maxima (this file's docstring); the assertions are at 10x
DS_POSE_MEASURED, DS_POS_MEASURED, DS_MEDIAN_MEASURED = 7.5e-9, 7.3e-11, 0.0


def test_header_declares_and_library_exports_the_initmap_block():
    from orbslamm_amd import _lib
    src = open(os.path.join(ROOT, "include", "orbslamm_initmap.h")).read()
    assert "ORBB_MAX_PROBLEMS %d" % im.MAX_PROBLEMS in src and "ORBB_MAX_FEATURES %d" % im.MAX_FEATURES in src and im.MAX_FEATURES == 65535
    assert "ORBB_MAX_ITERATIONS %d" % im.MAX_ITERATIONS in src and im.MAX_ITERATIONS == 20
    for name, value in (("OK", im.OK), ("RESET_DEPTH", im.RESET_DEPTH), ("RESET_TRACKED", im.RESET_TRACKED), ("RESET_NONFINITE", im.RESET_NONFINITE),
                        ("STOP_ITERATIONS", im.STOP_ITERATIONS), ("STOP_TRIALS", im.STOP_TRIALS), ("STOP_RHO_ZERO", im.STOP_RHO_ZERO),
                        ("STOP_FLAT", im.STOP_FLAT)):
        assert "#define ORBB_%s %d" % (name, value) in src, name
    declared = ref_shim.declared("orbslamm_initmap.h", "orbb_")
    assert declared == ["orbb_initial_map", "orbb_initial_map_frames"]
    assert declared == ref_shim.declared("orbslamm_initmap.h")
    assert '#include "orbslamm_initmap.h"' in open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    import orbslamm_amd
    assert orbslamm_amd.initial_map is im.initial_map and orbslamm_amd.initial_map_batch is im.initial_map_batch
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "initmap_ref.hpp"))
    for name in ("orbg_schur.hip", "orbb_kernels.hip", "orbb_host.inc"):
        assert "initmap_ref" not in open(os.path.join(ROOT, "orbslamm_amd", "csrc", name)).read().split("#pragma once")[-1], name


def test_record_sizes_agree_between_mirror_header_and_shim():
    """the mirror's dtypes, the header's static_asserts (orbb_host.inc) and the restatement's records"""
    L = ic.ref_lib()   # (its declare() compares the shim's sizes with the mirror's)
    assert [L.initmapref_sizes(i) for i in range(3)] == [136, 224, 48]
    host = open(os.path.join(ROOT, "orbslamm_amd", "csrc", "orbb_host.inc")).read()
    assert "sizeof(OrbbProblem) == 136 && sizeof(OrbbResult) == 224 && sizeof(OrbbPoint) == 48" in host
    assert (im.PROBLEM_DTYPE.itemsize, im.RESULT_DTYPE.itemsize, im.POINT_DTYPE.itemsize) == (136, 224, 48)
    assert im.RESULT_DTYPE.fields["chi2_first"][1] == 200 and im.POINT_DTYPE.fields["status"][1] == 44


def test_dropin_header_compiles_against_the_mock():
    """include/Tracking_hip.hpp's InitialMapT instantiated on the mock of tests/cpp/initmap_dropin_gpu.cpp (the GPU test runs it)"""
    dropin.syntax_only("initmap_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "Tracking_hip.hpp")).read()
    for member in ("InitialMapT", "Run(", "UpdateNormalAndDepth", "SetWorldPos"):
        assert member in hdr, member


def test_refusals_that_need_no_gpu():
    """the argument checks come before the handle's: with a NULL handle every refusal still names its own reason"""
    from orbslamm_amd import _lib
    L = _lib.lib()
    sig, sf = ic.inv_level_sigma2(), ic.scale_factors()
    base = ic.make_case("noisy", 5, 1)

    def call(resident=False, sig_=sig, sf_=sf, nlevels=None, **change):
        c = dict(base)
        c.update(change)
        pr = np.zeros(1, dtype=im.PROBLEM_DTYPE)
        pr[0] = im.pack_problem(c)
        for k in ("n1", "n2", "iterations", "fixed_second"):
            if "set_" + k in change:
                pr[k][0] = change["set_" + k]
        import ctypes as C
        rc, _, _ = im.initial_map_raw(None, pr, None if resident else [c["keys_un1"]], None if resident else [c["keys_un2"]],
                                      [C.c_void_p(0)] if resident else None, [C.c_void_p(0)] if resident else None, [c["matches12"]], [c["P3D"]], sig_,
                                      sf_, nlevels)
        return rc, L.orbx_last_error().decode()

    assert call() == (ORBX_E_INVALID, "null handle")                    # everything else is in order: the handle is what is missing
    m = base["matches12"].copy()
    i0 = int(np.nonzero(m >= 0)[0][0])
    m[i0] = base["keys_un2"].shape[0]
    rc, msg = call(matches12=m)
    assert rc == ORBX_E_INVALID and "outside the second frame" in msg and "feature %d" % i0 in msg
    m = base["matches12"].copy()
    i0, i1 = [int(v) for v in np.nonzero(m >= 0)[0][:2]]
    m[i1] = m[i0]
    rc, msg = call(matches12=m)
    assert rc == ORBX_E_INVALID and "matched twice" in msg and "feature %d of the second frame" % m[i0] in msg
    k1 = base["keys_un1"].copy()
    k1["octave"][i0] = 8
    rc, msg = call(keys_un1=k1)
    assert rc == ORBX_E_INVALID and "octave 8" in msg
    k2 = base["keys_un2"].copy()
    k2["octave"][base["matches12"][i0]] = -1
    rc, msg = call(keys_un2=k2)
    assert rc == ORBX_E_INVALID and "octave -1" in msg
    k2 = base["keys_un2"].copy()
    k2["x"][base["matches12"][i0]] = np.nan
    assert call(keys_un2=k2)[0] == ORBX_E_INVALID and "not finite" in call(keys_un2=k2)[1]
    for nl in (0, 17, -3):
        rc, msg = call(sig_=np.ones(17, np.float32), sf_=np.ones(17, np.float32), nlevels=nl)
        assert rc == ORBX_E_INVALID and "nlevels" in msg
    assert call(sig_=None, nlevels=8)[0] == ORBX_E_INVALID and call(sf_=None)[0] == ORBX_E_INVALID
    bad_sig = sig.copy()
    bad_sig[2] = np.inf
    assert "not finite" in call(sig_=bad_sig)[1]
    for it in (-1, 21):
        rc, msg = call(set_iterations=it)
        assert rc == ORBX_E_INVALID and "iterations %d" % it in msg
    rc, msg = call(set_fixed_second=1)
    assert rc == ORBX_E_INVALID and "both poses fixed" in msg
    assert call(fixed_first=False, set_fixed_second=1) == (ORBX_E_INVALID, "null handle")   # the second alone may be fixed
    T = base["Tcw2"].copy()
    T[1, 3] = np.nan
    assert "not finite" in call(Tcw2=T)[1]
    P = base["P3D"].copy()
    P[i0, 1] = np.inf
    rc, msg = call(P3D=P)
    assert rc == ORBX_E_INVALID and "position of feature %d" % i0 in msg
    unmatched = int(np.nonzero(base["matches12"] < 0)[0][0])
    P = base["P3D"].copy()
    P[unmatched] = np.nan
    assert call(P3D=P) == (ORBX_E_INVALID, "null handle")                # an unmatched feature's position is not read
    rc, msg = call(set_n1=-1)
    assert rc == ORBX_E_INVALID and "negative" in msg
    rc, msg = call(set_n2=im.MAX_FEATURES + 1)
    assert rc == ORBX_E_UNSUPPORTED and "features in a frame" in msg
    # counts and nulls on the raw entries
    assert L.orbb_initial_map(None, None, -1, None, None, None, None, None, None, 8, None, None) == ORBX_E_INVALID
    assert "negative" in L.orbx_last_error().decode()
    assert L.orbb_initial_map(None, None, im.MAX_PROBLEMS + 1, None, None, None, None, sig.ctypes.data, sf.ctypes.data, 8, None, None) == ORBX_E_UNSUPPORTED
    assert "problems" in L.orbx_last_error().decode()
    assert L.orbb_initial_map(None, None, 1, None, None, None, None, sig.ctypes.data, sf.ctypes.data, 8, None, None) == ORBX_E_INVALID
    assert "null argument" in L.orbx_last_error().decode()
    # more features of initial frames than a call takes, no frame above the ceiling
    many = np.zeros(im.MAX_PROBLEMS, dtype=im.PROBLEM_DTYPE)
    many["n1"], many["fixed_first"] = 2048, 1
    none, zeros, nokeys = np.full(2048, -1, np.int32), np.zeros((2048, 3), np.float32), np.zeros(2048, KP_DTYPE)
    rc, _, _ = im.initial_map_raw(None, many, [nokeys] * im.MAX_PROBLEMS, [nokeys[:0]] * im.MAX_PROBLEMS, None, None, [none] * im.MAX_PROBLEMS,
                                  [zeros] * im.MAX_PROBLEMS, sig, sf)
    assert rc == ORBX_E_UNSUPPORTED and "in one call" in L.orbx_last_error().decode()
    # the key arrays, then the resident entry: the same checks, then a null frame
    rc, _, _ = im.initial_map_raw(None, np.array([im.pack_problem(base)]), None, None, None, None, [base["matches12"]], [base["P3D"]], sig, sf)
    assert rc == ORBX_E_INVALID and "null key arrays" in L.orbx_last_error().decode()
    rc, msg = call(resident=True)
    assert rc == ORBX_E_INVALID and "frame" in msg
    rc, msg = call(resident=True, set_fixed_second=1)
    assert rc == ORBX_E_INVALID and "both poses fixed" in msg
    # zero problems: ORBX_OK at once, whatever else is passed (the handle included)
    assert L.orbb_initial_map(None, None, 0, None, None, None, None, None, None, 0, None, None) == 0
    assert L.orbb_initial_map_frames(None, None, 0, None, None, None, None, None, None, 0, None, None) == 0
    assert KP_DTYPE.itemsize == 28


def test_huber_precondition_on_the_open_seeds():
    """In Serial (and in Defined) no edge's chi2 lies within a relative 1e-6 of the Huber threshold at any linearisation: where
    it did, the other mode could weight the edge the other way for a reason that is no fault.  Asserted, not skipped, on every
    family's open seeds; the generator's noise was fixed before the seeds were looked at."""
    linearised = 0
    for fam in ic.FAMILIES:
        for mode in (ic.SERIAL, ic.DEFINED):
            for c, (res, _, dg) in zip(ic.family_cases(fam), ic.family_ref(fam, mode)):
                assert not (dg["huber_gap"] <= 1e-6), (fam, c["n"], c["seed"], mode, dg["huber_gap"])
                linearised += int(res["iterations"]) if c["n"] else 0
    assert linearised > 10000


def test_defined_against_serial_on_open_seeds():
    """every family, every size, seeds 1 .. 10, none left out: the verdict and n_points are equal; poses, positions and the
    median depth agree to 10x the measured maxima (this file's docstring).  Iteration and trial counts are printed."""
    worst = dict(pose=0.0, pos=0.0, median=0.0)
    differ = 0
    for fam in ic.FAMILIES:
        for c, (rs, ps, _), (rd, pd, _) in zip(ic.family_cases(fam), ic.family_ref(fam, ic.SERIAL), ic.family_ref(fam, ic.DEFINED)):
            tag = (fam, c["n"], c["seed"])
            assert rs["verdict"] == rd["verdict"] and rs["n_points"] == rd["n_points"] == (0 if fam == "no_points" else c["n"]), tag
            assert np.array_equal(ps["matched"], pd["matched"]) and np.array_equal(ps["status"], pd["status"]), tag
            differ += int(rs["iterations"] != rd["iterations"] or rs["trials"] != rd["trials"])
            for name in ("Tcw1", "Tcw2", "Ow1", "Ow2", "Tcw2_scaled"):
                both = np.isfinite(rs[name]) & np.isfinite(rd[name])
                assert np.array_equal(np.isfinite(rs[name]), np.isfinite(rd[name])), tag
                worst["pose"] = max(worst["pose"], float(np.abs(rs[name][both].astype(np.float64) - rd[name][both]).max(initial=0.0)))
            m = ps["matched"] == 1
            for name in ("pos", "pos_scaled"):
                a, b = ps[name][m].astype(np.float64), pd[name][m].astype(np.float64)
                fin = np.isfinite(a) & np.isfinite(b)
                assert np.array_equal(np.isfinite(a), np.isfinite(b)), tag
                if fin.any():
                    worst["pos"] = max(worst["pos"], float(np.abs(a[fin] - b[fin]).max() / max(np.abs(a[fin]).max(), 1e-30)))
            if np.isfinite(rs["median_depth"]) and rs["median_depth"] != 0:
                worst["median"] = max(worst["median"], abs(float(rs["median_depth"]) - float(rd["median_depth"])) / abs(float(rs["median_depth"])))
            else:
                assert rs["median_depth"].tobytes() == rd["median_depth"].tobytes(), tag
    print("Defined against Serial, open seeds: pose %.3g, positions %.3g (relative), median depth %.3g (relative); "
          "iteration or trial counts differ in %d problems" % (worst["pose"], worst["pos"], worst["median"], differ))
    assert worst["pose"] <= 10 * DS_POSE_MEASURED and worst["pos"] <= 10 * DS_POS_MEASURED and worst["median"] <= 10 * DS_MEDIAN_MEASURED


def test_the_diagnostics_show_the_branches():
    """far_start rejects at least one trial; ten_trials ends by the trial limit; from_truth ends by _nBad (at the sizes where the
    problem is determined: with one or two points the chi2 reaches zero and a gain of exactly zero ends the run first); the
    verdict families give their verdicts; z_zero's plane variant has a non-finite chi2 and rejects every trial"""
    for mode in (ic.SERIAL, ic.DEFINED):
        assert sum(int(dg["rejected_trials"]) for _, _, dg in ic.family_ref("far_start", mode)) >= 1
        for c, (res, _, dg) in zip(ic.family_cases("ten_trials"), ic.family_ref("ten_trials", mode)):
            assert res["stop"] == im.STOP_TRIALS and res["iterations"] == 1 and res["trials"] == 10 and dg["failed_solves"] == 10, (c["n"], c["seed"])
        for c, (res, _, _) in zip(ic.family_cases("from_truth"), ic.family_ref("from_truth", mode)):
            if c["n"] >= 63:
                assert res["stop"] == im.STOP_FLAT, (c["n"], c["seed"], res["stop"])
        for c, (res, _, _) in zip(ic.family_cases("behind"), ic.family_ref("behind", mode)):
            assert res["verdict"] == im.RESET_DEPTH and res["median_depth"] < 0, (c["n"], c["seed"])
        for c, (res, _, _) in zip(ic.family_cases("few"), ic.family_ref("few", mode)):
            assert res["verdict"] == (im.RESET_TRACKED if c["n"] == 89 else im.OK), (c["n"], c["seed"])
        for c, (res, pts, dg) in zip(ic.family_cases("z_zero"), ic.family_ref("z_zero", mode)):
            if c["seed"] % 2:
                assert np.isnan(res["chi2_first"]) and res["stop"] == im.STOP_ITERATIONS and dg["rejected_trials"] == res["trials"] == 20, (c["n"], c["seed"])
            else:
                assert res["verdict"] == im.RESET_NONFINITE and np.isnan(res["median_depth"]), (c["n"], c["seed"])
                assert np.array_equal(pts["pos"], pts["pos_scaled"]) and np.array_equal(res["Tcw2"], res["Tcw2_scaled"])
        for c, (res, pts, _) in zip(ic.family_cases("iterations_0"), ic.family_ref("iterations_0", mode)):
            assert res["iterations"] == 0 and res["trials"] == 0 and res["lambda_"] == 0
            m = pts["matched"] == 1
            assert np.array_equal(pts["pos"][m], c["P3D"][m]) and int(m.sum()) == c["n"]
        for c, (res, pts, _) in zip(ic.family_cases("no_points"), ic.family_ref("no_points", mode)):
            assert res["n_points"] == 0 and res["verdict"] == im.RESET_TRACKED and res["median_depth"] == 0 and not pts.tobytes().strip(b"\0")
        assert any(res["verdict"] == im.OK for res, _, _ in ic.family_ref("noisy", mode))
        gross = ic.family_ref("gross_20", mode)
        assert all(res["chi2_last"] < res["chi2_first"] for (res, _, _), c in zip(gross, ic.family_cases("gross_20")) if c["n"] >= 63)


# ------------------------------------------------------------------ the independent minimiser
def _exp_se3(d):
    om, up = d[:3], d[3:]
    th = np.linalg.norm(om)
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Om, up
    dR = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * (Om @ Om)
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Om + (th - np.sin(th)) / th ** 3 * (Om @ Om)
    return dR, V @ up


def _gauss_newton(case, T1, T2, X, sig):
    """a dense Gauss-Newton on the FULL system in numpy float64: the second pose (6) and every point (3 each), no Schur step, no
    kernel, the first pose held; the scale direction, which nothing constrains, is left to the minimum-norm solution of the
    normal equations.  From (T2, X) to convergence; returns (T2, X)."""
    fx, fy, cx, cy = [float(v) for v in case["K"]]
    feat1 = np.nonzero(case["matches12"] >= 0)[0]
    n = feat1.size
    kp = [case["keys_un1"][feat1], case["keys_un2"][case["matches12"][feat1]]]
    obs = [np.stack([k["x"], k["y"]], axis=1).astype(np.float64) for k in kp]
    w = [sig[k["octave"]].astype(np.float64) for k in kp]
    R = [T1[:3, :3].copy(), T2[:3, :3].copy()]
    t = [T1[:3, 3].copy(), T2[:3, 3].copy()]
    X = X.copy()
    for _ in range(12):
        J = np.zeros((4 * n, 6 + 3 * n))
        r = np.zeros(4 * n)
        ww = np.zeros(4 * n)
        for s in range(2):
            P = X @ R[s].T + t[s]
            x, y, z = P[:, 0], P[:, 1], P[:, 2]
            r[2 * s * n:2 * (s + 1) * n] = (obs[s] - np.stack([fx * x / z + cx, fy * y / z + cy], axis=1)).reshape(-1)
            ww[2 * s * n:2 * (s + 1) * n] = np.repeat(w[s], 2)
            dp = np.zeros((n, 2, 3))
            dp[:, 0, 0], dp[:, 0, 2], dp[:, 1, 1], dp[:, 1, 2] = fx / z, -fx * x / z ** 2, fy / z, -fy * y / z ** 2
            JX = -dp @ R[s]                                           # by the point
            for k in range(n):
                J[2 * s * n + 2 * k:2 * s * n + 2 * k + 2, 6 + 3 * k:9 + 3 * k] = JX[k]
            if s == 1:
                Px = np.zeros((n, 3, 3))                              # -[P]x
                Px[:, 0, 1], Px[:, 0, 2], Px[:, 1, 0], Px[:, 1, 2], Px[:, 2, 0], Px[:, 2, 1] = z, -y, -z, x, y, -x
                J[2 * n:4 * n, 0:3] = (-dp @ Px).reshape(2 * n, 3)
                J[2 * n:4 * n, 3:6] = (-dp).reshape(2 * n, 3)
        H = J.T @ (J * ww[:, None])
        g = -J.T @ (ww * r)
        d = np.linalg.lstsq(H, g, rcond=1e-13)[0]
        dR, dt = _exp_se3(d[:6])
        R[1], t[1] = dR @ R[1], dR @ t[1] + dt
        X = X + d[6:].reshape(n, 3)
        if np.linalg.norm(d) < 1e-11 * max(1.0, np.linalg.norm(X)):
            break
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R[1], t[1]
    return out, X


def _to_unit_baseline(T1, T2, X):
    """the scale gauge fixed: the world scaled about the first camera's centre so that the baseline is 1"""
    C1, C2 = -T1[:3, :3].T @ T1[:3, 3], -T2[:3, :3].T @ T2[:3, 3]
    s = 1.0 / np.linalg.norm(C2 - C1)
    C2n = C1 + s * (C2 - C1)
    T = T2.copy()
    T[:3, 3] = -T2[:3, :3] @ C2n
    return T, C1 + s * (X - C1)


# measured per family (rotation entries, translation in baselines, positions in scene depths); each asserted at 10x its own
GN_MEASURED = {"clean": (1.9e-8, 5.2e-7, 5.6e-7), "first_fixed": (1.2e-6, 1.2e-6, 3.1e-5), "mixed_octaves": (1.1e-5, 4.2e-5, 2.2e-4)}


@pytest.mark.parametrize("family", ["clean", "first_fixed", "mixed_octaves"])
def test_serial_against_a_dense_gauss_newton(family):
    """a sane minimiser: Serial with bRobust off against a dense Gauss-Newton on the full system (numpy float64, written here, no
    Schur step, no kernel) started from Serial's own result, at 130 and 600 points.  The first pose is fixed in both, so the
    gauge left is the scale: both are brought to a unit baseline about the first camera's centre.  What separates them is that
    Levenberg stops at three flat iterations (a gain under a thousandth each) and the float32 of its outputs.  Measured (seeds
    1 .. 3 at 130 points, seed 1 at 600) per family in GN_MEASURED; each family is asserted at 10x its own figures."""
    worst = [0.0, 0.0, 0.0]
    for n, seeds in ((130, (1, 2, 3)), (600, (1,))):
        for seed in seeds:
            c = dict(ic.make_case(family, n, seed))
            c["robust"] = False
            res, pts, _ = ic.ref_run(c, ic.SERIAL)
            assert res["iterations"] >= 3 and res["n_points"] == n
            m = pts["matched"] == 1
            T1, T2 = np.eye(4), np.eye(4)
            T1[:3], T2[:3] = res["Tcw1"].reshape(3, 4), res["Tcw2"].reshape(3, 4)
            X = pts["pos"][m].astype(np.float64)
            Tg, Xg = _gauss_newton(c, T1, T2, X, ic.inv_level_sigma2(family))
            Ta, Xa = _to_unit_baseline(T1, T2, X)
            Tb, Xb = _to_unit_baseline(T1, Tg, Xg)
            depth = np.median(np.linalg.norm(Xb - (-T1[:3, :3].T @ T1[:3, 3]), axis=1))
            worst = [max(worst[0], float(np.abs(Ta[:3, :3] - Tb[:3, :3]).max())), max(worst[1], float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))),
                     max(worst[2], float(np.abs(Xa - Xb).max() / depth))]
    print("%s: Serial against the Gauss-Newton: rotation %.3g, translation %.3g baselines, positions %.3g of the depth" % (family, *worst))
    assert all(w <= 10 * m for w, m in zip(worst, GN_MEASURED[family])), (worst, GN_MEASURED[family])
