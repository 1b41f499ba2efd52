"""PoseOptimization on the host, no GPU: the ABI of include/orbslamm_poseopt.h, the drop-in header against the mock, the
refusals that need no GPU, and the restatement (tools/poseopt_ref.hpp) against itself and against numpy: its Defined mode
against its Serial mode over the scene families of poseopt_cases.py, its sin / cos routine against glibc, its Serial pose
against a Gauss-Newton written here, and the stale-error trap kept exercised.

Figures measured on x86-64 / glibc (recorded in DESIGN.md §8o) and asserted here:
  Defined against Serial, pose: at most 1.4e-8 rad / 3.0e-8 over seeds 1 .. 40 of the five compared families (2 000 frames; one
    float32 step of the returned Tcw in 18 of them, nothing in the rest); asserted at 10x on seeds 1 .. 10.
  sin / cos against glibc: at most 1 ulp of glibc's value, for both, over 10^7 arguments in [1e-5, 2 pi] and 10^5 in [2 pi, 1e3].
  Serial against the Gauss-Newton on the ground-truth inliers: see GN_ROT_MEASURED / GN_TRANS_MEASURED below."""
import os

import numpy as np
import pytest

import dropin
import poseopt_cases as pc
import ref_shim
from orbslamm_amd import optimizer as opt
from orbslamm_amd._lib import KP_DTYPE, ORBX_E_INVALID, ORBX_E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARED = [f for f in pc.FAMILIES if f not in pc.INTEGER_ONLY]

# measured maxima (this file's docstring); the assertions are at 10x
DS_ROT_MEASURED, DS_TRANS_MEASURED = 1.4e-8, 3.0e-8    # radians, scene units: seeds 1 .. 40 of the five compared families
SINCOS_ULP_MEASURED = 1.0
GN_ROT_MEASURED, GN_TRANS_MEASURED = 1.8e-8, 4.5e-8     # radians, scene units (metres): test_serial_against_a_gauss_newton...


def test_header_declares_and_library_exports_the_poseopt_block():
    from orbslamm_amd import _lib
    src = open(os.path.join(ROOT, "include", "orbslamm_poseopt.h")).read()
    assert "ORBO_MAX_FRAMES %d" % opt.MAX_FRAMES in src and "ORBO_MAX_EDGES %d" % opt.MAX_EDGES in src
    assert "ORBO_MAX_CALL_EDGES (1 << 22)" in src and opt.MAX_CALL_EDGES == 1 << 22
    assert opt.MAX_FRAMES >= 4096 and opt.MAX_EDGES >= 65535
    declared = ref_shim.declared("orbslamm_poseopt.h", "orbo_")
    assert len(declared) == 2
    assert declared == ref_shim.declared("orbslamm_poseopt.h")
    assert '#include "orbslamm_poseopt.h"' in open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    import orbslamm_amd
    assert orbslamm_amd.pose_optimization is opt.pose_optimization and orbslamm_amd.pose_optimization_batch is opt.pose_optimization_batch
    assert opt.RESULT_DTYPE.itemsize == pc.REF_RESULT.itemsize == 176
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "poseopt_ref.hpp"))
    for name in ("orbg_kernels.hip", "orbo_kernels.hip", "orbo_host.inc"):
        assert "poseopt_ref" not in open(os.path.join(ROOT, "orbslamm_amd", "csrc", name)).read()


def test_dropin_header_compiles_against_the_mock():
    """include/Optimizer_hip.hpp instantiated on tests/cpp/mock_poseopt.hpp (the GPU test runs it)"""
    dropin.syntax_only("poseopt_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "Optimizer_hip.hpp")).read()
    for member in ("PoseOptimizationT", "Run(", "RunAll(", "stereo"):
        assert member in hdr, member


def test_refusals_that_need_no_gpu():
    """the argument checks come before the handle's: with a NULL handle every refusal still names its own reason"""
    import ctypes as C
    from orbslamm_amd import _lib
    L = _lib.lib()
    sig = pc.inv_level_sigma2()
    keys = np.zeros(5, dtype=KP_DTYPE)
    keys["octave"] = [0, 1, 2, 7, 8]

    def call(frames=1, feats=(0, 1, 2), start=None, keys_=keys, sig_=sig, nlevels=None, edges="default", resident=None, frames_arr="default"):
        fr = np.zeros(frames, dtype=opt.FRAME_DTYPE) if frames_arr == "default" else frames_arr
        ed = opt.pack_edges(feats, np.ones((len(feats), 3))) if edges == "default" else edges
        st = [0] + [len(feats)] * frames if start is None else start
        rc, _, _ = opt.pose_optimize_raw(None, fr, None if resident is not None else [keys_] * max(frames, 0), resident, st, ed, sig_, nlevels)
        return rc, L.orbx_last_error().decode()

    rc, msg = call()
    assert rc == ORBX_E_INVALID and "null handle" in msg               # everything else is in order: the handle is what is missing
    rc, msg = call(feats=(0, 1, 5))
    assert rc == ORBX_E_INVALID and "feature 5" in msg
    rc, msg = call(feats=(0, -1, 2))
    assert rc == ORBX_E_INVALID and "feature -1" in msg
    rc, msg = call(feats=(0, 1, 4))
    assert rc == ORBX_E_INVALID and "octave 8" in msg                  # octave 8 of 8 levels
    rc, msg = call(feats=(0, 1, 3), nlevels=7)
    assert rc == ORBX_E_INVALID and "octave 7" in msg
    for nl in (0, 17, -3):
        rc, msg = call(sig_=np.ones(17, np.float32), nlevels=nl)
        assert rc == ORBX_E_INVALID and "nlevels" in msg
    assert call(sig_=None, nlevels=8)[0] == ORBX_E_INVALID
    rc, msg = call(frames=2, start=[0, 3, 2])
    assert rc == ORBX_E_INVALID and "descends" in msg
    rc, msg = call(start=[1, 3])
    assert rc == ORBX_E_INVALID and "starts at 0" in msg
    st1 = np.array([0, 0], np.int32)
    assert L.orbo_pose_optimize(None, None, None, None, 1, st1.ctypes.data, None, sig.ctypes.data, 8, np.zeros(1, opt.RESULT_DTYPE).ctypes.data,
                                None) == ORBX_E_INVALID                # null frames with a frame count
    assert L.orbo_pose_optimize(None, np.zeros(1, opt.FRAME_DTYPE).ctypes.data, None, None, 1, st1.ctypes.data, None, sig.ctypes.data, 8, None,
                                None) == ORBX_E_INVALID                # null results with a frame count
    assert call(edges=None)[0] == ORBX_E_INVALID                       # null edges with an edge count
    # the key arrays: a negative n_keys, a null array with keys, null keys_un / n_keys with frames
    fr1, ed3, st3 = np.zeros(1, opt.FRAME_DTYPE), opt.pack_edges((0, 1, 2), np.ones((3, 3))), np.array([0, 3], np.int32)
    out1, fl3 = np.zeros(1, opt.RESULT_DTYPE), np.zeros(3, np.uint8)
    kptr = (C.c_void_p * 1)(keys.ctypes.data)

    def keys_call(kp, nk):
        nk = None if nk is None else np.array(nk, np.int32)
        rc = L.orbo_pose_optimize(None, fr1.ctypes.data, kp, None if nk is None else nk.ctypes.data, 1, st3.ctypes.data, ed3.ctypes.data,
                                  sig.ctypes.data, 8, out1.ctypes.data, fl3.ctypes.data)
        return rc, L.orbx_last_error().decode()
    assert keys_call(kptr, [5]) == (ORBX_E_INVALID, "null handle")     # (in order)
    rc, msg = keys_call(kptr, [-1])
    assert rc == ORBX_E_INVALID and "key array" in msg
    rc, msg = keys_call((C.c_void_p * 1)(None), [5])
    assert rc == ORBX_E_INVALID and "key array" in msg
    assert keys_call(None, [5])[0] == ORBX_E_INVALID and "null key arrays" in keys_call(None, [5])[1]
    assert keys_call(kptr, None)[0] == ORBX_E_INVALID and "null key arrays" in keys_call(kptr, None)[1]
    # zero frames: ORBX_OK at once, whatever else is passed (the handle included)
    assert L.orbo_pose_optimize(None, None, None, None, 0, None, None, None, 0, None, None) == 0
    assert L.orbo_pose_optimize_frames(None, None, None, 0, None, None, None, 0, None, None) == 0
    rc, _, _ = opt.pose_optimize_raw(None, np.zeros(1, opt.FRAME_DTYPE), None, None, None, None, sig)
    assert rc == ORBX_E_INVALID                                        # null edge_start
    assert L.orbo_pose_optimize(None, None, None, None, -1, None, None, None, 8, None, None) == ORBX_E_INVALID
    assert "negative" in L.orbx_last_error().decode()
    # the ceilings
    st = np.zeros(opt.MAX_FRAMES + 2, dtype=np.int32)
    rc, msg = call(frames=opt.MAX_FRAMES + 1, feats=(), start=st)
    assert rc == ORBX_E_UNSUPPORTED and "frames" in msg
    big = opt.MAX_EDGES + 1
    rc, _, _ = opt.pose_optimize_raw(None, np.zeros(1, opt.FRAME_DTYPE), [keys], None, [0, big], np.zeros(big, opt.EDGE_DTYPE), sig)
    assert rc == ORBX_E_UNSUPPORTED and "edges" in L.orbx_last_error().decode()
    # more than MAX_CALL_EDGES edges in one call, no frame above MAX_EDGES
    nfr = opt.MAX_CALL_EDGES // opt.MAX_EDGES + 1
    st = (np.arange(nfr + 1, dtype=np.int64) * opt.MAX_EDGES).astype(np.int32)
    rc = L.orbo_pose_optimize(None, np.zeros(nfr, opt.FRAME_DTYPE).ctypes.data, None, None, nfr, st.ctypes.data, None, sig.ctypes.data, 8,
                              np.zeros(nfr, opt.RESULT_DTYPE).ctypes.data, None)
    assert rc == ORBX_E_UNSUPPORTED and "in one call" in L.orbx_last_error().decode()
    # the resident entry: the same checks, then a null frame
    rc, msg = call(resident=[C.c_void_p(0)])
    assert rc == ORBX_E_INVALID and "frame" in msg
    rc, msg = call(resident=[C.c_void_p(0)], start=[0, 3, 2], frames=2)
    assert rc == ORBX_E_INVALID and "descends" in msg


def test_defined_against_serial_preconditions():
    """In Serial, at none of the four classifications does any edge's chi2 lie within a relative 1e-6 of 5.991: where it did,
    Defined could classify the edge the other way for a reason that is no fault.  Asserted, not skipped, on the ten open
    seeds and on the selected ones."""
    checked = 0
    for fam in pc.FAMILIES:
        for cases, (res, _, _, chis) in ((pc.open_cases(fam), pc.open_ref(fam, pc.SERIAL)), (pc.family_cases(fam), pc.family_ref(fam, pc.SERIAL))):
            for i, c in enumerate(cases):
                ch = chis[i][:res["rounds"][i]]
                ch = ch[np.isfinite(ch)]
                assert not np.any(np.abs(ch - 5.991) <= 1e-6 * 5.991), (fam, c["n"], c["seed"])
                checked += ch.size
    assert checked > 400000


def test_defined_against_serial_on_open_seeds():
    """Seeds 1 .. 10 of every family, not chosen by the comparison: the outlier bytes, n_good and rounds are equal, and in the
    five families where the pose is compared (all_wrong and behind: integers only) it agrees to 10x the measured maximum.
    Measured over seeds 1 .. 40 (2 000 frames): rotation 1.4e-8 rad, translation 3.0e-8, one float32 step of the returned
    Tcw in 18 frames and nothing in the others.  `iterations` is NOT asserted here: see poseopt_cases.SEEDS."""
    worst = [0.0, 0.0]
    for fam in pc.FAMILIES:
        rs, fs, _, _ = pc.open_ref(fam, pc.SERIAL)
        rd, fd, _, _ = pc.open_ref(fam, pc.DEFINED)
        for i, c in enumerate(pc.open_cases(fam)):
            tag = (fam, c["n"], c["seed"])
            assert np.array_equal(fs[i], fd[i]), tag
            assert rs["n_good"][i] == rd["n_good"][i] and rs["rounds"][i] == rd["rounds"][i] and rs["n_initial"][i] == rd["n_initial"][i] == c["n"], tag
            assert rs["rounds"][i] == (0 if c["n"] < 3 else 1 if c["n"] < 10 else 4), tag
            if fam in COMPARED:
                a, t = pc.pose_distance(rs["Tcw"][i].reshape(4, 4), rd["Tcw"][i].reshape(4, 4))
                worst = [max(worst[0], a), max(worst[1], t)]
    print("Defined against Serial, open seeds: rotation %.3g rad, translation %.3g" % tuple(worst))
    assert worst[0] <= 10 * DS_ROT_MEASURED and worst[1] <= 10 * DS_TRANS_MEASURED


def test_defined_against_serial_iterations_on_the_selected_seeds():
    """`iterations` (with the other integer outputs) on poseopt_cases.SEEDS, the seeds chosen so that the two modes' converged
    rounds end alike: rounding noise decides a converged round's last solver calls, so this equality holds by the choice of
    the seeds and says only that nothing but that noise separates the modes' control flow"""
    for fam in pc.FAMILIES:
        rs, fs, _, _ = pc.family_ref(fam, pc.SERIAL)
        rd, fd, _, _ = pc.family_ref(fam, pc.DEFINED)
        for i, c in enumerate(pc.family_cases(fam)):
            tag = (fam, c["n"], c["seed"])
            assert np.array_equal(fs[i], fd[i]) and rs["n_good"][i] == rd["n_good"][i] and rs["rounds"][i] == rd["rounds"][i], tag
            assert np.array_equal(rs["iterations"][i], rd["iterations"][i]), tag


def test_fewer_than_three_edges_and_fewer_than_ten():
    for mode in (pc.SERIAL, pc.DEFINED):
        res, flags, _, _ = pc.family_ref("clean", mode)
        for i, c in enumerate(pc.family_cases("clean")):
            if c["n"] < 3:
                assert res["n_good"][i] == 0 and res["rounds"][i] == 0 and res["Tcw"][i].tobytes() == c["Tcw"].tobytes() and not flags[i].any()
            elif c["n"] < 10:
                assert res["rounds"][i] == 1 and res["iterations"][i][0] > 0 and not res["iterations"][i][1:].any()


def test_sincos_routine_against_glibc():
    """the Defined sin / cos against libm's: 10^7 arguments dense in [1e-5, 2 pi] and 10^5 in [2 pi, 1e3]; the largest error in
    units of the last place of libm's value is measured (1.0 for both functions, both ranges) and asserted"""
    L = pc.ref_lib()
    worst = 0.0
    for lo, hi, count in ((1e-5, 2 * np.pi, 10_000_000), (2 * np.pi, 1e3, 100_000)):
        m, at = np.zeros(2), np.zeros(2)
        L.poseoptref_sincos_sweep(lo, hi, count, m.ctypes.data, at.ctypes.data)
        print("sin/cos against glibc on [%g, %g]: %.3f / %.3f ulp at %r / %r" % (lo, hi, m[0], m[1], at[0], at[1]))
        worst = max(worst, m[0], m[1])
    assert worst <= np.ceil(SINCOS_ULP_MEASURED)
    # defined for every finite argument, odd / even, NaN for what is not finite
    x = np.array([0.0, -0.0, 5e-324, 1e-300, 0.5, -0.5, 1e6, 1048576.0, 1e7, 1e18, 1e300, -1e300, 1.7976931348623157e308, np.inf, -np.inf, np.nan])
    s, c = np.zeros_like(x), np.zeros_like(x)
    L.poseoptref_sincos(x.ctypes.data, x.size, s.ctypes.data, c.ctypes.data)
    fin = np.isfinite(x)
    assert np.all(np.isfinite(s[fin])) and np.all(np.isfinite(c[fin])) and np.all(np.abs(s[fin]) <= 1.0 + 1e-15) and np.all(np.abs(c[fin]) <= 1.0 + 1e-15)
    assert np.all(np.isnan(s[~fin])) and np.all(np.isnan(c[~fin]))
    assert s[0] == 0 and c[0] == 1 and s[4] == -s[5] and c[4] == c[5] and s[10] == -s[11] and c[10] == c[11]
    assert abs(s[6] - np.sin(1e6)) < 1e-10 and abs(c[6] - np.cos(1e6)) < 1e-10


def _gauss_newton(case, use, sig):
    """a Gauss-Newton in numpy float64 on the edges `use`, no robust kernel, from the true pose to convergence"""
    fx, fy, cx, cy = [float(v) for v in case["K"]]
    T = case["truth"].astype(np.float64)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    u, s = np.linalg.svd(R)[0], np.linalg.svd(R)[2]
    R = u @ s                                                   # (the float32 entries made orthonormal)
    kp = case["keys_un"][case["feature"]][use]
    obs = np.stack([kp["x"], kp["y"]], axis=1).astype(np.float64)
    w = sig[kp["octave"]].astype(np.float64)
    X = case["Xw"][use].astype(np.float64)
    for _ in range(100):
        P = X @ R.T + t
        x, y, iz = P[:, 0], P[:, 1], 1.0 / P[:, 2]
        r = obs - np.stack([fx * x * iz + cx, fy * y * iz + cy], axis=1)
        z0 = np.zeros_like(x)
        J = np.stack([np.stack([x * y * iz * iz * fx, -(1 + x * x * iz * iz) * fx, y * iz * fx, -iz * fx, z0, x * iz * iz * fx], axis=1),
                      np.stack([(1 + y * y * iz * iz) * fy, -x * y * iz * iz * fy, -x * iz * fy, z0, -iz * fy, y * iz * iz * fy], axis=1)], axis=1)
        Hm = np.einsum("nki,n,nkj->ij", J, w, J)
        g = -np.einsum("nki,n,nk->i", J, w, r)
        d = np.linalg.solve(Hm, g)
        om, up = d[:3], d[3:]
        th = np.linalg.norm(om)
        Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
        if th < 1e-12:
            dR, V = np.eye(3) + Om, np.eye(3)
        else:
            dR = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * (Om @ Om)
            V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Om + (th - np.sin(th)) / th ** 3 * (Om @ Om)
        R, t = dR @ R, dR @ t + V @ up
        if np.linalg.norm(d) < 1e-13:
            break
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, t
    return out


@pytest.mark.parametrize("family", ["clean", "gross_30", "mixed_octaves"])
def test_serial_against_a_gauss_newton_on_the_true_inliers(family):
    """a sane minimiser: the Serial pose against a Gauss-Newton (numpy float64, written here) on the ground-truth inlier set
    without a kernel, at 63 edges and more; and the inlier set it returns is the ground truth's except for edges whose true
    displacement is under 4 px.  Measured over the three families: rotation <= 1.8e-8 rad, translation <= 4.5e-8 (clean
    1.77e-8 / 3.74e-8, gross_30 1.16e-8 / 3.28e-8, mixed_octaves 1.17e-8 / 4.45e-8: the size of the float32 rounding of the
    pose the optimiser returns -- its last round runs without a kernel on exactly the true inliers); asserted at 10x."""
    sig = pc.inv_level_sigma2()
    res, flags, _, _ = pc.family_ref(family, pc.SERIAL)
    worst = [0.0, 0.0]
    for i, c in enumerate(pc.family_cases(family)):
        if c["n"] < 63:
            continue
        truth = c["truth"].astype(np.float64)
        P = c["Xw"].astype(np.float64) @ truth[:3, :3].T + truth[:3, 3]
        kp = c["keys_un"][c["feature"]]
        proj = np.stack([c["K"][0] * P[:, 0] / P[:, 2] + c["K"][2], c["K"][1] * P[:, 1] / P[:, 2] + c["K"][3]], axis=1)
        true_disp = np.linalg.norm(np.stack([kp["x"], kp["y"]], axis=1) - proj, axis=1)
        differ = flags[i].astype(bool) != c["displaced"]
        assert np.all(true_disp[differ] < 4.0), (family, c["n"], c["seed"], true_disp[differ].max())
        assert res["n_good"][i] == c["n"] - flags[i].sum()
        gn = _gauss_newton(c, ~c["displaced"], sig)
        a, t = pc.pose_distance(res["Tcw"][i].reshape(4, 4), gn)
        worst = [max(worst[0], a), max(worst[1], t)]
    print("%s: Serial against the Gauss-Newton: rotation %.3g rad, translation %.3g" % (family, worst[0], worst[1]))
    assert worst[0] <= 10 * GN_ROT_MEASURED and worst[1] <= 10 * GN_TRANS_MEASURED


def test_the_stale_error_trap_is_exercised():
    """over the family seeds the restatement's diagnostic shows rounds whose LAST Levenberg trial was rejected: their level-0
    edges are classified with the error of the rejected pose, the trap the device has to reproduce"""
    total = 0
    for fam in pc.FAMILIES:
        for mode in (pc.SERIAL, pc.DEFINED):
            total += int(pc.family_ref(fam, mode)[2].sum())
    assert total >= 1
    assert int(pc.family_ref("far_start", pc.DEFINED)[2].sum()) >= 1
