"""OptimizeSim3 on the host, no GPU: the ABI of include/orbslamm_sim3opt.h, the drop-in header against the mocks, the refusals
that need no GPU, and the restatement (tools/sim3opt_ref.hpp) against itself and against numpy: its Defined mode against its
Serial mode over the scene families of sim3opt_cases.py, its cached-perturbation evaluation (the device's) against the per-edge
push / oplus / pop, its exp routine against glibc, its Serial Sim3 against a Gauss-Newton written here, the stale-error trap
and the early return kept exercised.

Figures measured on x86-64 / glibc (recorded in DESIGN.md §8p) and asserted here:
  Defined against Serial, Sim3: 1.5e-8 rad / 1.3e-7 / 9.6e-7 in scale (DS_*_MEASURED below), over seeds 1 .. 40 of the five compared families x both fix_scale x
    OPEN_COUNTS (2 800 problems); asserted at 10x on seeds 1 .. 10.
  exp against glibc: at most 1 ulp of glibc's value (it does not exceed 1 ulp), over 10^7 arguments in [-1, 1] and 10^5 in [-20, 20].
  Serial against the Gauss-Newton on the ground-truth inliers: 6.9e-6 rad / 3.2e-5 / 7.1e-5 in scale (GN_*_MEASURED below)."""
import os

import numpy as np
import pytest

import dropin
import ref_shim
import sim3opt_cases as sc
from orbslamm_amd import optimizer as opt
from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARED = [f for f in sc.FAMILIES if f not in sc.INTEGER_ONLY]

# measured maxima (this file's docstring); the assertions are at 10x
DS_ROT_MEASURED, DS_TRANS_MEASURED, DS_SCALE_MEASURED = 1.5e-8, 1.3e-7, 9.6e-7    # radians, scene units, scale: seeds 1 .. 40
EXP_ULP_MEASURED = 1.0                                                           # ulp of glibc's value, both ranges
# clean 3.7e-8 / 2.6e-7 / 2.4e-7, gross_30 6.9e-6 / 3.2e-5 / 7.1e-5, scale_off 5.5e-7 / 6.8e-6 / 2.7e-5: the maximum of the three
GN_ROT_MEASURED, GN_TRANS_MEASURED, GN_SCALE_MEASURED = 6.9e-6, 3.2e-5, 7.1e-5    # radians, scene units, scale
# (seed, fix_scale) pairs on which Serial and Defined make the same number of solver calls at every count of COUNTS: the first
# three of seed 1, 2, 3, ... a family where that holds (gross_30, few_left, behind, all_wrong: nearly every seed; scale_off and
# far_start: about one seed in eight for both fix_scale at once; clean and mixed_octaves, whose second pass starts converged: no
# seed of 1 .. 40 for both fix_scale at once, so the pairs are taken one fix_scale at a time)
ITER_PAIRS = {"clean": ((51, 0), (102, 0), (103, 0)), "gross_30": ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)),
              "scale_off": ((1, 0), (1, 1), (6, 0), (6, 1), (19, 0), (19, 1)), "far_start": ((2, 0), (2, 1), (10, 0), (10, 1), (15, 0), (15, 1)),
              "mixed_octaves": ((23, 0), (24, 0), (25, 0)), "few_left": ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)),
              "behind": ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)), "all_wrong": ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1))}


def test_header_declares_and_library_exports_the_sim3opt_block():
    from orbslamm_amd import _lib
    src = open(os.path.join(ROOT, "include", "orbslamm_sim3opt.h")).read()
    assert "ORBZ_MAX_PROBLEMS %d" % opt.SIM3_MAX_PROBLEMS in src and "ORBZ_MAX_CORR %d" % opt.SIM3_MAX_CORR in src
    assert "ORBZ_MAX_CALL_CORR (1 << 21)" in src and opt.SIM3_MAX_CALL_CORR == 1 << 21
    assert opt.SIM3_MAX_PROBLEMS == 4096 and opt.SIM3_MAX_CORR == 32767
    assert ref_shim.declared("orbslamm_sim3opt.h") == ["orbz_optimize_sim3"]
    assert '#include "orbslamm_sim3opt.h"' in open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    assert hasattr(_lib.lib(), "orbz_optimize_sim3")
    import orbslamm_amd
    assert orbslamm_amd.optimize_sim3 is opt.optimize_sim3 and orbslamm_amd.optimize_sim3_batch is opt.optimize_sim3_batch
    assert orbslamm_amd.sim3_from_rts is opt.sim3_from_rts
    assert opt.SIM3_PROBLEM_DTYPE.itemsize == sc.REF_PROBLEM.itemsize == 200 and opt.SIM3_CORR_DTYPE.itemsize == 52
    assert opt.SIM3_RESULT_DTYPE.itemsize == sc.REF_RESULT.itemsize == 128
    # the restatement includes poseopt_ref.hpp alone
    ref = os.path.join(ROOT, "tools", "sim3opt_ref.hpp")
    ref_shim.assert_shares_no_code_with_the_library(ref)
    assert ref_shim.quoted_includes(ref)[1:] == [os.path.join(ROOT, "tools", "poseopt_ref.hpp")]
    for name in ("orbg_kernels.hip", "orbz_kernels.hip", "orbz_host.inc"):
        text = open(os.path.join(ROOT, "orbslamm_amd", "csrc", name)).read()
        assert "sim3opt_ref" not in text and "poseopt_ref" not in text


def test_dropin_header_compiles_against_the_mocks():
    """include/Optimizer_hip.hpp's OptimizeSim3T instantiated on tests/cpp/mock_sim3opt.hpp (the GPU test runs it)"""
    dropin.syntax_only("sim3opt_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "Optimizer_hip.hpp")).read()
    for member in ("OptimizeSim3T", "PoseOptimizationT", "struct Job", "stereo", "orbz_optimize_sim3"):
        assert member in hdr, member


def test_refusals_that_need_no_gpu():
    """the argument checks come before the handle's: with a NULL handle every refusal still names its own reason"""
    from orbslamm_amd import _lib
    L = _lib.lib()
    sig = sc.inv_level_sigma2()
    case = sc.make_case("clean", 3, 1)

    def call(problems=1, n=3, start=None, sig1=sig, sig2=sig, nlevels=None, corrs="default", th2=10.0, oct1=None, oct2=None, probs="default"):
        pr = np.concatenate([opt.pack_sim3_problem(dict(case, S12=(case["q"], case["t"], case["s"]), th2=th2))] * problems) if probs == "default" and problems > 0 else \
            (np.zeros(0, opt.SIM3_PROBLEM_DTYPE) if probs == "default" else probs)
        co = opt.pack_sim3_corrs(case)[:n] if corrs == "default" else corrs
        if oct1 is not None:
            co["oct1"][-1] = oct1
        if oct2 is not None:
            co["oct2"][-1] = oct2
        st = [0] + [n] * problems if start is None else start
        rc, _, _ = opt.optimize_sim3_raw(None, pr, st, co, sig1, sig2, nlevels)
        return rc, L.orbx_last_error().decode()

    rc, msg = call()
    assert rc == ORBX_E_INVALID and "null handle" in msg               # everything else is in order: the handle is what is missing
    rc, msg = call(oct1=8)
    assert rc == ORBX_E_INVALID and "octave 8 of keyframe 1" in msg
    rc, msg = call(oct2=-1)
    assert rc == ORBX_E_INVALID and "octave -1 of keyframe 2" in msg
    rc, msg = call(oct2=7, nlevels=7)
    assert rc == ORBX_E_INVALID and "octave 7 of keyframe 2" in msg
    for nl in (0, 17, -3):
        rc, msg = call(sig1=np.ones(17, np.float32), sig2=np.ones(17, np.float32), nlevels=nl)
        assert rc == ORBX_E_INVALID and "nlevels" in msg
    assert call(sig1=None, nlevels=8)[0] == ORBX_E_INVALID and call(sig2=None, nlevels=8)[0] == ORBX_E_INVALID
    rc, msg = call(problems=2, start=[0, 3, 2])
    assert rc == ORBX_E_INVALID and "descends" in msg
    rc, msg = call(start=[1, 3])
    assert rc == ORBX_E_INVALID and "starts at 0" in msg
    for bad in (0.0, -1.0, np.inf, np.nan):
        rc, msg = call(th2=bad)
        assert rc == ORBX_E_INVALID and "th2" in msg, bad
    st1 = np.array([0, 0], np.int32)
    out1 = np.zeros(1, opt.SIM3_RESULT_DTYPE)
    pr1 = np.zeros(1, opt.SIM3_PROBLEM_DTYPE)
    assert L.orbz_optimize_sim3(None, None, 1, st1.ctypes.data, None, sig.ctypes.data, sig.ctypes.data, 8, out1.ctypes.data, None) == ORBX_E_INVALID
    assert L.orbz_optimize_sim3(None, pr1.ctypes.data, 1, st1.ctypes.data, None, sig.ctypes.data, sig.ctypes.data, 8, None, None) == ORBX_E_INVALID
    assert call(corrs=None)[0] == ORBX_E_INVALID                       # null correspondences with a count
    assert L.orbz_optimize_sim3(None, pr1.ctypes.data, 1, None, None, sig.ctypes.data, sig.ctypes.data, 8, out1.ctypes.data, None) == ORBX_E_INVALID
    assert "corr_start" in L.orbx_last_error().decode()
    # zero problems: ORBX_OK at once, whatever else is passed (the handle included)
    assert L.orbz_optimize_sim3(None, None, 0, None, None, None, None, 0, None, None) == 0
    assert L.orbz_optimize_sim3(None, None, -1, None, None, None, None, 8, None, None) == ORBX_E_INVALID
    assert "negative" in L.orbx_last_error().decode()
    # the ceilings
    st = np.zeros(opt.SIM3_MAX_PROBLEMS + 2, dtype=np.int32)
    rc, msg = call(problems=opt.SIM3_MAX_PROBLEMS + 1, n=0, start=st)
    assert rc == ORBX_E_UNSUPPORTED and "problems" in msg
    big = opt.SIM3_MAX_CORR + 1
    rc, _, _ = opt.optimize_sim3_raw(None, pr1, [0, big], np.zeros(big, opt.SIM3_CORR_DTYPE), sig, sig)
    assert rc == ORBX_E_UNSUPPORTED and "correspondences in problem 0" in L.orbx_last_error().decode()
    npb = opt.SIM3_MAX_CALL_CORR // opt.SIM3_MAX_CORR + 1
    st = (np.arange(npb + 1, dtype=np.int64) * opt.SIM3_MAX_CORR).astype(np.int32)
    rc = L.orbz_optimize_sim3(None, np.zeros(npb, opt.SIM3_PROBLEM_DTYPE).ctypes.data, npb, st.ctypes.data, None, sig.ctypes.data, sig.ctypes.data, 8,
                              np.zeros(npb, opt.SIM3_RESULT_DTYPE).ctypes.data, None)
    assert rc == ORBX_E_UNSUPPORTED and "in one call" in L.orbx_last_error().decode()


def test_the_huber_width_reading_is_immaterial_at_th2_10():
    """deltaHuber = sqrt(th2) (ref:1398) is taken as the float square root of the float; for th2 = 10, the value both call sites
    pass, that equals the double square root narrowed"""
    th2 = np.float32(10.0)
    assert np.sqrt(th2).dtype == np.float32 and np.sqrt(th2) == np.float32(np.sqrt(np.float64(th2)))


def test_sim3_from_rts_is_eigens_quaternion_by_bits():
    rng = np.random.default_rng(3)
    mats = [sc.rot_axis_angle(rng.normal(size=3), a) for a in (0.0, 1e-9, 0.3, 1.5, 2.8, np.pi - 1e-3, np.pi)]
    for ax in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.2]):                         # each branch of the largest diagonal entry
        mats.append(sc.rot_axis_angle(ax, 3.0))
    mats.append(np.eye(3) + rng.normal(size=(3, 3)) * 0.01)                            # not a rotation: taken as it is
    for R in mats:
        q, t, s = opt.sim3_from_rts(R, [1, 2, 3], 1.5)
        assert q.tobytes() == sc.quat_of(R).tobytes() and t.tolist() == [1.0, 2.0, 3.0] and s == 1.5


def test_exp_routine_against_glibc():
    """definedExp against libm's: 10^7 arguments dense in [-1, 1] and 10^5 in [-20, 20]; the largest error in units of the last
    place of libm's value is measured and asserted at that value"""
    L = sc.ref_lib()
    worst = 0.0
    for lo, hi, count in ((-1.0, 1.0, 10_000_000), (-20.0, 20.0, 100_000)):
        m, at = np.zeros(1), np.zeros(1)
        L.sim3optref_exp_sweep(lo, hi, count, m.ctypes.data, at.ctypes.data)
        print("exp against glibc on [%g, %g]: %.3f ulp at %r" % (lo, hi, m[0], at[0]))
        worst = max(worst, m[0])
    assert worst <= EXP_ULP_MEASURED
    # defined for every input: NaN -> NaN, overflow -> inf, underflow -> 0, exact at 0
    x = np.array([0.0, -0.0, 5e-324, 1e-300, 1.0, -1.0, 709.0, 709.9, 1e300, np.inf, -708.0, -740.0, -746.0, -1e300, -np.inf, np.nan])
    e = np.zeros_like(x)
    L.sim3optref_exp(x.ctypes.data, x.size, e.ctypes.data)
    assert e[0] == 1.0 and e[1] == 1.0 and e[2] == 1.0 and e[3] == 1.0
    assert abs(e[4] - np.e) <= 4.5e-16 and abs(e[5] - 1 / np.e) <= 1.2e-16 and np.isfinite(e[6]) and abs(e[6] / np.exp(709.0) - 1) < 1e-15
    assert np.all(np.isinf(e[7:10])) and np.all(e[7:10] > 0)
    assert abs(e[10] / np.exp(-708.0) - 1) < 1e-15 and 0 < e[11] < 1e-320 and np.all(e[12:15] == 0.0) and np.isnan(e[15])


def test_defined_against_serial_preconditions():
    """In Serial, at neither check does any edge's chi2 lie within a relative 1e-6 of th2: where it did, Defined could decide the
    pair the other way for a reason that is no fault.  Asserted, not skipped, on the ten open seeds."""
    checked = 0
    for fam in sc.FAMILIES:
        res, _, _, chis = sc.open_ref(fam, sc.SERIAL)
        for i, c in enumerate(sc.open_cases(fam)):
            ch = chis[i][:1 + int(res["written"][i])]
            ch = ch[np.isfinite(ch)]
            assert not np.any(np.abs(ch - sc.TH2) <= 1e-6 * sc.TH2), (fam, c["n"], c["seed"], c["fix_scale"])
            checked += ch.size
    assert checked > 50000


def test_defined_against_serial_on_open_seeds():
    """Seeds 1 .. 10 of every family, not chosen by the comparison: the removed bytes, n_bad, n_in and written are equal, and in
    the five families where the Sim3 is compared it agrees to 10x the maximum measured over seeds 1 .. 40.  `iterations` is NOT
    asserted here."""
    worst = [0.0, 0.0, 0.0]
    for fam in sc.FAMILIES:
        rs, fs, _, _ = sc.open_ref(fam, sc.SERIAL)
        rd, fd, _, _ = sc.open_ref(fam, sc.DEFINED)
        for i, c in enumerate(sc.open_cases(fam)):
            tag = (fam, c["n"], c["seed"], c["fix_scale"])
            assert np.array_equal(fs[i], fd[i]), tag
            for k in ("n_bad", "n_in", "written", "n_corr"):
                assert rs[k][i] == rd[k][i], (tag, k)
            assert rs["n_corr"][i] == c["n"] and (rs["written"][i] == 0 or c["n"] >= 10), tag
            if fam in COMPARED:
                d = sc.sim3_distance((rs["q"][i], rs["t"][i], rs["s"][i]), (rd["q"][i], rd["t"][i], rd["s"][i]))
                worst = [max(a, b) for a, b in zip(worst, d)]
    print("Defined against Serial, open seeds: rotation %.3g rad, translation %.3g, scale %.3g" % tuple(worst))
    assert worst[0] <= 10 * DS_ROT_MEASURED and worst[1] <= 10 * DS_TRANS_MEASURED and worst[2] <= 10 * DS_SCALE_MEASURED


def test_defined_against_serial_iterations_on_the_selected_seeds():
    """`iterations` on ITER_PAIRS, the seeds chosen so that the two modes' converged passes end alike: rounding noise decides a
    converged pass's last solver calls (DESIGN.md §8o's caveat), so this equality holds by the choice of the seeds and says only
    that nothing but that noise separates the modes' control flow"""
    assert set(ITER_PAIRS) == set(sc.FAMILIES)
    for fam, pairs in ITER_PAIRS.items():
        assert len(pairs) >= 3
        cases = [sc.make_case(fam, n, s, fs) for s, fs in pairs for n in sc.COUNTS]
        rs, fs_, _, _ = sc.ref_run(sc.SERIAL, cases)
        rd, fd, _, _ = sc.ref_run(sc.DEFINED, cases)
        for i, c in enumerate(cases):
            tag = (fam, c["n"], c["seed"], c["fix_scale"])
            assert np.array_equal(fs_[i], fd[i]) and rs["n_in"][i] == rd["n_in"][i] and rs["written"][i] == rd["written"][i], tag
            assert np.array_equal(rs["iterations"][i], rd["iterations"][i]), tag


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_cached_perturbations_equal_the_per_edge_push_oplus_pop(family):
    """the 14 perturbed estimates taken once per linearisation (what the device does) against g2o's per-edge push / oplus /
    computeError / pop, both in Defined: equal by bits, every field and every removed byte"""
    cases = list(sc.family_cases(family))
    per_edge, pf, _, _ = sc.family_ref(family, sc.DEFINED)
    cached, cf, _, _ = sc.ref_run(sc.DEFINED_CACHED, cases)
    assert per_edge.tobytes() == cached.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pf, cf))
    assert any(r["iterations"][0] > 0 for r in per_edge)


def _sim3_apply(R, t, s, P):
    return s * (P @ R.T) + t


def _gn_residual(c, use, sig, R, t, s):
    R1, t1 = c["R1w"].reshape(3, 3).astype(np.float64), c["t1w"].astype(np.float64)
    R2, t2 = c["R2w"].reshape(3, 3).astype(np.float64), c["t2w"].astype(np.float64)
    P1 = c["X1w"][use].astype(np.float64) @ R1.T + t1
    P2 = c["X2w"][use].astype(np.float64) @ R2.T + t2
    K1, K2 = c["K1"].astype(np.float64), c["K2"].astype(np.float64)
    a = _sim3_apply(R, t, s, P2)                                  # into camera 1
    b = ((P1 - t) @ R) / s                                        # the inverse, into camera 2
    w1 = np.sqrt(sig[c["oct1"][use]].astype(np.float64))[:, None]
    w2 = np.sqrt(sig[c["oct2"][use]].astype(np.float64))[:, None]
    r1 = c["obs1"][use].astype(np.float64) - np.stack([K1[0] * a[:, 0] / a[:, 2] + K1[2], K1[1] * a[:, 1] / a[:, 2] + K1[3]], axis=1)
    r2 = c["obs2"][use].astype(np.float64) - np.stack([K2[0] * b[:, 0] / b[:, 2] + K2[2], K2[1] * b[:, 1] / b[:, 2] + K2[3]], axis=1)
    return np.concatenate([(r1 * w1).ravel(), (r2 * w2).ravel()])


def _gauss_newton(c, use, sig):
    """a Gauss-Newton in numpy float64 on the correspondences `use`, both edges each, no robust kernel, from the true Sim3 to
    convergence; the Jacobian by central differences (step 1e-6) of a left perturbation (omega, dt, dsigma)"""
    R, t, s = c["truth"]
    R, t, s = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64), float(s)
    for _ in range(50):
        r0 = _gn_residual(c, use, sig, R, t, s)
        J = np.zeros((r0.size, 7))
        for d in range(7):
            cols = []
            for sgn in (1.0, -1.0):
                dv = np.zeros(7)
                dv[d] = sgn * 1e-6
                cols.append(_gn_residual(c, use, sig, sc.rot_axis_angle(dv[:3] if d < 3 else [1, 0, 0], np.linalg.norm(dv[:3])) @ R, t + dv[3:6], s * np.exp(dv[6])))
            J[:, d] = (cols[0] - cols[1]) / 2e-6
        step = np.linalg.lstsq(J, -r0, rcond=None)[0]
        R = sc.rot_axis_angle(step[:3] if np.linalg.norm(step[:3]) > 0 else [1, 0, 0], np.linalg.norm(step[:3])) @ R
        t, s = t + step[3:6], s * np.exp(step[6])
        if np.linalg.norm(step) < 1e-12:
            break
    return sc.quat_of(R), t, s


@pytest.mark.parametrize("family", ["clean", "gross_30", "scale_off"])
def test_serial_against_a_gauss_newton_on_the_true_inliers(family):
    """a sane minimiser: with a free scale, at 32 correspondences and more, the Serial Sim3 against a Gauss-Newton (numpy
    float64, written here) on the ground-truth inliers without a kernel, run to convergence; the pairs it removes are exactly the
    displaced ones.  Asserted at 10x the distance measured over the three families (GN_*_MEASURED: what is left is the Levenberg's
    iteration budget -- 5 + 5 or 10 solver calls -- and the 1e-9 step of g2o's numeric Jacobian, not the arithmetic).  With
    fix_scale = 1 the returned scale is the input's by bits."""
    sig = sc.inv_level_sigma2()
    res, flags, _, _ = sc.family_ref(family, sc.SERIAL)
    worst = [0.0, 0.0, 0.0]
    seen = 0
    for i, c in enumerate(sc.family_cases(family)):
        if c["fix_scale"]:
            assert np.float64(res["s"][i]).tobytes() == np.float64(c["s"]).tobytes(), (family, c["n"], c["seed"])
            continue
        if c["n"] < 32:
            continue
        assert res["written"][i] == 1 and np.array_equal(flags[i] != 0, ~c["inlier"]), (family, c["n"], c["seed"])
        assert res["n_in"][i] == c["inlier"].sum()
        gn = _gauss_newton(c, c["inlier"], sig)
        d = sc.sim3_distance((res["q"][i], res["t"][i], res["s"][i]), gn)
        worst = [max(a, b) for a, b in zip(worst, d)]
        seen += 1
    print("%s: Serial against the Gauss-Newton: rotation %.3g rad, translation %.3g, scale %.3g" % (family, worst[0], worst[1], worst[2]))
    assert seen == 12
    assert worst[0] <= 10 * GN_ROT_MEASURED and worst[1] <= 10 * GN_TRANS_MEASURED and worst[2] <= 10 * GN_SCALE_MEASURED


def test_fix_scale_keeps_the_scale_by_bits_in_both_modes():
    for fam in sc.FAMILIES:
        for mode in (sc.SERIAL, sc.DEFINED):
            res = sc.family_ref(fam, mode)[0]
            for i, c in enumerate(sc.family_cases(fam)):
                if c["fix_scale"]:
                    assert np.float64(res["s"][i]).tobytes() == np.float64(c["s"]).tobytes(), (fam, c["n"], c["seed"])


def test_the_stale_error_trap_is_exercised():
    """over the family seeds the restatement's diagnostic shows passes whose LAST Levenberg trial was rejected: the check that
    follows reads the errors of the rejected estimate, the trap the device has to reproduce"""
    total = 0
    for fam in sc.FAMILIES:
        for mode in (sc.SERIAL, sc.DEFINED):
            total += int(sc.family_ref(fam, mode)[2].sum())
    assert total >= 1
    assert sum(int(sc.family_ref(fam, sc.DEFINED)[2][:, 1].sum()) for fam in COMPARED) >= 1   # before a second check that writes


def test_the_early_return_is_exercised():
    """few_left: fewer than 10 correspondences survive the first check, so the function returns 0 before g2oS12 is written, with
    the matches nulled by the first check staying nulled; and nothing below 10 correspondences is ever written back"""
    for mode in (sc.SERIAL, sc.DEFINED):
        res, flags, _, _ = sc.family_ref("few_left", mode)
        hit = 0
        for i, c in enumerate(sc.family_cases("few_left")):
            if c["n"] >= 10:
                assert res["written"][i] == 0 and res["n_in"][i] == 0 and c["n"] - res["n_bad"][i] < 10
                assert (flags[i] == 1).sum() == res["n_bad"][i] > 0 and not (flags[i] == 2).any()
                assert res["q"][i].tobytes() == c["q"].tobytes() and res["t"][i].tobytes() == c["t"].tobytes() and res["s"][i] == c["s"]
                assert res["iterations"][i][0] > 0 and res["iterations"][i][1] == 0 and res["trials"][i][1] == 0
                assert res["lambda_"][i][1] == 0 and res["chi2"][i][1] == 0
                hit += 1
        assert hit >= 1
        for fam in sc.FAMILIES:
            r = sc.family_ref(fam, mode)[0]
            for i, c in enumerate(sc.family_cases(fam)):
                if c["n"] < 10:
                    assert r["written"][i] == 0 and r["n_in"][i] == 0 and (c["n"] == 0) == (r["iterations"][i][0] == 0), (fam, c["n"])
