"""The device OptimizeSim3 (orbz_optimize_sim3) against the restatement's Defined mode (tools/sim3opt_ref.hpp) AS
BITS: every field of OrbzResult (the doubles and their NaNs by their bit patterns) and the removed bytes, over every scene
family x 3 seeds x both fix_scale x the correspondence counts 0, 1, 9, 10, 31, 32, 33, 150 and 1 000 (no edge; the early-return
border; 64 edges, the border of the partials; 32 edges on a lane); batches against single problems; the same call twice; two
keyframes with different K and level tables; the drop-in on the mock.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import numpy as np
import pytest

import dropin
import sim3opt_cases as sc
from orbslamm_amd import optimizer as opt
from orbslamm_amd._lib import lib

pytestmark = pytest.mark.gpu
SIG = sc.inv_level_sigma2()
FIELDS = ("q", "t", "s", "written", "n_corr", "n_bad", "n_in", "iterations", "trials", "lambda_", "chi2")


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.9, True, device=0)


def item_of(c):
    it = {k: c[k] for k in ("R1w", "t1w", "K1", "R2w", "t2w", "K2", "idx1", "obs1", "oct1", "obs2", "oct2", "X1w", "X2w", "th2", "fix_scale")}
    it["S12"] = (c["q"], c["t"], c["s"])
    return it


def device_run(matcher, cases, sig1=SIG, sig2=SIG):
    """one call for all cases: (SIM3_RESULT_DTYPE array, removed bytes, corr_start)"""
    probs = np.concatenate([opt.pack_sim3_problem(item_of(c)) for c in cases]) if cases else np.zeros(0, opt.SIM3_PROBLEM_DTYPE)
    corrs = [opt.pack_sim3_corrs(c) for c in cases]
    start = np.concatenate([[0], np.cumsum([c["n"] for c in cases])]).astype(np.int32)
    allc = np.concatenate(corrs) if corrs else np.zeros(0, opt.SIM3_CORR_DTYPE)
    rc, out, flags = opt.optimize_sim3_raw(matcher._h, probs, start, allc, sig1, sig2)
    assert rc == 0, lib().orbx_last_error().decode()
    return out, flags, start


def assert_bits(out, flags, start, i, ref, ref_flags, j, tag):
    """problem i of a device call against problem j of a restatement run, as bytes"""
    for name in FIELDS:
        assert out[name][i].tobytes() == ref[name][j].tobytes(), (tag, name, out[name][i], ref[name][j])
    assert flags[start[i]:start[i + 1]].tobytes() == ref_flags[j].tobytes(), (tag, "removed")


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_device_equals_defined_as_bits(matcher, family):
    """every count x seed x fix_scale of the family, each problem in a call of its own"""
    cases = sc.family_cases(family)
    ref, ref_flags, _, _ = sc.family_ref(family, sc.DEFINED)
    assert len(cases) == len(sc.SEEDS) * 2 * len(sc.COUNTS)
    for j, c in enumerate(cases):
        out, flags, start = device_run(matcher, [c])
        assert_bits(out, flags, start, 0, ref, ref_flags, j, (family, c["n"], c["seed"], c["fix_scale"]))
    # the early return is on both sides of its border: nothing below 10 correspondences is written back
    assert not any(ref["written"][j] for j, c in enumerate(cases) if c["n"] < 10)
    if family in ("clean", "gross_30", "far_start", "mixed_octaves"):
        assert all(ref["written"][j] for j, c in enumerate(cases) if c["n"] >= 31)
    if family == "few_left":
        assert any(ref["written"][j] == 0 and (ref_flags[j] == 1).any() for j, c in enumerate(cases) if c["n"] >= 31)


def _mixed(k):
    """k problems of mixed families, counts and fix_scale, empty problems in the middle included"""
    fams = [sc.FAMILIES[i % len(sc.FAMILIES)] for i in range(k)]
    counts = [150, 0, 33, 1, 1000, 0, 9, 32, 10, 31, 150, 0, 33, 9, 1000, 32, 10]
    return [sc.make_case(f, counts[i % len(counts)], 900 + i, i % 2) for i, f in enumerate(fams)]


@pytest.mark.parametrize("k", [1, 2, 17])
def test_a_batch_equals_its_single_problems_and_the_restatement(matcher, k):
    cases = _mixed(k)
    ref, ref_flags, _, _ = sc.ref_run(sc.DEFINED, cases)
    out, flags, start = device_run(matcher, cases)
    assert out.shape[0] == k
    for i, c in enumerate(cases):
        assert_bits(out, flags, start, i, ref, ref_flags, i, ("batch", k, i))
        one, f1, _ = device_run(matcher, [c])
        assert one.tobytes() == out[i:i + 1].tobytes() and f1.tobytes() == flags[start[i]:start[i + 1]].tobytes(), (k, i)
    again, flags2, _ = device_run(matcher, cases)
    assert again.tobytes() == out.tobytes() and flags2.tobytes() == flags.tobytes()      # the same call twice: the same bytes


def test_zero_problems(matcher):
    rc, out, flags = opt.optimize_sim3_raw(matcher._h, np.zeros(0, opt.SIM3_PROBLEM_DTYPE), [0], np.zeros(0, opt.SIM3_CORR_DTYPE), SIG, SIG)
    assert rc == 0 and out.shape[0] == 0 and flags.shape[0] == 0


def test_two_cameras_and_two_level_tables(matcher):
    """pKF1 and pKF2 with different K and different mvInvLevelSigma2: a swapped cam_map1 / cam_map2 or table cannot pass.  The
    restatement with the two swapped gives another answer, so the case tells them apart."""
    K2 = np.array([458.7, 457.3, 367.2, 248.4], dtype=np.float32)
    sig2 = sc.inv_level_sigma2().copy()
    sf = np.float32(1.0)
    for i in range(1, sc.NLEVELS):
        sf = np.float32(sf * np.float32(1.3))
        sig2[i] = np.float32(1.0) / (sf * sf)
    cases = [sc.make_case("mixed_octaves", n, 41, fs, K2=K2) for n in (33, 150) for fs in (0, 1)]
    ref, ref_flags, _, _ = sc.ref_run(sc.DEFINED, cases, sig1=SIG, sig2=sig2)
    swapped, _, _, _ = sc.ref_run(sc.DEFINED, cases, sig1=sig2, sig2=SIG)
    assert all(ref["written"]) and ref["q"].tobytes() != swapped["q"].tobytes()
    out, flags, start = device_run(matcher, cases, SIG, sig2)
    for i in range(len(cases)):
        assert_bits(out, flags, start, i, ref, ref_flags, i, ("two cameras", i))
    # the mirror's front door on the first of them
    r = opt.optimize_sim3(matcher, item_of(cases[0]), SIG, sig2)
    assert r["written"] and r["n_in"] == ref["n_in"][0] and r["S12"][0].tobytes() == ref["q"][0].tobytes()
    assert r["removed"].tobytes() == ref_flags[0].tobytes()


def test_sim3opt_dropin_on_mock_keyframes(gpu):
    """include/Optimizer_hip.hpp (OptimizeSim3T::Run, RunAll) on mock keyframes (tests/cpp/sim3opt_dropin_gpu.cpp) against
    tools/sim3opt_ref.hpp run on the same mocks"""
    dropin.run(dropin.build("sim3opt_dropin_gpu"), timeout=300, marker="sim3opt dropin ok")
