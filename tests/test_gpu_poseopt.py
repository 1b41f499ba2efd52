"""The device PoseOptimization (orbo_pose_optimize*) against the restatement's Defined mode
(tools/poseopt_ref.hpp) AS BITS: every field of OrboResult (the doubles and their NaNs by their bit patterns) and the outlier
bytes, over every scene family x 3 seeds x the edge counts 0, 2, 3, 9, 10, 63, 64, 65, 300 and 2000 (the `< 3` return, the
`< 10` break, the lane boundary of the one wave that serves a frame, many edges per lane); batches against single frames;
the host-array and resident-frame entries against each other; the same call twice; the drop-in on the mock.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import numpy as np
import pytest

import dropin
import poseopt_cases as pc
from orbslamm_amd import optimizer as opt
from orbslamm_amd._lib import ORBX_E_INVALID, lib

pytestmark = pytest.mark.gpu
SIG = pc.inv_level_sigma2()


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.9, True, device=0)


def device_run(matcher, cases, resident=None):
    """one call for all cases: (RESULT_DTYPE array, outlier bytes, edge_start)"""
    frames = np.zeros(len(cases), dtype=opt.FRAME_DTYPE)
    for i, c in enumerate(cases):
        frames["Tcw"][i], frames["K"][i] = c["Tcw"].reshape(16), c["K"]
    start = np.concatenate([[0], np.cumsum([c["n"] for c in cases])]).astype(np.int32)
    edges = np.concatenate([opt.pack_edges(c["feature"], c["Xw"]) for c in cases]) if cases else np.zeros(0, opt.EDGE_DTYPE)
    rc, out, flags = opt.pose_optimize_raw(matcher._h, frames, None if resident else [c["keys_un"] for c in cases], resident, start, edges, SIG)
    assert rc == 0, lib().orbx_last_error().decode()
    return out, flags, start


def assert_bits(out, flags, start, i, ref, ref_flags, j, tag):
    """frame i of a device call against frame j of a restatement run, as bytes (the padding word aside)"""
    for name in ("Tcw", "n_initial", "n_good", "rounds", "iterations", "trials", "lambda_", "chi2"):
        assert out[name][i].tobytes() == ref[name][j].tobytes(), (tag, name, out[name][i], ref[name][j])
    assert flags[start[i]:start[i + 1]].tobytes() == ref_flags[j].tobytes(), (tag, "outlier")


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_device_equals_defined_as_bits(matcher, family):
    """every count x seed of the family, each frame in a call of its own"""
    cases = pc.family_cases(family)
    ref, ref_flags, _, _ = pc.family_ref(family, pc.DEFINED)
    for j, c in enumerate(cases):
        out, flags, start = device_run(matcher, [c])
        assert_bits(out, flags, start, 0, ref, ref_flags, j, (family, c["n"], c["seed"]))
    ran = [c for c in cases if c["n"] >= 10]
    assert all(r == 4 for r in ref["rounds"][[j for j, c in enumerate(cases) if c["n"] >= 10]]) and len(ran) == 18


def _mixed(k):
    """k frames of mixed families and counts, empty frames in the middle included"""
    fams = [pc.FAMILIES[i % len(pc.FAMILIES)] for i in range(k)]
    counts = [300, 0, 65, 2, 2000, 0, 9, 64, 3, 10, 63, 300, 0, 2000, 65, 9, 64]
    return [pc.make_case(f, counts[i % len(counts)], 900 + i) for i, f in enumerate(fams)]


@pytest.mark.parametrize("k", [1, 2, 17])
def test_a_batch_equals_its_single_frames_and_the_restatement(matcher, k):
    cases = _mixed(k)
    ref, ref_flags, _, _ = pc.ref_run(pc.DEFINED, cases)
    out, flags, start = device_run(matcher, cases)
    assert out.shape[0] == k
    for i, c in enumerate(cases):
        assert_bits(out, flags, start, i, ref, ref_flags, i, ("batch", k, i))
        one, f1, s1 = device_run(matcher, [c])
        assert one.tobytes()[:176] == out[i:i + 1].tobytes() and f1.tobytes() == flags[start[i]:start[i + 1]].tobytes(), (k, i)
    again, flags2, _ = device_run(matcher, cases)
    assert again.tobytes() == out.tobytes() and flags2.tobytes() == flags.tobytes()      # the same call twice: the same bytes


def test_zero_frames(matcher):
    rc, out, flags = opt.pose_optimize_raw(matcher._h, np.zeros(0, opt.FRAME_DTYPE), [], None, [0], np.zeros(0, opt.EDGE_DTYPE), SIG)
    assert rc == 0 and out.shape[0] == 0 and flags.shape[0] == 0


def test_resident_frames_give_the_host_arrays_bytes(matcher):
    """a frame extracted and undistorted on the device: its keys as host arrays (orbo_pose_optimize) and where they lie
    (orbo_pose_optimize_frames) give the same bytes, which are the restatement's; an octave outside nlevels, which only the
    device can see in a resident frame, is refused"""
    from orbslamm_amd import ORBextractor, make_grid, synth
    w, h, nf = 640, 480, 1000
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2, device=0)
    gex.extract_batch_device(*gex.upload_frames(synth.make_frames(w, h, 2, stream=3)))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    rng = np.random.default_rng(5)
    cases, resident = [], []
    for f in range(2):
        k0, _ = gex.download(f)
        F = matcher.frame_from_device(dk + f * cap * 28, dd + f * cap * 32, len(k0), pc.K_TUM, [0.1, -0.05, 0.001, 0.0005, 0.0],
                                      make_grid(0.0, 0.0, float(w), float(h)))
        ku = matcher.frame_keys_un(F)
        assert len(ku) > 300 and ku["octave"].max() >= 3
        # map points: a third of the keys unprojected at seeded depths under a true pose, a sixth of those wrong
        feat = np.sort(rng.choice(len(ku), size=len(ku) // 3, replace=False)).astype(np.int32)
        Rt, tt = pc.rot_axis_angle([0.1, 1, 0.2], 0.2 + 0.1 * f), np.array([0.3, -0.1, 0.4])
        depth = rng.uniform(2, 8, feat.size)
        fx, fy, cx, cy = [float(v) for v in pc.K_TUM]
        Xc = np.stack([(ku["x"][feat] - cx) / fx * depth, (ku["y"][feat] - cy) / fy * depth, depth], axis=1)
        Xw = ((Xc - tt) @ Rt).astype(np.float32)
        wrong = rng.random(feat.size) < 1 / 6
        Xw[wrong] += rng.uniform(0.3, 1.0, (int(wrong.sum()), 3)).astype(np.float32)
        Rs = pc.rot_axis_angle([1, 0.2, -0.3], np.deg2rad(2.0)) @ Rt
        cases.append(dict(Tcw=pc.tcw_of(Rs, tt + 0.03), K=pc.K_TUM.copy(), keys_un=ku, feature=feat, Xw=Xw, n=feat.size))
        resident.append(F)
    ref, ref_flags, _, _ = pc.ref_run(pc.DEFINED, cases)
    host, hflags, start = device_run(matcher, cases)
    res, rflags, _ = device_run(matcher, cases, resident=resident)
    assert host.tobytes() == res.tobytes() and hflags.tobytes() == rflags.tobytes()
    for i in range(2):
        assert_bits(host, hflags, start, i, ref, ref_flags, i, ("resident", i))
        assert 0 < host["n_good"][i] < cases[i]["n"] and host["rounds"][i] == 4
    # the mirror's front door, on a resident frame
    r = opt.pose_optimization(matcher, cases[0]["Tcw"], pc.K_TUM, None, cases[0]["feature"], cases[0]["Xw"], SIG, frame=resident[0])
    assert r["n_good"] == host["n_good"][0] and r["Tcw"].tobytes() == host["Tcw"][0].tobytes() and r["outlier"].sum() == hflags[:start[1]].sum()
    # an octave outside nlevels: with 3 levels the frame's keys of level 3 and up are out of range
    frames = np.zeros(1, dtype=opt.FRAME_DTYPE)
    frames["Tcw"][0], frames["K"][0] = cases[0]["Tcw"].reshape(16), pc.K_TUM
    edges = opt.pack_edges(cases[0]["feature"], cases[0]["Xw"])
    assert (cases[0]["keys_un"]["octave"][cases[0]["feature"]] >= 3).any()
    rc, _, _ = opt.pose_optimize_raw(matcher._h, frames, None, resident[:1], [0, edges.shape[0]], edges, SIG[:3])
    assert rc == ORBX_E_INVALID and "octave" in lib().orbx_last_error().decode()
    rc, _, _ = opt.pose_optimize_raw(matcher._h, frames, [cases[0]["keys_un"]], None, [0, edges.shape[0]], edges, SIG[:3])
    assert rc == ORBX_E_INVALID and "octave" in lib().orbx_last_error().decode()
    for F in resident:
        matcher.frame_destroy(F)


def test_poseopt_dropin_on_mock_frames(gpu):
    """include/Optimizer_hip.hpp (PoseOptimizationT::Run, RunAll) on mock frames (tests/cpp/poseopt_dropin_gpu.cpp) against
    tools/poseopt_ref.hpp run on the same mocks"""
    dropin.run(dropin.build("poseopt_dropin_gpu"), timeout=300, marker="poseopt dropin ok")
