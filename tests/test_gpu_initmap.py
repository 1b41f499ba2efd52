"""The device initial map (orbb_initial_map*) against the restatement's Defined mode (tools/initmap_ref.hpp) AS
BITS: every field of OrbbResult (the doubles and their NaNs by their bit patterns) and every point record, over every scene
family x size x open seed of initmap_cases.py, one batched call per family; a problem alone, at another position of a batch
and in a repeated call; bRobust off and the second pose fixed alone; the resident-frame entry against the host-array entry;
the drop-in on mocks, which also holds the normal / depth outputs to the reference's own member.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""
import importlib

import numpy as np
import pytest

import dropin
import initmap_cases as ic
from orbslamm_amd._lib import ORBX_E_INVALID, lib

im = importlib.import_module("orbslamm_amd.initial_map")
pytestmark = pytest.mark.gpu
RESULT_FIELDS = [n for n in im.RESULT_DTYPE.names if n != "_pad"]
POINT_FIELDS = [n for n in im.POINT_DTYPE.names if n != "_pad"]


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.9, True, device=0)


def device_run(matcher, cases, family=None, resident=None):
    """one call for all cases: (RESULT_DTYPE array, [POINT_DTYPE array per case])"""
    problems = np.zeros(len(cases), dtype=im.PROBLEM_DTYPE)
    for i, c in enumerate(cases):
        problems[i] = im.pack_problem(c)
    sig = ic.inv_level_sigma2(family or cases[0]["family"])
    rc, out, points = im.initial_map_raw(matcher._h, problems, None if resident else [c["keys_un1"] for c in cases],
                                         None if resident else [c["keys_un2"] for c in cases], resident and [r[0] for r in resident],
                                         resident and [r[1] for r in resident], [c["matches12"] for c in cases], [c["P3D"] for c in cases], sig,
                                         ic.scale_factors())
    assert rc == 0, lib().orbx_last_error().decode()
    return out, points


def assert_bits(out, points, i, ref, tag):
    """problem i of a device call against a restatement run (result, points, diagnostics), as bytes"""
    res, pts, _ = ref
    for name in RESULT_FIELDS:
        assert out[name][i].tobytes() == res[name].tobytes(), (tag, name, out[name][i], res[name])
    assert points[i].shape == pts.shape, tag
    for name in POINT_FIELDS:
        if points[i][name].tobytes() != pts[name].tobytes():
            bad = np.nonzero((points[i][name] != pts[name]).reshape(pts.shape[0], -1).any(axis=1))[0]
            raise AssertionError((tag, name, bad[:5], points[i][name][bad[:2]], pts[name][bad[:2]]))
    assert points[i].tobytes() == pts.tobytes(), (tag, "padding")


@pytest.mark.parametrize("family", list(ic.FAMILIES))
def test_device_equals_defined_as_bits(matcher, family):
    """every size x open seed of the family in ONE batched call"""
    cases = ic.family_cases(family)
    ref = ic.family_ref(family, ic.DEFINED)
    out, points = device_run(matcher, cases)
    assert out.shape[0] == len(cases)
    for i, c in enumerate(cases):
        assert_bits(out, points, i, ref[i], (family, c["n"], c["seed"]))


def test_a_problem_alone_at_any_position_and_twice(matcher):
    """a problem's bytes do not depend on the batch around it, on its place in it, or on the call before"""
    picks = [("noisy", 65, 3), ("both_free", 130, 2), ("gross_20", 1, 1), ("no_points", 64, 1), ("far_start", 600, 4), ("few", 89, 1)]
    cases = [ic.make_case(f, n, s) for f, n, s in picks]
    plain = dict(ic.make_case("mixed_octaves", 130, 7))
    plain["robust"] = False                                           # bRobust off: the other form of Hpl's block, no kernel
    second = dict(ic.make_case("noisy", 90, 8))
    second["fixed_first"], second["fixed_second"] = False, True       # the second pose fixed alone: pose 0 is the free one
    cases, picks = cases + [plain, second], picks + [("plain", 130, 7), ("second_fixed", 90, 8)]
    ref = [ic.ref_run(c, ic.DEFINED) for c in cases]
    assert ref[-2][0]["iterations"] >= 3 and ref[-1][0]["iterations"] >= 3 and not np.array_equal(ref[-1][0]["Tcw1"], second["Tcw1"][:3].reshape(12))
    out, points = device_run(matcher, cases, family="noisy")
    again, points2 = device_run(matcher, cases, family="noisy")
    assert again.tobytes() == out.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(points, points2))
    rev, rpoints = device_run(matcher, cases[::-1], family="noisy")
    for i, c in enumerate(cases):
        assert_bits(out, points, i, ref[i], ("batch", picks[i]))
        one, p1 = device_run(matcher, [c], family="noisy")
        assert one.tobytes() == out[i:i + 1].tobytes() and p1[0].tobytes() == points[i].tobytes(), picks[i]
        j = len(cases) - 1 - i
        assert rev[j:j + 1].tobytes() == out[i:i + 1].tobytes() and rpoints[j].tobytes() == points[i].tobytes(), picks[i]


def test_zero_problems_and_the_front_door(matcher):
    rc, out, points = im.initial_map_raw(matcher._h, np.zeros(0, im.PROBLEM_DTYPE), [], [], None, None, [], [], ic.inv_level_sigma2(), ic.scale_factors())
    assert rc == 0 and out.shape[0] == 0 and points == []
    c = ic.make_case("noisy", 130, 5)
    res, pts, _ = ic.ref_run(c, ic.DEFINED)
    import orbslamm_amd
    r = orbslamm_amd.initial_map(matcher, c["Tcw1"], c["Tcw2"], c["K"], c["keys_un1"], c["keys_un2"], c["matches12"], c["P3D"], ic.inv_level_sigma2(),
                                 ic.scale_factors())
    assert r["verdict"] == im.OK == res["verdict"] and r["n_points"] == 130 and r["points"].tobytes() == pts.tobytes()
    assert r["Tcw2_scaled"][:3].astype(np.float32).tobytes() == res["Tcw2_scaled"].tobytes() and r["median_depth"] == res["median_depth"]
    assert orbslamm_amd.initial_map_batch(matcher, [], ic.inv_level_sigma2(), ic.scale_factors()) == []


def test_resident_frames_give_the_host_arrays_bytes(matcher):
    """two frames extracted and undistorted on the device: their keys as host arrays (orbb_initial_map) and where they lie
    (orbb_initial_map_frames) give the same bytes, which are the restatement's; an octave outside nlevels, which only the
    device can see in a resident frame, is refused"""
    from orbslamm_amd import ORBextractor, make_grid, synth
    w, h, nf = 640, 480, 1000
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2, device=0)
    gex.extract_batch_device(*gex.upload_frames(synth.make_frames(w, h, 2, stream=3)))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    F, ku = [], []
    for f in range(2):
        k0, _ = gex.download(f)
        F.append(matcher.frame_from_device(dk + f * cap * 28, dd + f * cap * 32, len(k0), ic.K, [0.1, -0.05, 0.001, 0.0005, 0.0],
                                           make_grid(0.0, 0.0, float(w), float(h))))
        ku.append(matcher.frame_keys_un(F[-1]))
    n1, n2 = len(ku[0]), len(ku[1])
    assert n1 > 300 and n2 > 300 and ku[0]["octave"].max() >= 3
    # a third of frame 1's keys matched to distinct keys of frame 2; the points unprojected from frame 1 at seeded depths (the
    # second observation is whatever key the match names: a scene with large residuals, which the bytes do not mind)
    rng = np.random.default_rng(11)
    feat1 = np.sort(rng.choice(n1, size=n1 // 3, replace=False))
    matches12 = np.full(n1, -1, dtype=np.int32)
    matches12[feat1] = rng.permutation(n2)[:feat1.size]
    depth = rng.uniform(3, 8, feat1.size)
    fx, fy, cx, cy = [float(v) for v in ic.K]
    P3D = np.zeros((n1, 3), dtype=np.float32)
    P3D[feat1] = np.stack([(ku[0]["x"][feat1] - cx) / fx * depth, (ku[0]["y"][feat1] - cy) / fy * depth, depth], axis=1)
    T2 = np.eye(4, dtype=np.float32)
    T2[:3, 3] = [-0.5, 0.02, 0.01]
    case = dict(family="noisy", Tcw1=np.eye(4, dtype=np.float32), Tcw2=T2, K=ic.K, keys_un1=ku[0], keys_un2=ku[1], matches12=matches12, P3D=P3D,
                fixed_first=True, iterations=20, robust=True)
    ref = ic.ref_run(case, ic.DEFINED)
    host, hp = device_run(matcher, [case])
    res, rp = device_run(matcher, [case], resident=[(F[0], F[1])])
    assert host.tobytes() == res.tobytes() and hp[0].tobytes() == rp[0].tobytes()
    assert_bits(host, hp, 0, ref, "resident")
    assert host["n_points"][0] == feat1.size and host["iterations"][0] >= 1
    # an octave outside nlevels: with 3 levels the frames' keys of level 3 and up are out of range
    assert (ku[0]["octave"][feat1] >= 3).any()
    pr = np.zeros(1, dtype=im.PROBLEM_DTYPE)
    pr[0] = im.pack_problem(case)
    for resident in (True, False):
        rc, _, _ = im.initial_map_raw(matcher._h, pr, None if resident else [ku[0]], None if resident else [ku[1]], [F[0]] if resident else None,
                                      [F[1]] if resident else None, [matches12], [P3D], ic.inv_level_sigma2()[:3], ic.scale_factors()[:3])
        assert rc == ORBX_E_INVALID and "octave" in lib().orbx_last_error().decode()
    for f in F:
        matcher.frame_destroy(f)


def test_initmap_dropin_on_mock_keyframes(gpu):
    """include/Tracking_hip.hpp (InitialMapT::Run) on mock keyframes and map points (tests/cpp/initmap_dropin_gpu.cpp): the map ends
    as Tracking.cc:728-758 written serially over tools/initmap_ref.hpp leaves it"""
    dropin.run(dropin.build("initmap_dropin_gpu"), timeout=300, marker="initmap dropin ok")


@pytest.mark.parametrize("family,n,seed", [("mixed_octaves", 65, 2), ("mixed_octaves", 130, 5), ("both_free", 90, 3)])
def test_normal_and_depth_equal_orbr_refresh_points_on_a_two_keyframe_store(matcher, family, n, seed):
    """the header says the normal / depth outputs are the normal / depth half of orbslamm_refresh.h: held here to that kernel itself.
    The two keyframes go into a store (slot 0 the initial one, slot 1 the current one: the ascending slot is the defined order) with
    the adjusted centres and their octaves, every point into a pool with its two observations in the keyframes' match slots, and
    orbr_refresh_points runs with ref_kf = the current keyframe and new_pos = the adjusted positions: normal, both bounds and the
    status are the same bytes"""
    from orbslamm_amd import KeyFrameStore, MapPool, map_pool
    c = ic.make_case(family, n, seed)
    out, points = device_run(matcher, [c])
    pts = points[0]
    feat1 = np.nonzero(pts["matched"] == 1)[0]
    assert feat1.size == n and np.array_equal(feat1, np.nonzero(c["matches12"] >= 0)[0])
    if family == "mixed_octaves":
        assert len(set(c["keys_un2"]["octave"][c["matches12"][feat1]].tolist())) >= 4
    ids = np.arange(n, dtype=np.int32)
    pool = MapPool(matcher, n)
    pool.set(ids, map_pool.map_points(c["P3D"][feat1], np.zeros((n, 3)), 0.0, 0.0, np.zeros((n, 32), np.uint8), map_pool.FLAG_OBSERVED))
    n1, n2 = c["keys_un1"].shape[0], c["keys_un2"].shape[0]
    rows = [np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)]
    rows[0][feat1] = ids
    rows[1][c["matches12"][feat1]] = ids
    store = KeyFrameStore(pool, 2, max(n1, n2), 4, 2 * max(n1, n2))
    store.set([0, 1], [0, 0], rows, [[], []], [-1, -1], [[], []])
    store.set_octaves(0, c["keys_un1"]["octave"])
    store.set_octaves(1, c["keys_un2"]["octave"])
    store.set_centres([0, 1], np.stack([out["Ow1"][0], out["Ow2"][0]]))
    got = store.refresh_points(ids, np.ones(n, np.int32), ic.scale_factors(), map_pool.REFRESH_NORMAL_DEPTH, pts["pos"][feat1], commit=False)
    assert np.all(got["n_obs"] == 2) and got["st_normal_depth"].tobytes() == pts["status"][feat1].tobytes() and np.all(got["st_normal_depth"] == 1)
    for name in ("pos", "normal", "min_distance", "max_distance"):
        assert got[name].tobytes() == pts[name][feat1].tobytes(), (family, n, seed, name)
