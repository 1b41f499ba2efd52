"""The device Sim3Solver (orbs_*) against the restatement (tools/sim3_ref.hpp via tests/sim3_cases.py) as bits: every
hypothesis's inlier count, T12, R12, t12, s12 (NaNs by their bits), and for each iterate the flag, bNoMore, nInliers, the
mask and the best fields -- over the scene families, both scale modes, sizes, iteration counts, batches and refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dropin
import sim3_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.9, True, device=0)


def run_case(matcher, case, seed=0, step=5, what=""):
    from orbslamm_amd.sim3 import run_all
    dev = sc.device_solver(matcher, case)
    sets = sc.case_sets(case, dev.max_iterations, seed)
    run_all([dev], [sets])
    outs = sc.compare_solver(dev, case, sets, step, what)
    dev.close()
    return outs


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_families_bit_exact(matcher, name, fix_scale):
    returned = 0
    for seed in (0, 1):
        case = sc.family_case(name, seed, fix_scale=fix_scale)
        outs = run_case(matcher, case, seed, what="%s seed %d fix %d" % (name, seed, fix_scale))
        returned += sum(r["returned"] for r in outs)
    kw, noiseless, quirk = sc.FAMILIES[name]
    if noiseless and fix_scale == kw.get("fix_scale", False):
        assert returned >= 2


def test_constructor_products(matcher):
    """Rcw*Xw + tcw, FromCameraToImage and the truncated thresholds, against numpy float32 mirrors of the same chains"""
    f = np.float32
    case = sc.family_case("general", 3)
    case["sigma2_1"][:8] = sc.SIGMA2
    dev = sc.device_solver(matcher, case)
    p = dev.points()
    e1, e2 = sc.RefSolver(case).thresholds()
    assert sc.same(p["max_error1"], e1) and sc.same(p["max_error2"], e2)
    assert list(p["max_error1"][:8]) == [9, 13, 19, 27, 39, 57, 82, 118]
    for X, Xw, R, t, K, uv in ((p["X1c"], case["X1w"], case["Rcw1"], case["tcw1"], case["K1"], p["p1"]),
                               (p["X2c"], case["X2w"], case["Rcw2"], case["tcw2"], case["K2"], p["p2"])):
        R = R.reshape(3, 3)
        for r in range(3):
            acc = f(f(f(R[r, 0] * Xw[:, 0]) + f(R[r, 1] * Xw[:, 1])) + f(R[r, 2] * Xw[:, 2]))
            assert sc.same(X[:, r], (acc.astype(np.float64) + np.float64(t[r])).astype(f))
        invz = f(1) / X[:, 2]
        assert sc.same(uv[:, 0], f(f(K[0] * f(X[:, 0] * invz)) + K[2])) and sc.same(uv[:, 1], f(f(K[1] * f(X[:, 1] * invz)) + K[3]))
    dev.close()


def test_threshold_truncation_on_the_device(matcher):
    """test_sim3_cpu's 9-versus-9.21 point, on the device"""
    f = np.float32
    K = np.array([500, 500, 320, 240], f)
    X = np.array([[0, 0, 4], [1, 0, 4], [0, 1, 4], [0.5, 0.5, 4], [0.25, 0.75, 4]], f)
    X2 = (X.astype(np.float64) @ sc.rot_axis_angle([0, 0, 1], 0.5)).astype(f)
    X1 = X.copy()
    X1[3, 0] += f(3.02 * 4 / 500)
    X1[4, 0] += f(2.9 * 4 / 500)
    case = dict(n1=5, idx1=np.arange(5, dtype=np.int32), X1w=X1, X2w=X2, Rcw1=np.eye(3, dtype=f).reshape(9), tcw1=np.zeros(3, f),
                Rcw2=np.eye(3, dtype=f).reshape(9), tcw2=np.zeros(3, f), K1=K, K2=K, sigma2_1=np.ones(5, f), sigma2_2=np.ones(5, f),
                fix_scale=True, ransac=(0.99, 3, 300))
    dev = sc.device_solver(matcher, case)
    sets = np.tile(np.array([[0, 1, 2]], np.int32), (dev.max_iterations, 1))
    dev.run(sets)
    outs = sc.compare_solver(dev, case, sets, dev.max_iterations)
    assert outs[0]["returned"] and list(outs[0]["inliers"]) == [True, True, True, False, True]
    dev.close()


def test_repeated_and_degenerate_sets(matcher):
    case = sc.family_case("general", 0)
    case["ransac"] = (0.99, 10, 6)
    dev = sc.device_solver(matcher, case)
    sets = np.array([[5, 5, 5], [3, 3, 9], [9, 3, 3], [7, 8, 7], [1, 2, 3], [4, 4, 4]], np.int32)
    dev.run(sets)
    outs = sc.compare_solver(dev, case, sets, 1, "repeated sets")
    assert outs[0]["has_best"] and np.isnan(outs[0]["best_R"]).all() and outs[4]["returned"]
    dev.close()


@pytest.mark.parametrize("n,min_inliers,max_its", [(3, 2, 300), (4, 3, 300), (7, 6, 300), (20, 10, 300), (63, 10, 64), (64, 10, 65), (65, 10, 1),
                                                   (100, 10, 300), (500, 10, 300), (1024, 20, 300), (1025, 20, 300), (3000, 50, 1000),
                                                   (20000, 100, 4096), (20000, 6, 40)])
def test_sizes_and_iteration_counts(matcher, n, min_inliers, max_its):
    case = sc.family_case("outliers_30" if n >= 20 else "general", 5, n=n, ransac=(0.99, min_inliers, max_its))
    dev = sc.device_solver(matcher, case)
    if (n, max_its) in ((20, 300), (100, 300), (500, 300)):
        assert dev.max_iterations == (35 if n == 20 else 300)
    if max_its == 4096:
        assert dev.max_iterations == 4096
    dev.close()
    run_case(matcher, case, 5, step=max(1, max_its // 7), what="n %d" % n)


@pytest.mark.parametrize("count", [1, 7, 32])
def test_batches_of_unequal_solvers_equal_their_solo_runs(matcher, count):
    from orbslamm_amd.sim3 import run_all
    rng = np.random.default_rng(count)
    names = sorted(sc.FAMILIES)
    cases = []
    for c in range(count):
        name = names[(c * 5 + count) % len(names)]
        over = {} if name.startswith("n_") else dict(n=int(rng.choice([20, 37, 100, 333, 1024, 1500])))
        if "n" in over and not name.startswith(("outliers", "behind", "zero")):
            over["ransac"] = (0.99, 10, int(rng.choice([35, 300])))
        cases.append(sc.family_case(name, c, fix_scale=bool(c & 1), **over))
    devs = [sc.device_solver(matcher, case) for case in cases]
    sets = [sc.case_sets(case, d.max_iterations, seed=c) for c, (case, d) in enumerate(zip(cases, devs))]
    run_all(devs, sets)
    tables = []
    for c, (case, d) in enumerate(zip(cases, devs)):
        tables.append(d.hypotheses().copy())
        sc.compare_solver(d, case, sets[c], 50, "batch of %d, solver %d" % (count, c))
    # and each solver alone gives the same table
    for c, (case, d) in enumerate(zip(cases, devs)):
        solo = sc.device_solver(matcher, case)
        solo.run(sets[c])
        sc.assert_same_table(solo.hypotheses(), tables[c], "solo %d" % c)
        solo.close()
        d.close()
    assert len({len(t) for t in tables}) > 1 or count == 1


def test_state_persists_and_set_ransac_resets_the_cursor_only(matcher):
    case = sc.family_case("outliers_30", 2)
    dev = sc.device_solver(matcher, case)
    sets = sc.case_sets(case, dev.max_iterations, 2)
    dev.run(sets)
    outs = sc.compare_solver(dev, case, sets, 5)
    best = outs[-1]["best_inliers"]
    assert best > 100
    # SetRansacParameters zeroes mnIterations, not mnBestInliers: nothing below the old best is returned any more
    dev.set_ransac(*case["ransac"])
    with pytest.raises(Exception):
        dev.iterate(1)                      # no table: orbs_run comes first
    dev.run(sets)
    r = dev.iterate(dev.max_iterations)
    assert r["best_inliers"] >= best and (not r["returned"] or r["n_inliers"] >= best) and r["iterations"] >= 1


def test_refusals(matcher):
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError
    from orbslamm_amd.sim3 import Sim3Solver, run_all
    case = sc.family_case("general", 0)

    def code(fn):
        with pytest.raises(OrbError) as e:
            fn()
        return e.value.code
    bad = dict(case)
    bad["idx1"] = case["idx1"].copy()
    bad["idx1"][3] = case["n1"]
    assert code(lambda: sc.device_solver(matcher, bad)) == ORBX_E_INVALID
    bad["idx1"][3] = -1
    assert code(lambda: sc.device_solver(matcher, bad)) == ORBX_E_INVALID
    dev = sc.device_solver(matcher, case)
    its = dev.max_iterations
    good = sc.case_sets(case, its)
    assert code(lambda: dev.iterate(1)) == ORBX_E_INVALID            # no table yet
    for v in (-1, dev.n):
        s = good.copy()
        s[its // 2, 1] = v
        assert code(lambda: run_all([dev], [s])) == ORBX_E_INVALID
    assert code(lambda: run_all([dev, dev], [good, good])) == ORBX_E_INVALID
    assert code(lambda: dev.set_ransac(0.999999999, 6, 5000)) == ORBX_E_UNSUPPORTED   # above ORBS_MAX_ITERATIONS
    assert dev.max_iterations == its                                                  # (a refusal changes nothing)
    other = __import__("orbslamm_amd").ORBmatcher(0.9, True, device=0)
    dev2 = sc.device_solver(other, case)
    assert code(lambda: run_all([dev, dev2], [good, good])) == ORBX_E_INVALID
    # N < 3 with N >= min_inliers: the reference would draw from an emptied vector
    tiny = sc.family_case("general", 0, n=2)
    t = Sim3Solver(matcher, tiny["n1"], tiny["idx1"], tiny["X1w"], tiny["X2w"], tiny["Rcw1"], tiny["tcw1"], tiny["Rcw2"], tiny["tcw2"],
                   tiny["K1"], tiny["K2"], tiny["sigma2_1"], tiny["sigma2_2"], False)
    assert code(lambda: t.set_ransac(0.99, 2, 300)) == ORBX_E_UNSUPPORTED
    r = t.iterate(5)                                                 # (0.99, 6, 300): N < min_inliers, bNoMore at once
    assert r["no_more"] and not r["returned"] and r["iterations"] == 0
    # above ORBS_MAX_POINTS
    big = sc.family_case("general", 0, n=65536, n1=65536)
    assert code(lambda: sc.device_solver(matcher, big)) == ORBX_E_UNSUPPORTED
    # an empty solver is allowed and says bNoMore
    empty = sc.family_case("general", 0, n=0, n1=4)
    e = sc.device_solver(matcher, empty)
    run_all([e, dev], [None, good])
    assert e.iterate(3)["no_more"] and len(e.hypotheses()) == 0
    sc.compare_solver(dev, case, good, 5)


def test_end_to_end_bow_matches_to_sim3_to_window_search(gpu):
    """the merge chain on synthetic keyframes through the Python mirror: SearchByBoW between two device-resident frames ->
    Sim3Solver on the matched map points (orbs_run) -> keyframe 2's points projected into keyframe 1 with the returned
    R, t, s -> window_best_frame as SearchBySim3 uses it; equal to the same chain with the restatement in the middle"""
    from orbslamm_amd import ORBextractor, ORBmatcher, ORBVocabulary, make_grid, synth
    from orbslamm_amd.sim3 import Sim3Solver, make_sim3_sets
    from vocab_cases import make_vocab
    w, h, nf = 640, 480, 1000
    rng = np.random.default_rng(191)
    voc = make_vocab(rng, 10, 4)
    G = ORBVocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
    fr = synth.make_frames(w, h, 2, stream=4)
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2, device=0)
    gex.extract_batch_device(*gex.upload_frames(fr))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    (k1, d1), (k2, d2) = [gex.download(f) for f in range(2)]
    K, D0 = np.array([517.3, 516.5, 318.6, 255.3], np.float32), [0, 0, 0, 0, 0]
    m = ORBmatcher(0.75, True, device=0)
    g = make_grid(0.0, 0.0, float(w), float(h))
    frames = [m.frame_from_device(dk + f * cap * 28, dd + f * cap * 32, n, K, D0, g) for f, n in ((0, len(k1)), (1, len(k2)))]
    for F in frames:
        m.frame_compute_bow(F, G, 4)
    m12, nm = m.SearchByBoWFrames(frames[0], None, frames[1], None, False)     # vpMatches12: per key of keyframe 1
    assert nm > 50
    # map points: keyframe 2's keys unprojected at seeded depths in its camera; keyframe 1's matched keys see the same
    # points under a true Sim3 (a fifth of them wrong), in map 1's world frame
    f64 = np.float64
    z2 = rng.uniform(3, 9, len(k2))
    X2c = np.stack([(k2["x"].astype(f64) - K[2]) / K[0] * z2, (k2["y"].astype(f64) - K[3]) / K[1] * z2, z2], axis=1)
    Rt, st, tt = sc.rot_axis_angle([0.2, 1, 0.1], 0.35), 1.4, np.array([0.3, -0.1, 0.6])
    Rcw1, tcw1 = sc.rot_axis_angle([0.2, 1.0, -0.3], 0.7), np.array([0.5, -1.0, 2.0])
    Rcw2, tcw2 = sc.rot_axis_angle([-0.5, 0.3, 1.0], -1.1), np.array([-3.0, 0.4, 1.0])
    idx1 = np.flatnonzero(m12 >= 0).astype(np.int32)
    src = m12[idx1].copy()
    wrong = rng.uniform(size=len(idx1)) < 0.2
    src[wrong] = rng.integers(0, len(k2), int(wrong.sum()))
    X1c = st * X2c[src] @ Rt.T + tt
    sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    case = dict(n1=len(k1), idx1=idx1, X1w=((X1c - tcw1) @ Rcw1).astype(np.float32), X2w=((X2c[m12[idx1]] - tcw2) @ Rcw2).astype(np.float32),
                Rcw1=Rcw1.astype(np.float32).reshape(9), tcw1=tcw1.astype(np.float32), Rcw2=Rcw2.astype(np.float32).reshape(9),
                tcw2=tcw2.astype(np.float32), K1=K, K2=K, sigma2_1=(sf * sf)[k1["octave"][idx1]], sigma2_2=(sf * sf)[k2["octave"][m12[idx1]]],
                fix_scale=False, ransac=(0.99, 20, 300))
    dev = sc.device_solver(m, case)
    sets = make_sim3_sets(dev.n, dev.max_iterations, seed=3)
    dev.run(sets)
    ref = sc.ref_solve(case, sets=sets)
    got, want = dev.find(), ref.find()
    sc.assert_same_result(got, want, "end to end")
    assert want["returned"] and want["n_inliers"] > 0.6 * len(idx1)

    def search_by_sim3(res):
        # SearchBySim3's first half (ORBmatcher.cc:1104): keyframe 2's points into keyframe 1 with sR12, t12
        f = np.float32
        sR = (res["best_s"] * res["best_R"]).astype(f)
        Xw2 = ((X2c - tcw2) @ Rcw2).astype(f)
        Xc2 = (Xw2 @ Rcw2.astype(f).T + tcw2.astype(f)).astype(f)
        P = (Xc2 @ sR.T + res["best_t"]).astype(f)
        ok = P[:, 2] > 0
        invz = f(1) / np.where(ok, P[:, 2], f(1))
        u, v = K[0] * P[:, 0] * invz + K[2], K[1] * P[:, 1] * invz + K[3]
        ok &= (u >= 0) & (u < w) & (v >= 0) & (v < h)
        lvl = np.clip(k2["octave"], 0, 7)
        uvr = np.stack([u, v, f(7.5) * sf[lvl]], axis=1).astype(f)[ok]
        return m.window_best_frame(uvr, lvl.astype(np.int8)[ok], d2[ok], None, frames[0], None, False), int(ok.sum())
    (bi_g, bd_g), nq = search_by_sim3(got)
    (bi_w, bd_w), _ = search_by_sim3(want)
    assert np.array_equal(bi_g, bi_w) and np.array_equal(bd_g, bd_w) and nq > 100
    dev.close()
    for F in frames:
        m.frame_destroy(F)


def test_sim3_dropin_on_mock_keyframes(gpu):
    """include/Sim3Solver_hip.hpp (Sim3SolverT, RunAll) on mock keyframes (tests/cpp/sim3_dropin_gpu.cpp) through
    MultiMapper's round-robin loop against tools/sim3_ref.hpp, and the process's rand() position after RunAll"""
    dropin.run(dropin.build("sim3_dropin_gpu"), timeout=600, marker="sim3 dropin ok")


def test_soak_slice(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "soak", "fuzz_sim3.py"), "60", "107"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "sim3 soak: 60 cases" in out.stdout and "equal" in out.stdout
