"""The PnPsolver restatement's contract (tools/pnp_ref.hpp via tests/pnp_cases.py), no GPU: its OpenCV pieces against numpy,
the set drawing, SetRansacParameters, the scene families against float64 geometry, iterate's state machine (the OR loop,
the capacity boundary, Refine's returns), and the orbp_* block's header / exports / struct sizes."""
import ctypes as C
import os

import numpy as np
import pytest

import dropin
import pnp_cases as pc
import ref_shim
from orbslamm_amd._lib import RAND_MAX, libc, random_int, seed_rand
from orbslamm_amd.pnp import EXTRA_SETS, make_pnp_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ OpenCV pieces
def _check_svd(A, tol=1e-12):
    w, ut, vt = pc.ref_svd(A)
    m, n = A.shape
    scale = max(1.0, np.abs(A).max())
    assert np.all(np.diff(w) <= 0) and np.abs(w - np.linalg.svd(A, compute_uv=False)).max() <= tol * scale
    assert np.abs(ut.T @ np.diag(w) @ vt - A).max() <= tol * scale           # reconstruction
    assert np.abs(vt @ vt.T - np.eye(n)).max() <= tol
    return w, ut, vt


def test_jacobi_svd_against_numpy():
    rng = np.random.default_rng(1)
    B = rng.normal(size=(12, 8))
    A = B @ B.T                                                              # symmetric PSD of rank 8, as MtM is
    w, ut, _ = _check_svd(A, 1e-11)
    assert np.all(w[8:] <= 1e-12 * w[0])
    assert np.abs(ut @ ut.T - np.eye(12)).max() <= 1e-9                      # the null vectors are orthonormal too
    assert np.abs(A @ ut[8:].T).max() <= 1e-10 * w[0]
    for shape in ((3, 3), (6, 4), (6, 3), (6, 5)):
        w, ut, _ = _check_svd(rng.normal(size=shape))
        assert np.abs(ut @ ut.T - np.eye(shape[1])).max() <= 1e-12
    # an exactly zero matrix: every singular value 0, the left vectors come from the random completion, unit length
    w, ut, vt = pc.ref_svd(np.zeros((3, 3)))
    assert not w.any() and np.allclose((ut * ut).sum(axis=1), 1.0) and pc.same(vt, np.eye(3))


def test_svd_solves_inverse_and_qr_against_numpy():
    rng = np.random.default_rng(2)
    for nc in (4, 3, 5):
        A, b = rng.normal(size=(6, nc)), rng.normal(size=6)
        assert np.abs(pc.ref_solve_svd(A, b) - np.linalg.lstsq(A, b, rcond=None)[0]).max() <= 1e-12
    A = rng.normal(size=(3, 3))
    assert np.abs(pc.ref_invert3(A) - np.linalg.inv(A)).max() <= 1e-11
    # a rank-2 matrix: cvInvert(CV_SVD) turns into the pseudo-inverse (SVBkSb drops the singular value under its threshold)
    S = np.outer([1, 2, 3], [1, 0, 1]) + np.outer([0, 1, 1], [2, 1, 0.0])
    assert np.abs(pc.ref_invert3(S) - np.linalg.pinv(S)).max() <= 1e-12
    A, b = rng.normal(size=(6, 4)), rng.normal(size=6)
    ok, x = pc.ref_qr_solve(A, b)
    assert ok and np.abs(x - np.linalg.lstsq(A, b, rcond=None)[0]).max() <= 1e-12
    # the singular branch returns with X untouched
    Z = A.copy()
    Z[:, 1] = 0.0
    ok, x = pc.ref_qr_solve(Z, b, x0=[7, 8, 9, 10])
    assert not ok and list(x) == [7, 8, 9, 10]
    M = rng.normal(size=(10, 12))
    G = pc.ref_mul_transposed(M)
    assert np.abs(G - M.T @ M).max() <= 1e-13 and pc.same(G, G.T.copy())
    # each entry is one sequential sum over the rows
    s = 0.0
    for k in range(10):
        s += M[k, 2] * M[k, 7]
    assert G[2, 7] == s


# ------------------------------------------------------------------------------------------------ the draw
def _literal_draw(n, iterations):
    """PnPsolver.cc:188-201 as written, over libc's rand()"""
    out = []
    for _ in range(iterations):
        avail = list(range(n))
        live = n
        row = []
        for _ in range(4):
            randi = int((float(libc().rand()) / (RAND_MAX + 1.0)) * live)
            idx = avail[randi]
            row.append(idx)
            avail[idx] = avail[live - 1]
            live -= 1
        out.append(row)
    return np.array(out, np.int32)


def test_draw_equals_the_literal_restatement_and_repeats_points():
    repeats = 0
    for n in (4, 5, 7, 30, 500):
        seed_rand(11)
        want = _literal_draw(n, 200)
        seed_rand(11)
        assert np.array_equal(pc.ref_draw_sets(n, 200), want)
        assert np.array_equal(make_pnp_sets(n, 200, seed=11), want)
        assert want.min() >= 0 and want.max() < n
        if n <= 7:
            repeats += sum(len(set(r)) < 4 for r in want.tolist())
    assert repeats > 0        # overwriting by VALUE lets a point come back
    seed_rand(5)
    a = random_int(10)
    seed_rand(5)
    assert a == int((float(libc().rand()) / (RAND_MAX + 1.0)) * 10)
    with pytest.raises(ValueError):
        make_pnp_sets(3, 1)


# ------------------------------------------------------------------------------------------------ SetRansacParameters
def test_set_ransac_parameters():
    for n in (20, 100, 500):
        s = pc.RefSolver(pc.family_case("general", 0, n=n))
        assert s.set_ransac(*pc.TRACKING) == 0
        assert s.max_iterations == 35 and s.min_inliers == max(10, n // 2)
    s = pc.RefSolver(pc.family_case("general", 0, n=15))
    s.set_ransac(*pc.TRACKING)
    assert s.min_inliers == 10 and s.epsilon == np.float32(10) / np.float32(15)
    s = pc.RefSolver(pc.family_case("general", 0, n=10))
    s.set_ransac(*pc.TRACKING)
    assert s.min_inliers == 10 and s.max_iterations == 1
    # int(N * epsilon) is a float product, truncated: 100 * 0.35f rounds to 35.0f (the float epsilon times 100 in binary64
    # is 34.9999994: a double product would say 34)
    s = pc.RefSolver(pc.family_case("general", 0, n=100))
    s.set_ransac(0.99, 4, 300, 4, 0.35, 5.991)
    assert int(np.float32(100) * np.float32(0.35)) == 35 and int(100 * float(np.float32(0.35))) == 34 and s.min_inliers == 35
    # the constructor's defaults
    s = pc.RefSolver(pc.family_case("general", 0, n=100))
    assert s.min_inliers == 40 and s.max_iterations == int(np.ceil(np.log(0.01) / np.log(1 - np.float64(np.float32(0.4)) ** 3)))
    # mvMaxError is a float product
    case = pc.family_case("mixed_octaves", 0)
    s = pc.RefSolver(case)
    s.set_ransac(*pc.TRACKING)
    assert pc.same(s.thresholds(), case["sigma2"] * np.float32(5.991))
    # refusals
    assert s.set_ransac(0.99, 10, 300, 5, 0.5, 5.991) == -5


def test_set_ransac_does_not_rewind():
    case = pc.family_case("wrong_60", 0)
    s = pc.ref_solve(case)
    its = s.max_iterations
    r = s.iterate(5)
    assert r["iterations"] == its and r["no_more"]
    s.set_ransac(*pc.TRACKING)
    assert s.iterations == its
    r = s.iterate(2)                       # mnIterations >= mRansacMaxIts already: the OR loop still runs nIterations
    assert r["iterations"] == its + 2


# ------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("name", sorted(pc.FAMILIES))
def test_families_against_float64_geometry(name):
    exact = pc.FAMILIES[name][1]
    hits = 0
    for seed in pc.SEEDS:
        case = pc.family_case(name, seed)
        outs = pc.replay(pc.ref_solve(case, seed=seed), 5)
        ok = [r for r in outs if r["returned"]]
        for r in ok:
            (rot, te), (outside, share, _) = pc.check64(case, r)
            assert outside == 0 and share <= pc.BAND_SHARE_CAP, (name, seed, outside, share)
            assert r["n_inliers"] == int(r["inliers"].sum())
            if exact:
                assert rot <= pc.TOL_ROT and te <= pc.TOL_T, (name, seed, rot, te)
        if exact:
            assert ok and ok[0]["refined"] and ok[0]["n_inliers"] == case["idx"].shape[0]
        if name == "wrong_60":             # never 100 inliers of 200: the exhaustive path
            assert not ok and outs[-1]["no_more"] and outs[-1]["iterations"] == 35 and outs[-1]["best_inliers"] == 0
        if name in ("wrong_20", "wrong_40", "mixed_octaves"):
            hits += bool(ok)
            assert not ok or ok[0]["n_inliers"] >= 0.9 * (1 - pc.FAMILIES[name][0].get("wrong", 0)) * case["idx"].shape[0]
        if name == "n_below_min":
            assert len(outs) == 1 and outs[0]["no_more"] and outs[0]["iterations"] == 0 and not outs[0]["inliers"].any()
        if name == "n_equal_min":          # one iteration; its count can reach N but never exceed it
            assert not any(r["refined"] for r in outs)
        if name == "behind_camera":        # no depth test: the mirrored points project onto their keypoints and count
            assert ok and ok[0]["n_inliers"] == 80
    if name in ("wrong_20", "wrong_40", "mixed_octaves"):   # (a minimal set of noisy points does not always reach min: 35 draws)
        assert hits >= len(pc.SEEDS) // 2


def test_compute_pose_on_all_points_recovers_the_pose():
    case = pc.family_case("general", 3)
    s = pc.RefSolver(case)
    err, R, t = s.compute_pose(np.arange(100))
    assert err < 1e-3 and np.abs(R - case["true"]["R"]).max() < 1e-6 and np.abs(t - case["true"]["t"]).max() < 1e-5
    # four equal points: NaN, carried through
    err, R, t = s.compute_pose([5, 5, 5, 5])
    assert np.isnan(R).all() and np.isnan(t).all()


# ------------------------------------------------------------------------------------------------ iterate
@pytest.mark.parametrize("name", ["general", "wrong_20", "wrong_40", "wrong_60", "mixed_octaves"])
def test_iterate_in_steps_equals_find_and_continuations(name):
    for seed in list(pc.SEEDS)[:4]:
        case = pc.family_case(name, seed)
        a = pc.ref_solve(case, seed=seed)
        b = pc.ref_solve(case, seed=seed)
        ra, rb = a.iterate(5), b.find()
        # the loop is an OR: the first iterate(5) runs as far as find does
        for k in pc.RESULT_INTS:
            assert ra[k] == rb[k], k
        for k in pc.RESULT_BITS:
            assert pc.same(ra[k], rb[k]), k
        assert ra["returned"] or ra["iterations"] == a.max_iterations
        # ... and continued: iterate(5) on, against find on, call by call until bNoMore or mRansacMaxIts (find asks for
        # mRansacMaxIts more each time, iterate for 5: below mRansacMaxIts both run to the next Refine return or to the end)
        while not (ra["no_more"] or ra["iterations"] >= a.max_iterations):
            ra, rb = a.iterate(5), b.find()
            if rb["rc"] == -4 or ra["iterations"] != rb["iterations"]:
                # no Refine return before mRansacMaxIts: iterate(5) ends at max(mRansacMaxIts, its + 5), find at
                # max(mRansacMaxIts, its + mRansacMaxIts) or past the sets; up to mRansacMaxIts they saw the same
                assert ra["iterations"] >= a.max_iterations and (rb["rc"] == -4 or rb["iterations"] >= b.max_iterations)
                break
            for k in pc.RESULT_INTS:
                assert ra[k] == rb[k], k
            for k in pc.RESULT_BITS:
                assert pc.same(ra[k], rb[k]), k
        # all hypotheses of the table, and the records among them
        tab = a.all_hypotheses()
        q = tab["n_inliers"] >= a.min_inliers
        best = 0
        for i in range(len(tab)):
            rec = bool(q[i] and tab["n_inliers"][i] > best)
            assert bool(tab["is_record"][i]) == rec
            if rec:
                best = tab["n_inliers"][i]
                assert bool(tab["refine_ok"][i]) == (tab["refine_inliers"][i] > a.min_inliers)
        if ra["returned"] and ra["refined"]:
            h = ra["best_hypothesis"]
            assert tab["is_record"][h] and tab["refine_inliers"][h] == ra["n_inliers"]
            assert pc.same(ra["Tcw"][:3, :3], tab["refine_R"][h].astype(np.float32)) and pc.same(ra["Tcw"][:3, 3], tab["refine_t"][h].astype(np.float32))
            assert pc.same(ra["best_Tcw"][:3, :3], tab["R"][h].astype(np.float32))


def test_or_loop_overshoot_and_capacity_boundary():
    case = pc.family_case("wrong_60", 1)
    s = pc.ref_solve(case, sets=pc.case_sets(case, 35 + 3, 1))
    r = s.iterate(1)
    assert r["iterations"] == 35 and r["no_more"] and not r["returned"]    # iterate(1) ran all of mRansacMaxIts
    r = s.iterate(3)
    assert r["iterations"] == 38 and r["no_more"]
    r = s.iterate(1)
    assert r["rc"] == -4 and s.iterations == 38                            # past the sets: refused, state untouched
    # entered at mRansacMaxIts - 1, iterate(5) evaluates hypothesis indices up to mRansacMaxIts + 3
    case = pc.family_case("wrong_20", 2)
    full = pc.ref_solve(case, seed=2)
    tab = full.all_hypotheses()
    s = pc.ref_solve(case, seed=2)
    assert len(s.sets) == s.max_iterations + EXTRA_SETS
    seen = 0
    while True:
        r = s.iterate(5)
        assert r["rc"] == 0 and r["iterations"] <= s.max_iterations + 4
        seen += 1
        if r["no_more"] or r["iterations"] >= s.max_iterations:
            break
    assert seen > 1 and len(tab) == s.max_iterations + EXTRA_SETS


def test_refine_count_below_the_best_and_refine_failure():
    """Refine's count can be smaller than the best's: the refined pose, count and mask are returned all the same when the
    count still exceeds min; points behind the camera pass CheckInliers but wreck the n-point fit, so Refine fails and the
    best comes back at exhaustion; and a Refine that ends with count == min fails as well (strict `>`)"""
    case = pc.family_case("mixed_octaves", 2, noise=1.0)
    s = pc.ref_solve(case, seed=2)
    tab = s.all_hypotheses()
    rec = tab[tab["is_record"] == 1]
    assert ((rec["refine_inliers"] < rec["n_inliers"]) & (rec["refine_ok"] == 1)).any()
    seen = False
    for r in pc.replay(s, 5):
        if r["returned"] and r["refined"] and r["n_inliers"] < r["best_inliers"]:
            assert r["n_inliers"] == int(r["inliers"].sum()) and r["n_inliers"] > s.min_inliers
            seen = True
    assert seen
    wrecked = 0
    for seed in pc.SEEDS:
        case = pc.family_case("behind_camera", seed)
        tab = pc.ref_solve(case, seed=seed).all_hypotheses()
        full = tab[(tab["is_record"] == 1) & (tab["n_inliers"] == 80)]      # a best mask that holds the mirrored points
        assert (full["refine_inliers"] < 40).all() and not full["refine_ok"].any()
        wrecked += len(full)
    assert wrecked > 0
    # n_equal_min: ten exact points, min 10: a hypothesis that counts 10 is the best, Refine counts at most 10, not > 10
    fail = 0
    for seed in pc.SEEDS:
        case = pc.family_case("n_equal_min", seed)
        s = pc.ref_solve(case, seed=seed)
        r = s.iterate(5)
        tab = s.all_hypotheses()
        if (tab["n_inliers"] >= 10).any():
            h = int(np.flatnonzero(tab["is_record"])[0])
            assert tab["refine_inliers"][h] <= 10 and not tab["refine_ok"][h]
            assert r["returned"] and not r["refined"] and r["no_more"] and r["n_inliers"] == 10 and r["hypothesis"] == r["best_hypothesis"]
            fail += 1
    assert fail > 0


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_and_library_exports_the_orbp_block():
    src = open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    assert "ORBP_MAX_POINTS 65535" in src and "ORBP_MAX_ITERATIONS 4096" in src
    declared = ref_shim.declared("orbslamm_hip.h", "orbp_")
    from orbslamm_amd import _lib
    assert len(declared) >= 8
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    import orbslamm_amd
    assert orbslamm_amd.PnPsolver is not None and orbslamm_amd.make_pnp_sets is make_pnp_sets


def test_result_structs_and_the_restatement_stands_alone():
    from orbslamm_amd.pnp import HYP_DTYPE, OrbpHypothesis, OrbpResult
    assert C.sizeof(OrbpHypothesis) == 208 == HYP_DTYPE.itemsize and C.sizeof(OrbpResult) == 160
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "pnp_ref.hpp"))
    for name in ("orbp_kernels.hip", "orbp_host.inc"):
        assert "pnp_ref.hpp" not in open(os.path.join(ROOT, "orbslamm_amd", "csrc", name)).read()


def test_dropin_header_compiles_against_the_mocks():
    """include/PnPsolver_hip.hpp instantiated on mocks derived from tests/cpp/mock_slam.hpp (the GPU test runs it)"""
    dropin.syntax_only("pnp_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "PnPsolver_hip.hpp")).read()
    for member in ("SetRansacParameters", "find(", "iterate(", "RunAll"):
        assert member in hdr, member
