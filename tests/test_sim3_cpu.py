"""The Sim3Solver's contract on the CPU: the restatement's cv::eigen (JacobiImpl_<float>) against numpy.linalg.eigh and its
cv::Rodrigues against a float64 formula, the set draw against a literal restatement of Sim3Solver.cc:163-177 over libc's
rand() (repeated points included), the size_t thresholds, the scene families against float64 geometry, iterate's replay,
and the orbs_* block of the header declared and exported by the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import dropin
import ref_shim
import sim3_cases as sc
from orbslamm_amd.sim3 import make_sim3_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ OpenCV pieces
def _check_eigen(a):
    w, v = sc.ref_eigen(a)
    a64 = a.astype(np.float64)
    ws = np.linalg.eigh(a64)[0][::-1]
    scale = max(float(np.abs(ws).max()), 1e-30)
    assert np.all(np.diff(w.astype(np.float64)) <= 0), w                      # descending
    assert np.allclose(w, ws, rtol=0, atol=3e-6 * scale), (w, ws)
    v64 = v.astype(np.float64)
    assert np.allclose(v64 @ v64.T, np.eye(4), atol=3e-6)                     # orthonormal ROWS
    for k in range(4):
        assert np.abs(a64 @ v64[k] - float(w[k]) * v64[k]).max() < 1e-5 * scale, k


def _sym(rng):
    m = rng.normal(0, 1, (4, 4))
    return ((m + m.T) / 2).astype(np.float32)


def test_restated_eigen_against_numpy():
    rng = np.random.default_rng(4)
    for trial in range(40):
        a = _sym(rng)
        if trial % 4 == 1:   # rank deficient: u u^T + v v^T
            u, v = rng.normal(0, 1, 4), rng.normal(0, 1, 4)
            a = (np.outer(u, u) - np.outer(v, v)).astype(np.float32)
            a = ((a + a.T) / 2).astype(np.float32)
        if trial % 4 == 2:   # diagonal, unsorted
            a = np.diag(rng.normal(0, 1, 4)).astype(np.float32)
        if trial % 4 == 3:   # Horn's N of a real hypothesis: traceless
            a = (a - np.eye(4, dtype=np.float32) * np.float32(np.trace(a) / 4)).astype(np.float32)
            a = ((a + a.T) / 2).astype(np.float32)
        _check_eigen(a)
    w, v = sc.ref_eigen(np.zeros((4, 4), np.float32))
    assert not w.any() and np.array_equal(v, np.eye(4, dtype=np.float32))     # no rotation: V stays the identity
    w, v = sc.ref_eigen(np.diag(np.array([1, 3, 2, 4], np.float32)))
    assert list(w) == [4, 3, 2, 1] and np.array_equal(v, np.eye(4, dtype=np.float32)[[3, 1, 2, 0]])   # rows swapped with the values


def test_restated_eigen_reads_the_upper_triangle_only():
    rng = np.random.default_rng(6)
    a = _sym(rng)
    b = a.copy()
    b[np.tril_indices(4, -1)] = 77.0
    wa, va = sc.ref_eigen(a)
    wb, vb = sc.ref_eigen(b)
    assert sc.same(wa, wb) and sc.same(va, vb)


def _rodrigues64(v):
    v = v.astype(np.float64)
    th = np.sqrt((v * v).sum())
    if th < np.finfo(np.float64).eps:
        return np.eye(3)
    return sc.rot_axis_angle(v / th, th)


def test_restated_rodrigues_against_float64():
    rng = np.random.default_rng(8)
    for trial in range(50):
        axis = rng.normal(0, 1, 3)
        axis /= np.linalg.norm(axis)
        th = [rng.uniform(0, np.pi), 1e-5, np.pi - 1e-6, np.pi, 1e-9, 2.5][trial % 6]
        v = (axis * th).astype(np.float32)
        R = sc.ref_rodrigues(v)
        assert R.dtype == np.float32
        assert np.abs(R.astype(np.float64) - _rodrigues64(v)).max() < 1e-7
    # theta below DBL_EPSILON (also exactly zero) is the identity, exactly; just above it is not special-cased
    for v in ([0, 0, 0], [1e-17, 0, 0], [1e-17, -1e-17, 1e-17]):
        assert np.array_equal(sc.ref_rodrigues(np.array(v, np.float32)), np.eye(3, dtype=np.float32))
    R = sc.ref_rodrigues(np.array([1e-3, 0, 0], np.float32))
    assert R[1, 2] != 0 and R[1, 2] == np.float32(-np.sin(np.float64(np.float32(1e-3))))
    # a NaN vector gives a NaN matrix (theta < DBL_EPSILON is false for NaN)
    assert np.isnan(sc.ref_rodrigues(np.array([np.nan, 0, 0], np.float32))).all()


# ------------------------------------------------------------------------------------------------ the draw
def _literal_draw(n, iterations, libc):
    """Sim3Solver.cc:163-177 as written: a Python list stands for vAvailableIndices; the write at [idx] may land one
    past the live part, which a list emulates with a spare slot"""
    sets = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(n)) + [None]
        size = n
        for i in range(3):
            d = (size - 1) - 0 + 1
            randi = int((float(libc.rand()) / (2147483647 + 1.0)) * d) + 0
            idx = avail[randi]
            sets[it, i] = idx
            avail[idx] = avail[size - 1]      # vAvailableIndices[idx] = vAvailableIndices.back()
            size -= 1                         # pop_back
    return sets


@pytest.mark.parametrize("n", [3, 4, 10, 20, 100])
def test_set_draw_is_the_references_with_its_repeated_points(n):
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    iterations = 4000
    libc.srand(n)
    want = _literal_draw(n, iterations, libc)
    got = make_sim3_sets(n, iterations, seed=n)
    assert np.array_equal(got, want)
    libc.srand(n)
    assert np.array_equal(sc.ref_draw_sets(n, iterations), want)
    assert want.min() >= 0 and want.max() < n
    rep = (want[:, 0] == want[:, 1]) | (want[:, 0] == want[:, 2]) | (want[:, 1] == want[:, 2])
    if n <= 10:
        # the trap: idx is the drawn value, not the drawn position -- a "corrected" draw never repeats a point
        assert rep.any(), "no repeated point in %d sets of %d" % (iterations, n)
    assert not (want[:, 0] == want[:, 1]).all()
    # the first draw of a set is uniform over all n
    assert len(np.unique(want[:, 0])) == n


def test_make_sim3_sets_continues_the_stream_and_refuses_two_points():
    libc = C.CDLL(None)
    libc.srand(0)
    a = make_sim3_sets(30, 2, seed=None)
    assert np.array_equal(a, make_sim3_sets(30, 2, seed=0))
    with pytest.raises(ValueError):
        make_sim3_sets(2, 1)


# ------------------------------------------------------------------------------------------------ thresholds, parameters
def test_thresholds_are_truncated_to_size_t():
    """mvnMaxError1/2 are vector<size_t>: (size_t)(9.210 * sigma2) for the eight levels' mvLevelSigma2 at scale 1.2"""
    rng = np.random.default_rng(0)
    case = sc.make_case(rng, n=8)
    case["sigma2_1"] = sc.SIGMA2.copy()
    case["sigma2_2"] = sc.SIGMA2[::-1].copy()
    e1, e2 = sc.RefSolver(case).thresholds()
    want = [9, 13, 19, 27, 39, 57, 82, 118]
    assert [int(9.210 * float(s2)) for s2 in sc.SIGMA2] == want
    assert list(e1) == want and list(e2) == want[::-1]
    assert e1.dtype == np.float32 and e1[0] == 9.0      # level 0 gives 9, not 9.21


def test_threshold_truncation_decides_an_inlier():
    """a point whose error lies between 9 and 9.21 at level 0 is an outlier: identity Sim3 (fixed scale, three exact
    points) and a fourth point displaced by 3.02 pixels in image 1"""
    f = np.float32
    K = np.array([500, 500, 320, 240], f)
    X = np.array([[0, 0, 4], [1, 0, 4], [0, 1, 4], [0.5, 0.5, 4], [0.25, 0.75, 4]], f)
    R = sc.rot_axis_angle([0, 0, 1], 0.5)
    X2 = (X.astype(np.float64) @ R).astype(f)            # X1 = R X2
    X1 = X.copy()
    X1[3, 0] += f(3.02 * 4 / 500)                        # err1 = 3.02^2 = 9.12: inside 9.21, outside 9
    X1[4, 0] += f(2.9 * 4 / 500)                         # err1 = 8.41: inside both
    case = dict(n1=5, idx1=np.arange(5, dtype=np.int32), X1w=X1, X2w=X2, Rcw1=np.eye(3, dtype=f).reshape(9), tcw1=np.zeros(3, f),
                Rcw2=np.eye(3, dtype=f).reshape(9), tcw2=np.zeros(3, f), K1=K, K2=K, sigma2_1=np.ones(5, f), sigma2_2=np.ones(5, f),
                fix_scale=True, ransac=(0.99, 3, 300))
    s = sc.RefSolver(case)
    s.set_ransac(0.99, 3, 300)
    s.use_sets(np.tile(np.array([[0, 1, 2]], np.int32), (s.max_iterations, 1)))
    r = s.find()
    assert r["returned"] and r["n_inliers"] == 4
    assert list(r["inliers"]) == [True, True, True, False, True]


def test_set_ransac_parameters():
    rng = np.random.default_rng(0)

    def its(n, *params):
        s = sc.RefSolver(sc.make_case(rng, n=n))
        s.set_ransac(*params)
        return s.max_iterations
    assert its(20, 0.99, 10, 300) == 35 and its(100, 0.99, 10, 300) == 300
    assert sc.RefSolver(sc.make_case(rng, n=50)).max_iterations == 300     # the constructor's (0.99, 6, 300)
    assert its(10, 0.99, 10, 300) == 1                                     # mRansacMinInliers == N
    assert its(5, 0.99, 6, 300) == 1                                       # epsilon above 1: log of a negative -> max(1, .)
    assert its(100, 0.99, 10, 50) == 50
    # epsilon is a FLOAT: ceil(log(0.01) / log(1 - pow((double)(float)(min/N), 3)))
    n, m = 37, 11
    eps = np.float32(m) / np.float32(n)
    assert its(n, 0.99, m, 100000) == int(np.ceil(np.log(1 - 0.99) / np.log(1 - float(eps) ** 3)))


# ------------------------------------------------------------------------------------------------ families
def _replay(case, seed, step=None):
    s = sc.ref_solve(case, seed=seed)
    outs = []
    while True:
        r = s.iterate(s.max_iterations if step is None else step)
        outs.append(r)
        if r["no_more"]:
            return s, outs


@pytest.mark.parametrize("name", [n for n, (_, noiseless, _) in sc.FAMILIES.items() if noiseless])
def test_noiseless_families_recover_the_true_sim3(name):
    for seed in sc.SEEDS:
        case = sc.family_case(name, seed)
        r = sc.ref_solve(case, seed=seed).find()
        assert r["returned"] and r["n_inliers"] > case["ransac"][1]
        (rot, dt, ds), (outside, share, worst) = sc.check64(case, r)
        print("%s seed %d: rot %.3e t %.3e s %.3e band share %.4f" % (name, seed, rot, dt, ds, share))
        assert rot <= sc.TOL_ROT and dt <= sc.TOL_T and ds <= sc.TOL_S, (rot, dt, ds)
        assert outside == 0 and share <= sc.BAND_SHARE_CAP
        assert r["inliers"].sum() == r["n_inliers"] or share > 0
        if case["fix_scale"]:
            assert r["best_s"] == np.float32(1.0)


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_returned_masks_agree_with_a_float64_recount(name):
    """every return of an iterate-to-exhaustion replay: the mask equals the float64 recount under the returned T12 except
    inside the float32 rounding band of a threshold, and at most 2 % of a case's points are inside it"""
    for seed in sc.SEEDS:
        case = sc.family_case(name, seed)
        s, outs = _replay(case, seed)
        for r in outs:
            if not r["returned"]:
                continue
            _, (outside, share, worst) = sc.check64(case, r)
            assert outside == 0, (name, seed, r["hypothesis"], worst)
            assert share <= sc.BAND_SHARE_CAP, (name, seed, share)
            # vbInliers has mN1 entries indexed by mvnIndices1
            assert r["inliers"].shape[0] == case["n1"] and not np.delete(r["inliers"], case["idx1"]).any()
            assert r["inliers"].sum() == r["n_inliers"]


def test_outlier_families_find_the_true_inliers():
    for name, good in (("outliers_30", 0.7), ("outliers_60", 0.4)):
        for seed in sc.SEEDS:
            case = sc.family_case(name, seed)
            s, outs = _replay(case, seed)
            best = max(r["n_inliers"] for r in outs)
            assert best >= 0.9 * good * 200, (name, seed, best)


def test_quirk_families_do_what_the_restatement_does():
    # identity rotation: X2c == X1c exactly -> M symmetric -> the quaternion is exactly (1, 0, 0, 0) -> 0 * inf = NaN
    for seed in sc.SEEDS:
        case = sc.family_case("identity_rotation", seed)
        s, outs = _replay(case, seed)
        tab = s.all_hypotheses()
        assert len(outs) == 1 and not outs[0]["returned"] and outs[0]["no_more"]
        nan = np.isnan(tab["s12"])
        # (an occasional near-collinear set ties N's two largest eigenvalues and rounding picks the other vector: finite)
        assert nan.sum() >= len(tab) - 2 and np.isnan(tab["R12"][nan]).all() and not tab["n_inliers"][nan].any()
        # zero inliers still pass `>= mnBestInliers` while the best is 0: the stored best is a NaN matrix
        assert outs[0]["has_best"] and outs[0]["best_inliers"] == tab["n_inliers"].max()
        last = np.flatnonzero(tab["n_inliers"] == tab["n_inliers"].max())[-1]
        assert sc.same(outs[0]["best_R"], tab["R12"][last]) and (not nan[last] or np.isnan(outs[0]["best_R"]).all())
        assert any(np.isnan(r["best_R"]).all() for r in _replay(case, seed, step=1)[1])
    # N below min_inliers: bNoMore at once, nothing drawn, nothing stored
    case = sc.family_case("n_below_min", 0)
    r = sc.ref_solve(case).iterate(5)
    assert r["no_more"] and not r["returned"] and r["iterations"] == 0 and not r["has_best"]
    # N equal to min_inliers: one iteration, whose count can reach N but never exceed min_inliers -> never returned
    case = sc.family_case("n_equal_min", 0)
    s = sc.ref_solve(case)
    assert s.max_iterations == 1
    r = s.find()
    assert not r["returned"] and r["no_more"] and r["has_best"] and r["best_inliers"] == 10 and r["iterations"] == 1
    # collinear points: the rotation about the line is free; whatever the restatement returns maps the line onto itself
    case = sc.family_case("collinear", 0)
    r = sc.ref_solve(case).find()
    assert r["returned"] and r["n_inliers"] == 60


def test_repeated_points_go_through_compute_sim3():
    """a set with a point twice is two distinct points (a rank-1 M): finite or not, it is what IEEE gives; three equal
    points give NaN, zero inliers and `>=` still stores them while the best is 0"""
    case = sc.family_case("general", 0)
    s = sc.RefSolver(case)
    s.set_ransac(0.99, 10, 4)
    s.use_sets(np.array([[5, 5, 5], [3, 3, 9], [9, 3, 3], [1, 2, 3]], np.int32))
    r = s.iterate(1)
    assert not r["returned"] and r["has_best"] and r["best_inliers"] == 0 and np.isnan(r["best_R"]).all() and np.isnan(r["best_s"])
    r = s.iterate(10)
    assert r["returned"] and r["hypothesis"] == 3 and r["n_inliers"] == 100
    tab = s.table
    assert np.isnan(tab["T12"][0][:3]).all() and tab["n_inliers"][0] == 0
    assert tab["n_inliers"][1] < 100 and tab["n_inliers"][2] < 100     # a two-point fit does not explain the scene
    X = (case["X1w"].astype(np.float64) @ case["Rcw1"].astype(np.float64).reshape(3, 3).T + case["tcw1"]).astype(np.float32)
    P = X[[5, 5, 5]].T
    assert np.isnan(sc.ref_compute(P, P, False)["R"]).all()


def test_fixed_and_free_scale():
    case = sc.family_case("general", 0)
    X1 = np.array([[0, 0, 4], [1, 0, 5], [0, 1, 6]], np.float32).T
    X2 = (sc.rot_axis_angle([0.2, 1, 0.1], 0.4).T @ X1.astype(np.float64) * 0.5).astype(np.float32)   # X1 = 2 R X2
    free, fixed = sc.ref_compute(X1, X2, False), sc.ref_compute(X1, X2, True)
    assert fixed["s"] == np.float32(1.0) and abs(float(free["s"]) - 2.0) < 1e-6
    assert sc.same(free["R"], fixed["R"]) and not sc.same(free["t"], fixed["t"])
    assert case["fix_scale"] is False


# ------------------------------------------------------------------------------------------------ iterate
@pytest.mark.parametrize("name", ["general", "outliers_30", "outliers_60", "behind_camera"])
def test_iterate_in_steps_equals_find(name):
    """iterate(5) repeated to exhaustion returns, first, what one find on a fresh solver returns; later successes are
    possible (the best is replaced on >=) and equal the continued find's"""
    for seed in list(sc.SEEDS)[:4]:
        case = sc.family_case(name, seed)
        _, by5 = _replay(case, seed, step=5)
        _, whole = _replay(case, seed)
        ok5 = [r for r in by5 if r["returned"]]
        okw = [r for r in whole if r["returned"]]
        assert len(ok5) == len(okw) >= 1
        if name != "general":
            assert len(okw) >= 2, "no second success"
        for a, b in zip(ok5, okw):
            for k in ("hypothesis", "n_inliers", "best_inliers"):
                assert a[k] == b[k], k
            for k in ("T12", "best_R", "best_t", "best_s", "inliers"):
                assert sc.same(a[k], b[k]), k
        assert [r["hypothesis"] for r in okw] == sorted(r["hypothesis"] for r in okw)
        assert all(x["n_inliers"] <= y["n_inliers"] for x, y in zip(okw, okw[1:]))
        assert by5[-1]["no_more"] and all(not r["no_more"] for r in by5[:-1])
        assert all(r["iterations"] <= 5 * (i + 1) for i, r in enumerate(by5))


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_and_library_exports_the_orbs_block():
    src = open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    assert "ORBS_MAX_POINTS 65535" in src and "ORBS_MAX_ITERATIONS 4096" in src
    declared = ref_shim.declared("orbslamm_hip.h", "orbs_")
    from orbslamm_amd import _lib
    assert len(declared) >= 6
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name


def test_result_structs_match_the_restatement():
    from orbslamm_amd.sim3 import HYP_DTYPE, OrbsHypothesis, OrbsResult
    assert C.sizeof(OrbsHypothesis) == 120 == HYP_DTYPE.itemsize and C.sizeof(OrbsResult) == 36 * 4
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "sim3_ref.hpp"))


def test_dropin_header_compiles_against_the_mocks():
    """include/Sim3Solver_hip.hpp instantiated on tests/cpp/mock_slam.hpp's KeyFrame / MapPoint (the GPU test runs it)"""
    dropin.syntax_only("sim3_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "Sim3Solver_hip.hpp")).read()
    for member in ("SetRansacParameters", "find(", "iterate(", "GetEstimatedRotation", "GetEstimatedTranslation", "GetEstimatedScale", "RunAll"):
        assert member in hdr, member
