"""CreateNewMapPoints without a GPU: orbl_compute_f12 (a host entry) against float64 geometry, the restatement
(tools/newpoints_ref.hpp) against a float64 recount on every scene family, the conditions that keep the GPU parity tests
from proving nothing, the exactness argument of the batch (serial loop == all neighbours independently, first success
wins), and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dropin
import newpoints_cases as nc
import ref_shim
from orbslamm_amd import local_mapping as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = np.float64


@pytest.fixture(scope="module")
def runs(oracle):
    """the serial reference of every family and seed, computed once"""
    out = {}
    for name in sorted(nc.FAMILIES):
        for seed in nc.SEEDS:
            case = nc.family_case(name, seed)
            out[(name, seed)] = (case, nc.serial_reference(oracle, case))
    return out


# ------------------------------------------------------------------------------------------------ ComputeF12 and the epipole
def _f64_f12(kf1, kf2):
    R1, R2 = kf1["Rcw"].astype(f64), kf2["Rcw"].astype(f64)
    t1, t2 = kf1["tcw"].astype(f64), kf2["tcw"].astype(f64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    def Km(k):
        k = k.astype(f64)
        return np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]])
    K1, K2 = Km(kf1["K"]), Km(kf2["K"])
    F = np.linalg.inv(K1.T) @ tx @ R12 @ np.linalg.inv(K2)
    C2 = R2 @ kf1["Ow"].astype(f64) + t2
    e = np.array([K2[0, 0] * C2[0] / C2[2] + K2[0, 2], K2[1, 1] * C2[1] / C2[2] + K2[1, 2]])
    return F, e


def test_compute_f12_against_float64_and_the_restatement():
    """The library's host entry equals the restatement's as bits, and float64 numpy to float32 rounding; the epipole is the
    float64 projection of the current camera centre.  The bounds follow the arithmetic, not the code's output: t12 = -R12 t2 +
    t1 and C2 = R2w Cw + t2w are differences of vectors of length |t| that cancel down to the baseline, so both carry an
    ABSOLUTE float32 error of a few eps (|t1| + |t2|).  F12 is linear in t12 and every entry is a sum of products bounded by
    S = |K1^-T|_inf |t12| |K2^-1|_inf (its terms may cancel below that): its error is bounded by 16 eps S (|t1| + |t2|) / |t12|,
    the three further float products adding a few eps of S.  The epipole is f C2x / C2z +
    c: its error is bounded by f (1 + |e - c| / f) * 16 eps (|R2w Cw| + |t2w|) / |C2z|."""
    eps = float(np.finfo(np.float32).eps)
    worst_f = worst_e = 0.0
    for name in ("general", "mixed_intrinsics", "short_baseline"):
        for seed in nc.SEEDS:
            case = nc.family_case(name, seed)
            kf1 = case["cur"]["kf"]
            for nb in case["nbs"]:
                kf2 = nb["kf"]
                F, e = lm.compute_f12(kf1, kf2)
                Fr, er = nc.ref_f12(kf1, kf2)
                assert nc.same(F, Fr) and nc.same(e, er)
                F6, e6 = _f64_f12(kf1, kf2)
                t1, t2 = kf1["tcw"].astype(f64), kf2["tcw"].astype(f64)
                R12 = kf1["Rcw"].astype(f64) @ kf2["Rcw"].astype(f64).T
                amp = (np.linalg.norm(t1) + np.linalg.norm(t2)) / np.linalg.norm(-R12 @ t2 + t1)
                k1, k2 = kf1["K"].astype(f64), kf2["K"].astype(f64)
                S = (1 + k1[2] / k1[0] + k1[3] / k1[1]) * np.linalg.norm(-R12 @ t2 + t1) * (1 + k2[2] / k2[0] + k2[3] / k2[1])
                worst_f = max(worst_f, float(np.abs(F - F6).max() / (S * amp * 16 * eps)))
                RC = kf2["Rcw"].astype(f64) @ kf1["Ow"].astype(f64)
                C2 = RC + t2
                f = float(kf2["K"][0])
                bound = f * (1 + np.abs(e6 - kf2["K"][2:].astype(f64)).max() / f) * 16 * eps * (np.linalg.norm(RC) + np.linalg.norm(t2)) / abs(C2[2])
                worst_e = max(worst_e, float(np.abs(e - e6).max() / bound))
    print("F12 gap / bound %.3g, epipole gap / bound %.3g" % (worst_f, worst_e))
    assert worst_f <= 1 and worst_e <= 1


def test_true_correspondences_satisfy_f12():
    """x2' F12' ... consistency: a noiseless pair of projections of one point lies on its epipolar line.  The bound is the
    residual left by F12's float32 entries, measured at its largest over the seeds used (9.36e-5 px, printed) and given the
    project's 4x margin."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for seed in nc.SEEDS:
        case = nc.family_case("general", seed)
        kf1 = case["cur"]["kf"]
        R1, O1, K1 = kf1["Rcw"].astype(f64), kf1["Ow"].astype(f64), kf1["K"].astype(f64)
        Xc = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-1.5, 1.5, 200), rng.uniform(4, 9, 200)], axis=1)
        X = Xc @ R1 + O1
        u1, v1, _ = nc._project(R1, O1, K1, X)
        for nb in case["nbs"]:
            F, _ = lm.compute_f12(kf1, nb["kf"])
            u2, v2, _ = nc._project(nb["kf"]["Rcw"].astype(f64), nb["kf"]["Ow"].astype(f64), nb["kf"]["K"].astype(f64), X)
            l = np.stack([u1, v1, np.ones_like(u1)], axis=1) @ F.astype(f64)
            d = np.abs(l[:, 0] * u2 + l[:, 1] * v2 + l[:, 2]) / np.hypot(l[:, 0], l[:, 1])
            worst = max(worst, float(d.max()))
    print("largest epipolar residual of a true pair: %.3g px" % worst)
    assert worst <= 4 * 9.36e-5


# ------------------------------------------------------------------------------------------------ the restatement against float64
@pytest.mark.parametrize("name", sorted(nc.FAMILIES))
def test_families_against_float64_geometry(runs, name):
    for seed in nc.SEEDS:
        case, (pts, status, _, m12s) = runs[(name, seed)]
        pos, outside, share, total = nc.check64(case, pts, status, m12s)
        print("%s seed %d: %d points, %d pairs, position gap %.3g, outside %d, band share %.4f" % (name, seed, len(pts), total, pos, outside, share))
        assert pos <= nc.TOL_POS, (name, seed, pos)
        assert outside == 0, (name, seed, outside)
        assert share <= nc.BAND_SHARE_CAP, (name, seed, share)
        # what UpdateNormalAndDepth leaves, recomputed in float64 from the record's own position
        kf1 = case["cur"]["kf"]
        for r in pts[:50]:
            kf2 = case["nbs"][int(r["neighbour"])]["kf"]
            X = r["pos"].astype(f64)
            n1, n2 = X - kf1["Ow"].astype(f64), X - kf2["Ow"].astype(f64)
            normal = (n1 / np.linalg.norm(n1) + n2 / np.linalg.norm(n2)) / 2
            assert np.abs(r["normal"] - normal).max() <= 4 * np.finfo(np.float32).eps
            o1 = int(case["cur"]["keys"]["octave"][int(r["idx1"])])
            mx = np.linalg.norm(n1) * f64(case["sf"][o1])
            assert abs(r["max_distance"] - mx) <= 4 * np.finfo(np.float32).eps * mx
            assert abs(r["min_distance"] - mx / f64(case["sf"][-1])) <= 4 * np.finfo(np.float32).eps * mx


# ------------------------------------------------------------------------------------------------ the conditions
def test_every_status_code_occurs(runs, oracle):
    seen = np.zeros(12, np.int64)
    for (_, _), (_, (_, status, _, _)) in runs.items():
        seen += np.bincount(status.reshape(-1), minlength=12)
    case = nc.degenerate_case()
    pts, status, _, _ = nc.serial_reference(oracle, case)
    assert status[0, 0] == lm.ST_X3D_ZERO and status[1, 1] == lm.ST_REPROJ2 and status[2, 2] == lm.ST_DIST_ZERO
    seen += np.bincount(status.reshape(-1), minlength=12)
    print(dict(zip(lm.STATUS_NAMES, seen.tolist())))
    assert (seen > 0).all(), dict(zip(lm.STATUS_NAMES, seen.tolist()))


def test_general_yields_points_and_short_baseline_skips(runs):
    for seed in nc.SEEDS:
        pts, status = runs[("general", seed)][1][:2]
        assert len(pts) >= 100 and (status == lm.ST_ACCEPTED).sum() == len(pts)
        _, status = runs[("short_baseline", seed)][1][:2]
        skipped = (status == lm.ST_NEIGHBOUR_SKIPPED).all(axis=1)
        assert skipped.sum() >= 1 and (~skipped).sum() >= 1
        assert skipped[2]                    # median_depth = -1: a negative quotient is below 0.01
        assert not (status[skipped] != lm.ST_NEIGHBOUR_SKIPPED).any()
        for name in ("wrong_matches", "low_parallax", "scale_inconsistent"):
            st = runs[(name, seed)][1][1]
            want = {"wrong_matches": (lm.ST_Z1, lm.ST_Z2, lm.ST_REPROJ1), "low_parallax": (lm.ST_PARALLAX,), "scale_inconsistent": (lm.ST_SCALE,)}[name]
            for code in want:
                assert (st == code).sum() >= 3, (name, seed, lm.STATUS_NAMES[code])


@pytest.mark.parametrize("name", sorted(nc.FAMILIES))
def test_serial_loop_equals_resolved_batch(runs, oracle, name):
    """the exactness argument, checked: all neighbours independently under the initial flags, then first success wins,
    equals the serial loop -- points as bytes and the whole status table"""
    repeated = []
    for seed in nc.SEEDS:
        case, (pts, status, _, _) = runs[(name, seed)]
        rpts, rstatus, raw = nc.resolved_reference(oracle, case)
        assert nc.same(rstatus, status), (name, seed)
        assert nc.same(rpts, pts), (name, seed)
        twice = (raw == lm.ST_ACCEPTED).sum(axis=0) >= 2
        later = (raw == lm.ST_ACCEPTED) & (status == lm.ST_FEATURE_SKIPPED)
        assert later.sum() == (raw == lm.ST_ACCEPTED).sum() - len(pts)
        repeated.append(int(twice.sum()))
    if name == "repeat_features":
        print("features accepted by two or more neighbours:", repeated)
        assert min(repeated) >= 50


def test_empty_cases_on_the_restatement(oracle):
    for kind in nc.EMPTY_KINDS:
        pts, status, _, _ = nc.serial_reference(oracle, nc.empty_case(kind))
        if kind == "no_neighbour_features":
            assert (status[0] <= lm.ST_NO_MATCH).all() and len(pts) > 0
        else:
            assert len(pts) == 0 and not (status >= lm.ST_PARALLAX).any()


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_and_library_exports_the_orbl_block():
    src = open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    assert "ORBL_MAX_NEIGHBOURS 32" in src
    for code, name in enumerate(lm.STATUS_NAMES):
        assert re.search(r"#define ORBL_ST_%s %d\b" % (name.upper(), code), src), name
    declared = ref_shim.declared("orbslamm_hip.h", "orbl_")
    from orbslamm_amd import _lib
    assert len(declared) == 3
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    import orbslamm_amd
    assert orbslamm_amd.create_new_map_points is lm.create_new_map_points and orbslamm_amd.compute_f12 is lm.compute_f12


def test_structs_and_the_restatement_stands_alone():
    assert lm.KF_DTYPE.itemsize == 80 and lm.NEWPOINT_DTYPE.itemsize == 44 and lm.MAX_NEIGHBOURS == 32
    L = nc.ref_lib()
    assert (L.npref_sizes(0), L.npref_sizes(1)) == (80, 44)
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "newpoints_ref.hpp"))
    for name in ("orbl_kernels.hip", "orbl_host.inc"):
        assert "newpoints_ref.hpp" not in open(os.path.join(ROOT, "orbslamm_amd", "csrc", name)).read()


def test_dropin_header_compiles_against_the_mocks():
    """include/LocalMapping_hip.hpp instantiated on mocks derived from tests/cpp/mock_slam.hpp (the GPU test runs it)"""
    dropin.syntax_only("newpoints_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "LocalMapping_hip.hpp")).read()
    for member in ("CreateNewMapPointsT", "GetBestCovisibilityKeyFrames", "ComputeSceneMedianDepth", "checkNewKeyFrames()"):
        assert member in hdr, member


def test_refusals_that_need_no_gpu():
    """check_ori and the argument checks come before any device work; without a GPU no matcher handle exists, so the compute
    entries cannot be reached (no CPU fallback), while orbl_compute_f12 works"""
    from orbslamm_amd import ORBmatcher, _lib
    L = _lib.lib()
    case = nc.family_case("general", 0)
    F, e = lm.compute_f12(case["cur"]["kf"], case["nbs"][0]["kf"])
    assert np.isfinite(F).all() and np.isfinite(e).all()
    n_new = C.c_int(7)
    sf, kf = case["sf"], np.ascontiguousarray(case["cur"]["kf"], dtype=lm.KF_DTYPE)
    args = [None, None, kf.ctypes.data, None, None, None, 0, sf.ctypes.data, sf.ctypes.data, 8, C.c_float(1.2)]
    assert L.orbl_create_new_map_points_frames(None, *args, 1, None, 0, C.byref(n_new), None, None) == _lib.ORBX_E_UNSUPPORTED
    assert b"histogram" in L.orbx_last_error() and n_new.value == 0
    assert L.orbl_create_new_map_points_frames(None, *args, 0, None, 0, C.byref(n_new), None, None) == _lib.ORBX_E_INVALID   # null handle
    args[6] = 33
    assert L.orbl_create_new_map_points_frames(None, *args, 0, None, 0, C.byref(n_new), None, None) == _lib.ORBX_E_UNSUPPORTED
    if L.orbx_device_count() == 0:
        with pytest.raises(_lib.OrbError) as ei:
            ORBmatcher(0.6, False, device=0)
        assert ei.value.code == _lib.ORBX_E_NO_DEVICE
