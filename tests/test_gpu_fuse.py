"""The device SearchInNeighbors (orbl_fuse_batch*, k_fuse_batch) against the per-target reference (the restatement's
projection tools/fuse_ref.hpp, then the oracle's window_best with the chi-square gate: tests/fuse_cases.py) as bits: every
field of every OrblFuseResult, over the scene families, both entries (host arrays, device-resident frames), 25 targets x
2000 points, a target above 8192 features, the job counts around the tile sizes, repeated host arrays, the empty cases and
the refusals; against the library's own window_best fed with
the restatement's projections; and the C++ drop-in on mock keyframes."""
import ctypes as C

import numpy as np
import pytest

import dropin
import fuse_cases as fc
from orbslamm_amd import local_mapping as lm
from orbslamm_amd._lib import KP_DTYPE, OrbmGrid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.6, False, device=0)


@pytest.fixture(scope="module")
def breaks():
    return lm.level_breaks(fc.LOG_SF, fc.NLEVELS)


@pytest.fixture(scope="module")
def gex(gpu):
    """an extractor handle whose device buffers carry the keys and descriptors the frames are built from"""
    from orbslamm_amd import ORBextractor
    g = ORBextractor(500, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1, device=0)
    yield g
    g.close()


def run_host(matcher, case, breaks, **kw):
    return lm.fuse_batch(matcher, case["targets"], case["points"], case["jobs"], case["sf"], case["inv_sigma2"], breaks, th=case["th"], **kw)


class _Frames:
    """the targets of a case as device-resident frames (zero distortion: mvKeysUn = mvKeys); a keyframe listed twice is built once"""

    def __init__(self, matcher, gex, case):
        self.m, self.gex, self.frames, self.targets = matcher, gex, [], []
        self.mark = len(gex._dev_bufs)
        built = {}
        for t in case["targets"]:
            if id(t["keys"]) not in built:
                n = len(t["keys"])
                pad = np.zeros((1, 1, 64), np.uint8)            # (a frame without features still gets real addresses)
                dk = gex.upload_frames(np.ascontiguousarray(t["keys"]).view(np.uint8).reshape(1, 1, -1) if n else pad)[0]
                dd = gex.upload_frames(np.ascontiguousarray(t["desc"]).reshape(1, 1, -1) if n else pad)[0]
                g = t["rec"]["grid"]
                grid = OrbmGrid(float(g["minX"]), float(g["minY"]), float(g["invW"]), float(g["invH"]), int(g["cols"]), int(g["rows"]))
                built[id(t["keys"])] = matcher.frame_from_device(dk, dd, n, t["rec"]["K"], [0, 0, 0, 0, 0], grid)
                self.frames.append(built[id(t["keys"])])
            self.targets.append(dict(rec=t["rec"], frame=built[id(t["keys"])]))

    def run(self, case, breaks):
        return lm.fuse_batch(self.m, self.targets, case["points"], case["jobs"], case["sf"], case["inv_sigma2"], breaks, th=case["th"])

    def close(self):
        from orbslamm_amd._lib import check
        for F in self.frames:
            self.m.frame_destroy(F)
        for d in self.gex._dev_bufs[self.mark:]:   # (every call that read the buffers has returned)
            check(self.gex._L.orbx_device_free(self.gex._h, d))
        del self.gex._dev_bufs[self.mark:]


def assert_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])
        raise AssertionError((what, len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:4]]))


def both_entries(matcher, gex, oracle, case, breaks, what):
    want = fc.reference(oracle, case)
    got = run_host(matcher, case, breaks)
    assert_equal(got, want, what + " (host arrays)")
    fr = _Frames(matcher, gex, case)
    try:
        assert_equal(fr.run(case, breaks), want, what + " (frames)")
    finally:
        fr.close()
    return got


@pytest.mark.parametrize("name", sorted(fc.FAMILIES))
def test_families_bit_exact(matcher, gex, oracle, breaks, name):
    codes = np.zeros(7, np.int64)
    for seed in fc.SEEDS:
        case = fc.family_case(name, seed)
        got = both_entries(matcher, gex, oracle, case, breaks, "%s seed %d" % (name, seed))
        codes += np.bincount(got["status"], minlength=7)
        if seed == 0:   # the same call again: identical bytes (the kernel holds no atomics)
            assert run_host(matcher, case, breaks).tobytes() == got.tobytes()
    print(name, dict(zip(lm.FUSE_STATUS_NAMES, codes.tolist())))
    assert codes[lm.FUSE_ST_FOUND] >= fc.FOUND_FLOOR[name], (name, codes.tolist())
    if name in fc.FAMILY_CODES:
        assert codes[fc.FAMILY_CODES[name]] > 0, (name, lm.FUSE_STATUS_NAMES[fc.FAMILY_CODES[name]])


def test_25_targets_of_2000_points(matcher, gex, oracle, breaks):
    case = fc.make_case(2500, targets=(25, 25), points=(2000, 2000), feats=2000, all_points=True, repeat=True)
    assert len(case["targets"]) == 27 and case["jobs"][0][-1] == 27 * 2000 and min(len(t["keys"]) for t in case["targets"]) >= 2000
    got = both_entries(matcher, gex, oracle, case, breaks, "25 x 2000")
    assert (got["status"] == lm.FUSE_ST_FOUND).sum() >= 10000


def test_target_above_8192_features(matcher, gex, oracle, breaks):
    case = fc.make_case(8193, targets=(2, 2), points=(12000, 12000), feats=9000, vis=1.0, spread=0.0)
    assert max(len(t["keys"]) for t in case["targets"]) > 8192
    got = both_entries(matcher, gex, oracle, case, breaks, "> 8192 features")
    assert (got["status"] == lm.FUSE_ST_FOUND).sum() >= 4000


@pytest.fixture(scope="module")
def pool():
    """three targets against 300 points, every point listed for every target: the job lists around the tile sizes are cut from it"""
    return fc.make_case(5300, targets=(3, 3), points=(300, 300), feats=500, all_points=True)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_job_counts_around_the_tile_sizes(matcher, gex, oracle, breaks, pool, n):
    """one below, at and one above every tile of job entries the kernel can be built with (32, 64, 128, 256: the tile in use is
    among them); the targets hold n, 1 and n + 1 entries, so a tile's edge also falls between two targets.  The first target
    takes the head of the pool, the last its tail."""
    P = len(pool["points"])
    idx = [np.arange(n), np.arange(1), np.arange(P - (n + 1), P)]
    case = dict(pool, jobs=(np.cumsum([0] + [len(i) for i in idx]).astype(np.int32), np.concatenate(idx).astype(np.int32)))
    got = both_entries(matcher, gex, oracle, case, breaks, "%d, 1 and %d job entries" % (n, n + 1))
    assert len(got) == 2 * n + 2
    if n >= 31:   # (the walk ran: by the reference on the CPU about 0.9 n of these entries end FOUND; the floor is half of that)
        assert (got["status"] == lm.FUSE_ST_FOUND).sum() >= n // 2


def test_repeated_host_arrays_ride_once(matcher, oracle, breaks, pool):
    """two targets that name the SAME keys / desc arrays under different poses share one copy and one grid in the staging block;
    a third that names them under another grid (80 x 60 cells) gets a grid of its own.  Every result equals the call made with
    separate copies of the arrays, and the reference."""
    t0, t1 = pool["targets"][0], pool["targets"][1]
    fine = t0["rec"].copy()
    fine["grid"] = np.array(fc.grid_tuple(80, 60), dtype=lm.GRID_DTYPE)
    shared = [t0, dict(t0, rec=t1["rec"]), dict(t0, rec=fine)]
    assert all(t["keys"] is t0["keys"] and t["desc"] is t0["desc"] for t in shared)
    apart = [dict(t, keys=t["keys"].copy(), desc=t["desc"].copy()) for t in shared]
    got = run_host(matcher, dict(pool, targets=shared), breaks)
    assert_equal(got, run_host(matcher, dict(pool, targets=apart), breaks), "shared arrays against separate copies")
    assert_equal(got, fc.reference(oracle, dict(pool, targets=shared)), "shared arrays")
    P = len(pool["points"])
    assert all((got[k * P:(k + 1) * P]["status"] == lm.FUSE_ST_FOUND).sum() >= 50 for k in (0, 2))


def test_equals_window_best_fed_with_the_restatements_projections(matcher, breaks):
    """pair for pair what ORBmatcherT::Fuse's device call returns: orbm_window_best (chi2) on the restatement's (u, v, radius, level)"""
    from orbslamm_amd import make_grid
    for name, seed in (("general", 1), ("crowded_ties", 2), ("chi2_edge", 3)):
        case = fc.family_case(name, seed)
        got = run_host(matcher, case, breaks)
        js, jp = case["jobs"]
        for k, t in enumerate(case["targets"]):
            idx = jp[js[k]:js[k + 1]]
            res, _ = fc.ref_project(case, k, idx)
            rows, uvr, pred, qd = fc.window_queries(case, res, idx)
            bi, bd = matcher.window_best(uvr, pred, qd, None, make_grid(0.0, 0.0, fc.W, fc.H), t["keys"], t["desc"], case["inv_sigma2"], chi2=True)
            mine = got[js[k]:js[k + 1]]
            assert fc.same(mine["u"], res["u"]) and fc.same(mine["v"], res["v"]) and fc.same(mine["level"], res["level"])
            assert np.array_equal((mine["status"] >= lm.FUSE_ST_NO_CANDIDATE), res["status"] == lm.FUSE_ST_NO_CANDIDATE)
            assert np.array_equal(mine["best_idx"][rows], bi) and np.array_equal(mine["best_dist"][rows], bd), (name, k)


def test_empty_cases_and_non_finite_records(matcher, gex, oracle, breaks):
    case = fc.family_case("general", 2)
    T = len(case["targets"])
    # zero targets; zero jobs; nothing is written and nothing fails
    assert len(lm.fuse_batch(matcher, [], case["points"], (np.zeros(1, np.int32), np.zeros(0, np.int32)), case["sf"], case["inv_sigma2"], breaks)) == 0
    assert len(run_host(matcher, dict(case, jobs=(np.zeros(T + 1, np.int32), np.zeros(0, np.int32))), breaks)) == 0
    # a target without features: NO_CANDIDATE for every pair that passes the projection gates; a target without jobs
    bare = dict(case["targets"][1], keys=case["targets"][1]["keys"][:0], desc=case["targets"][1]["desc"][:0])
    js, jp = case["jobs"]
    keep = np.r_[0:js[2], js[3]:js[T]]
    shift = js.copy()
    shift[3:] -= js[3] - js[2]
    case2 = dict(case, targets=[case["targets"][0], bare] + case["targets"][2:], jobs=(shift, jp[keep]))
    got = both_entries(matcher, gex, oracle, case2, breaks, "bare target, target without jobs")
    mid = got[js[1]:js[2]]
    assert (mid["status"] <= lm.FUSE_ST_NO_CANDIDATE).all() and (mid["status"] == lm.FUSE_ST_NO_CANDIDATE).sum() > 50
    # a NaN maximum distance passes the distance gate and ends at LEVEL_RANGE below; dist3D == 0 (a record whose Ow is the
    # point itself, with no minimum distance) gives an infinite ratio: above
    case3 = fc.family_case("general", 3)
    first = fc.ref_project(case3, 0, np.arange(len(case3["points"])))[0]
    i = int(np.flatnonzero(first["status"] == lm.FUSE_ST_NO_CANDIDATE)[20])
    rec = case3["targets"][0]["rec"].copy()
    rec["Ow"] = case3["points"]["pos"][i]
    case3["targets"][0] = dict(case3["targets"][0], rec=rec)
    case3["points"]["min_distance"][i] = 0.0
    case3["points"]["max_distance"][:9] = np.nan
    got = both_entries(matcher, gex, oracle, case3, breaks, "non-finite ratios")
    hit = got[np.isin(case3["jobs"][1], np.arange(9)) & (got["status"] == lm.FUSE_ST_LEVEL_RANGE)]
    assert len(hit) and (hit["level"] == -1).all()
    assert case3["jobs"][1][i] == i and got[i]["status"] == lm.FUSE_ST_LEVEL_RANGE and got[i]["level"] == fc.NLEVELS


def test_refusals(matcher, gex, oracle, breaks):
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError

    def code(fn):
        with pytest.raises(OrbError) as ei:
            fn()
        return ei.value.code

    case = fc.family_case("general", 0)
    want = fc.reference(oracle, case)
    js, jp = case["jobs"]
    T, P = len(case["targets"]), len(case["points"])
    jobs = lambda s, p: dict(case, jobs=(np.asarray(s, np.int32), np.asarray(p, np.int32)))
    for bad in (P, -1):                                   # a job index outside the pool
        p = jp.copy()
        p[len(p) // 2] = bad
        assert code(lambda: run_host(matcher, jobs(js, p), breaks)) == ORBX_E_INVALID
    s = js.copy()
    s[1], s[2] = js[2], js[1]                            # a job_start that descends
    assert code(lambda: run_host(matcher, jobs(s, jp), breaks)) == ORBX_E_INVALID
    s = js.copy()
    s[0] = 1                                             # ... that does not start at 0
    assert code(lambda: run_host(matcher, jobs(s, jp), breaks)) == ORBX_E_INVALID
    for b in (breaks[::-1], np.r_[breaks[:3], breaks[2], breaks[4:]], np.r_[breaks[:3], np.nan, breaks[4:]]):   # a break table that does not ascend
        assert code(lambda: run_host(matcher, case, b.astype(np.float32))) == ORBX_E_INVALID
    many = dict(case, targets=[case["targets"][0]] * (lm.FUSE_MAX_TARGETS + 1), jobs=(np.zeros(lm.FUSE_MAX_TARGETS + 2, np.int32), jp[:0]))
    assert code(lambda: run_host(matcher, many, breaks)) == ORBX_E_UNSUPPORTED
    s = np.zeros(T + 1, np.int32)
    s[1:] = lm.FUSE_MAX_JOBS + 1                          # more job entries than a call takes
    assert code(lambda: run_host(matcher, jobs(s, np.zeros(lm.FUSE_MAX_JOBS + 1, np.int32)), breaks)) == ORBX_E_UNSUPPORTED
    big = dict(case["targets"][0], keys=np.zeros(65536, KP_DTYPE), desc=np.zeros((65536, 32), np.uint8))
    assert code(lambda: run_host(matcher, dict(case, targets=[big] + case["targets"][1:]), breaks)) == ORBX_E_INVALID
    rec = case["targets"][0]["rec"].copy()
    rec["grid"]["cols"] = 0                               # a bad grid
    assert code(lambda: run_host(matcher, dict(case, targets=[dict(case["targets"][0], rec=rec)] + case["targets"][1:]), breaks)) == ORBX_E_INVALID
    assert code(lambda: lm.fuse_batch(matcher, case["targets"], case["points"], case["jobs"], case["sf"][:0], case["inv_sigma2"][:0], breaks[:1])) == ORBX_E_INVALID
    fr = _Frames(matcher, gex, case)
    try:
        null = [dict(rec=t["rec"], frame=C.c_void_p(None)) for t in fr.targets[:1]] + fr.targets[1:]
        assert code(lambda: lm.fuse_batch(matcher, null, case["points"], case["jobs"], case["sf"], case["inv_sigma2"], breaks)) == ORBX_E_INVALID
        # after the refusals the next good call is still exact, by both entries
        assert_equal(fr.run(case, breaks), want, "frames after the refusals")
    finally:
        fr.close()
    assert_equal(run_host(matcher, case, breaks), want, "host arrays after the refusals")


def test_fuse_dropin_on_mock_keyframes(gpu, oracle, tmp_path):
    """include/LocalMapping_hip.hpp (SearchInNeighborsT) on mock keyframes and map points (tests/cpp/fuse_dropin_gpu.cpp): the
    replay leaves the object graph and the Replace / AddObservation sequences of the reference loop on the restatement's
    model, with repeated second neighbours and at least one dirty re-score"""
    scene = str(tmp_path / "scene.bin")
    fc.write_dropin_scene(fc.dropin_scene(0), scene)
    print(dropin.run(dropin.build("fuse_dropin_gpu", oracle=True), scene, timeout=600, marker="fuse dropin ok"))
