"""The device SearchAndFuse (orbc_search_and_fuse*, k_loopfuse_search / k_loopfuse_compact) against the restatement's
projection (tools/loopfuse_ref.hpp) and the oracle's window_best without chi-square (tests/loopfuse_cases.py) as bits: every
hit, hit_start, n_hits and every status byte, over the scene families, both entries (host arrays, device-resident frames),
the shapes around the tile sizes, the empty cases, 200 targets, a target of 9000 features, the capacity refusal and the
refusals that need a handle; against orbl_fuse_batch with its chi-square gate disabled; and the C++ drop-in on mock keyframes."""
import ctypes as C

import numpy as np
import pytest

import dropin
import fuse_cases as fc
import loopfuse_cases as lc
from orbslamm_amd import local_mapping as lm
from orbslamm_amd import loop_closing as lo
from orbslamm_amd._lib import KP_DTYPE, ORBX_E_CAPACITY, ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError, OrbmGrid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.8, False, device=0)


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
    kw.setdefault("want_status", True)
    return lo.search_and_fuse(matcher, case["targets"], case["points"], case["sf"], breaks, th=case["th"], **kw)


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

    def run(self, case, breaks, **kw):
        kw.setdefault("want_status", True)
        return lo.search_and_fuse(self.m, self.targets, case["points"], case["sf"], breaks, th=case["th"], **kw)

    def close(self):
        from orbslamm_amd._lib import check
        for F in self.frames:
            self.m.frame_destroy(F)
        for d in self.gex._dev_bufs[self.mark:]:   # (every call that read the buffers has returned)
            check(self.gex._L.orbx_device_free(self.gex._h, d))
        del self.gex._dev_bufs[self.mark:]


def assert_equal(got, want, what):
    """hits, hit_start (and with it n_hits) and the status table as bits"""
    for g, w, part in zip(got, want, ("hits", "hit_start", "status")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
            raise AssertionError((what, part, len(bad), [(int(i), g.reshape(-1)[i].tolist(), w.reshape(-1)[i].tolist()) for i in bad[:4]]))
    assert got[1][-1] == len(got[0])


def both_entries(matcher, gex, oracle, case, breaks, what, **kw):
    want = lc.reference(oracle, case, kw.get("max_dist", lo.TH_LOW))
    got = run_host(matcher, case, breaks, **kw)
    assert_equal(got, want, what + " (host arrays)")
    fr = _Frames(matcher, gex, case)
    try:
        assert_equal(fr.run(case, breaks, **kw), want, what + " (frames)")
    finally:
        fr.close()
    return got


@pytest.mark.parametrize("name", sorted(lc.FAMILIES))
def test_families_bit_exact(matcher, gex, oracle, breaks, name):
    codes, nhits = np.zeros(7, np.int64), 0
    for seed in lc.SEEDS:
        case = lc.family_case(name, seed)
        hits, start, status = both_entries(matcher, gex, oracle, case, breaks, "%s seed %d" % (name, seed))
        codes += np.bincount(status.reshape(-1), minlength=7)
        nhits += len(hits)
        if seed == 0:   # the same call again: identical bytes (no atomics), and production's NULL status changes nothing else
            again = run_host(matcher, case, breaks)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (hits, start, status)))
            bare = run_host(matcher, case, breaks, want_status=False)
            assert bare[2] is None and bare[0].tobytes() == hits.tobytes() and bare[1].tobytes() == start.tobytes()
    print(name, dict(zip(lm.FUSE_STATUS_NAMES, codes.tolist())), "hits", nhits)
    assert nhits >= lc.HIT_FLOOR[name], (name, nhits)
    if name in lc.FAMILY_CODES:
        assert codes[lc.FAMILY_CODES[name]] > 0, (name, lm.FUSE_STATUS_NAMES[lc.FAMILY_CODES[name]])
    if name == "sparse_survivors":
        assert (codes[lm.FUSE_ST_NO_CANDIDATE] + codes[lm.FUSE_ST_FOUND]) / codes.sum() < lc.SPARSE_SHARE_CAP


def _cut(case, n_points, name):
    return dict(case, points=np.ascontiguousarray(case["points"][:n_points]), name=name)


@pytest.fixture(scope="module")
def wide():
    """three targets against 600 points: the pool the point counts around the tile sizes are cut from"""
    return lc.make_dense(5100, targets=(3, 3), points=(600, 600), feats=500)


@pytest.mark.parametrize("n_points", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513])
def test_point_counts_around_the_tile_sizes(matcher, gex, oracle, breaks, wide, n_points):
    """one point, a wave more or less, and one below, at and one above every tile size the kernel can be built with (128,
    256, 512): the tile in use is among them"""
    case = _cut(wide, n_points, "wide/%d" % n_points)
    hits, start, status = both_entries(matcher, gex, oracle, case, breaks, "%d points" % n_points)
    assert status.shape == (3, n_points)
    if n_points >= 63:
        assert len(hits) >= n_points // 2


def test_empty_cases(matcher, gex, oracle, breaks, wide):
    # zero targets; zero points: ORBX_OK, no hits, hit_start all zero
    hits, start, status = lo.search_and_fuse(matcher, [], wide["points"], wide["sf"], breaks, want_status=True)
    assert len(hits) == 0 and start.tolist() == [0] and status.shape == (0, 600)
    hits, start, status = run_host(matcher, _cut(wide, 0, None), breaks)
    assert len(hits) == 0 and start.tolist() == [0, 0, 0, 0] and status.shape == (3, 0)
    # a target with zero features: NO_CANDIDATE for every pair that passes the gates, and no hit
    bare = dict(wide["targets"][1], keys=wide["targets"][1]["keys"][:0], desc=wide["targets"][1]["desc"][:0])
    case = dict(wide, targets=[wide["targets"][0], bare, wide["targets"][2]], name="wide/bare")
    hits, start, status = both_entries(matcher, gex, oracle, case, breaks, "a target without features")
    assert start[1] == start[2] and (status[1] <= lm.FUSE_ST_NO_CANDIDATE).all() and (status[1] == lm.FUSE_ST_NO_CANDIDATE).sum() > 100
    # a call with zero hits: every target looks away; and one whose survivors find nothing under max_dist 0
    away = [lc.with_pose(t, -t["rec"]["Rcw"], -t["rec"]["tcw"], t["rec"]["Ow"]) for t in wide["targets"]]      # (the mirrored camera: z changes sign)
    hits, start, status = both_entries(matcher, gex, oracle, dict(wide, targets=away, name="wide/away"), breaks, "every target looks away")
    assert len(hits) == 0 and start.tolist() == [0, 0, 0, 0] and (status == lm.FUSE_ST_DEPTH).all()
    hits, start, status = both_entries(matcher, gex, oracle, wide, breaks, "max_dist 0", max_dist=0)
    assert len(hits) == 0 and (status == lm.FUSE_ST_FOUND).sum() > 500
    # max_dist 256 keeps every FOUND pair
    hits, start, status = both_entries(matcher, gex, oracle, wide, breaks, "max_dist 256", max_dist=256)
    assert len(hits) == (status == lm.FUSE_ST_FOUND).sum()


def test_200_targets_over_5_frames(matcher, gex, oracle, breaks):
    """beyond orbl_fuse_batch's 128 targets: 200 poses of 5 distinct keyframes against 64 points"""
    case = lc.make_dense(5200, targets=(5, 5), points=(64, 64), feats=100)
    rng = np.random.default_rng(5201)
    tg = []
    for j in range(200):
        t = case["targets"][j % 5]
        if j < 5:
            tg.append(t)
            continue
        R = lc.rot_axis_angle(rng.normal(size=3), rng.uniform(0, 0.004)) @ t["rec"]["Rcw"].astype(np.float64)
        O = t["rec"]["Ow"].astype(np.float64) + rng.normal(size=3) * 0.005
        tg.append(lc.with_pose(t, R, -R @ O, O))
    case = dict(case, targets=tg, name="200x64")
    assert len({id(t["keys"]) for t in tg}) == 5 and all(len(t["keys"]) >= 100 for t in tg)
    hits, start, status = both_entries(matcher, gex, oracle, case, breaks, "200 targets")
    assert len(start) == 201 and len(hits) >= 2000 and (np.diff(start) > 0).sum() >= 150


def test_same_arrays_under_another_grid_do_not_share_a_grid(matcher, oracle, breaks, wide):
    """two targets that name the SAME keys / desc arrays under different poses ride in the staging block once; a third that
    names them under another grid (80 x 60 cells) gets a grid of its own: every output equals the call made with separate
    copies of the arrays, and the reference"""
    t0, t1 = wide["targets"][0], wide["targets"][1]
    fine = t0["rec"].copy()
    fine["grid"] = np.array(fc.grid_tuple(80, 60), dtype=lm.GRID_DTYPE)
    shared = [t0, lc.with_pose(t0, t1["rec"]["Rcw"], t1["rec"]["tcw"], t1["rec"]["Ow"]), dict(t0, rec=fine)]
    assert all(t["keys"] is t0["keys"] and t["desc"] is t0["desc"] for t in shared)
    apart = [dict(t, keys=t["keys"].copy(), desc=t["desc"].copy()) for t in shared]
    got = run_host(matcher, dict(wide, targets=shared, name=None), breaks)
    assert_equal(got, run_host(matcher, dict(wide, targets=apart, name=None), breaks), "shared arrays against separate copies")
    assert_equal(got, lc.reference(oracle, dict(wide, targets=shared, name=None)), "shared arrays")
    assert (got[2][0] == lm.FUSE_ST_FOUND).sum() >= 100 and (got[2][2] == lm.FUSE_ST_FOUND).sum() >= 100


def test_one_target_of_9000_features(matcher, gex, oracle, breaks):
    case = lc.make_dense(8193, name="9000", targets=(1, 1), points=(12000, 12000), feats=9000, vis=1.0, spread=0.0)
    assert len(case["targets"]) == 1 and len(case["targets"][0]["keys"]) >= 9000
    hits, start, status = both_entries(matcher, gex, oracle, case, breaks, "9000 features")
    assert len(hits) >= 3000 and hits["best_idx"].max() > 8192


def test_capacity_one_short_and_refusals(matcher, gex, oracle, breaks, wide):
    def code(fn):
        with pytest.raises(OrbError) as ei:
            fn()
        return ei.value

    want = lc.reference(oracle, wide)
    need = len(want[0])
    assert need > 500
    # capacity one short: ORBX_E_CAPACITY, *n_hits the need, nothing written (through the C entry, on canaries)
    L = lm.lib()
    recs = np.array([t["rec"] for t in wide["targets"]], dtype=lm.FUSE_TARGET_DTYPE)
    keys, desc = lm._ptr_array([t["keys"] for t in wide["targets"]]), lm._ptr_array([t["desc"] for t in wide["targets"]])
    n = np.array([len(t["keys"]) for t in wide["targets"]], np.int32)
    hits = np.full(need, 0x5A, dtype=np.uint8).repeat(16).view(lo.HIT_DTYPE)
    start, status = np.full(4, -77, np.int32), np.full((3, 600), 0xEE, np.uint8)
    nh = C.c_int(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.orbc_search_and_fuse(matcher._h, p(recs), keys, desc, p(n), 3, p(wide["points"]), 600, C.c_float(wide["th"]), 50, p(wide["sf"]), 8, p(breaks),
                                p(hits), need - 1, C.byref(nh), p(start), p(status))
    assert rc == ORBX_E_CAPACITY and nh.value == need
    assert (hits.view(np.uint8) == 0x5A).all() and (start == -77).all() and (status == 0xEE).all()
    e = code(lambda: run_host(matcher, wide, breaks, capacity=need - 1))
    assert e.code == ORBX_E_CAPACITY and e.needed == need
    assert_equal(run_host(matcher, wide, breaks, capacity=need), want, "capacity exactly the need")
    assert_equal(run_host(matcher, wide, breaks), want, "the mirror's own guess")
    # the refusals, now behind a real handle
    tg = wide["targets"]
    assert code(lambda: lo.search_and_fuse(matcher, [tg[0]] * (lo.MAX_TARGETS + 1), wide["points"], wide["sf"], breaks)).code == ORBX_E_UNSUPPORTED
    assert code(lambda: lo.search_and_fuse(matcher, [tg[0]] * 4096, np.zeros(lo.MAX_PAIRS // 4096 + 1, lm.FUSE_POINT_DTYPE), wide["sf"], breaks)).code == ORBX_E_UNSUPPORTED
    for b in (breaks[::-1], np.r_[breaks[:3], breaks[2], breaks[4:]], np.r_[breaks[:3], np.nan, breaks[4:]]):
        assert code(lambda: run_host(matcher, wide, b.astype(np.float32))).code == ORBX_E_INVALID
    for md in (-1, 257):
        assert code(lambda: run_host(matcher, wide, breaks, max_dist=md)).code == ORBX_E_INVALID
    assert code(lambda: lo.search_and_fuse(matcher, tg, wide["points"], wide["sf"][:0], breaks[:1])).code == ORBX_E_INVALID
    assert code(lambda: lo.search_and_fuse(matcher, tg, wide["points"], np.r_[wide["sf"], wide["sf"], 1.0].astype(np.float32), np.arange(18, dtype=np.float32))).code == ORBX_E_INVALID
    big = dict(tg[0], keys=np.zeros(65536, KP_DTYPE), desc=np.zeros((65536, 32), np.uint8))
    assert code(lambda: run_host(matcher, dict(wide, targets=[big] + tg[1:]), breaks)).code == ORBX_E_INVALID
    rec = tg[0]["rec"].copy()
    rec["grid"]["cols"] = 0
    assert code(lambda: run_host(matcher, dict(wide, targets=[dict(tg[0], rec=rec)] + tg[1:]), breaks)).code == ORBX_E_INVALID
    fr = _Frames(matcher, gex, wide)
    try:
        null = [dict(rec=fr.targets[0]["rec"], frame=C.c_void_p(None))] + fr.targets[1:]
        assert code(lambda: lo.search_and_fuse(matcher, null, wide["points"], wide["sf"], breaks)).code == ORBX_E_INVALID
        assert_equal(fr.run(wide, breaks), want, "frames after the refusals")
    finally:
        fr.close()
    assert_equal(run_host(matcher, wide, breaks), want, "host arrays after the refusals")


@pytest.mark.parametrize("name,seed", [("general", 1), ("crowded_ties", 2), ("mixed_intrinsics", 3), ("sparse_survivors", 0)])
def test_equals_fuse_batch_with_its_chi_square_gate_disabled(matcher, breaks, name, seed):
    """orbl_fuse_batch on the dense job list with inv_level_sigma2 all zero (e2 * 0 > 5.99 never holds), filtered by
    best_dist <= max_dist: the same hits and statuses, pair for pair.  (Its invz is the float division, which is what this
    entry's device code uses too; the restatement's `1.0/z` form is held equal to it on the CPU.)"""
    case = lc.family_case(name, seed)
    T, P = len(case["targets"]), len(case["points"])
    hits, start, status = run_host(matcher, case, breaks)
    got_b = []
    for t0 in range(0, T, lm.FUSE_MAX_TARGETS):
        tg = case["targets"][t0:t0 + lm.FUSE_MAX_TARGETS]
        js = (np.arange(len(tg) + 1) * P).astype(np.int32)
        jp = np.tile(np.arange(P, dtype=np.int32), len(tg))
        got_b.append(lm.fuse_batch(matcher, tg, case["points"], (js, jp), case["sf"], np.zeros(len(case["sf"]), np.float32), breaks, th=case["th"]))
    res = np.concatenate(got_b).reshape(T, P)
    assert res["status"].astype(np.uint8).tobytes() == status.tobytes()
    tk, pk = np.nonzero((res["best_idx"] >= 0) & (res["best_dist"] <= lo.TH_LOW))
    assert np.array_equal(tk, hits["target"]) and np.array_equal(pk, hits["point"])
    assert np.array_equal(res["best_idx"][tk, pk], hits["best_idx"]) and np.array_equal(res["best_dist"][tk, pk], hits["best_dist"])
    assert np.array_equal(np.r_[0, np.cumsum(np.bincount(tk, minlength=T))], start)


def test_loopfuse_dropin_on_mock_keyframes(gpu, tmp_path):
    """include/LoopClosing_hip.hpp (SearchAndFuseT) on mock keyframes and map points (tests/cpp/loopfuse_dropin_gpu.cpp): the
    replay leaves the object graph, the total and the Replace / AddObservation sequences of the serial loop on the
    restatement's model, under Scw of scale 0.5, 2 and 1; with the stale re-score disabled it does not"""
    scene = str(tmp_path / "scene.bin")
    lc.write_map_scene(lc.map_scene(0), scene)
    out = dropin.run(dropin.build("loopfuse_dropin_gpu"), scene, timeout=600, marker="loopfuse dropin ok")
    print(out)
    assert "share" in out
