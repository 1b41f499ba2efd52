"""The device CreateNewMapPoints (orbl_*) against the SERIAL reference loop (the oracle's SearchForTriangulation and the
restatement tools/newpoints_ref.hpp, one neighbour after the other: tests/newpoints_cases.py) as bits: n_new, every
OrblNewPoint, the whole status table and the F12 / epipole each neighbour's search used -- over the scene families, both
entries (host arrays, device-resident frames), 20 neighbours x 2000 features, more than 8192 features per keyframe, the
hand-made degenerate pairs, the empty cases and the refusals; and the C++ drop-in on mock keyframes."""

import numpy as np
import pytest

import dropin
import newpoints_cases as nc
from orbslamm_amd import local_mapping as lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.6, False, device=0)


def run_host(matcher, case, **kw):
    return lm.create_new_map_points(matcher, case["cur"], case["nbs"], case["sf"], case["sigma2"], case["scale_factor"], **kw)


def assert_equal(got, want, what):
    pts, status, f12 = got
    wpts, wstatus, wf12 = want[:3]
    assert len(pts) == len(wpts), (what, len(pts), len(wpts))
    assert nc.same(status, wstatus), (what, np.argwhere(status != wstatus)[:5].tolist())
    assert pts.tobytes() == wpts.tobytes(), what
    assert nc.same(f12, wf12), what


@pytest.mark.parametrize("name", sorted(nc.FAMILIES))
def test_families_bit_exact(matcher, oracle, name):
    total = 0
    for seed in nc.SEEDS:
        case = nc.family_case(name, seed)
        want = nc.serial_reference(oracle, case)
        got = run_host(matcher, case)
        assert_equal(got, want, "%s seed %d" % (name, seed))
        total += len(got[0])
        # orbl_compute_f12 is what the batch used for every neighbour it processed
        for k, nb in enumerate(case["nbs"]):
            if got[1].shape[1] and (got[1][k] != lm.ST_NEIGHBOUR_SKIPPED).any():
                F, e = lm.compute_f12(case["cur"]["kf"], nb["kf"])
                assert F.tobytes() == got[2][k, :9].tobytes() and e.tobytes() == got[2][k, 9:].tobytes()
        if seed == 0:   # the same call again: identical bytes (the path holds no atomics)
            again = run_host(matcher, case)
            assert again[0].tobytes() == got[0].tobytes() and nc.same(again[1], got[1])
    assert total >= 100


def test_degenerate_pairs_and_empty_cases(matcher, oracle):
    case = nc.degenerate_case()
    want = nc.serial_reference(oracle, case)
    got = run_host(matcher, case)
    assert_equal(got, want, "degenerate")
    assert got[1][0, 0] == lm.ST_X3D_ZERO and got[1][1, 1] == lm.ST_REPROJ2 and got[1][2, 2] == lm.ST_DIST_ZERO
    for kind in nc.EMPTY_KINDS:
        case = nc.empty_case(kind)
        got = run_host(matcher, case)
        assert_equal(got, nc.serial_reference(oracle, case), kind)
        if kind != "no_neighbour_features":
            assert len(got[0]) == 0


def _many_neighbours(rng, count):
    out = []
    for i in range(count):
        d = rng.normal(size=3) * np.array([1.0, 0.4, 0.2])
        out.append((tuple(d / np.linalg.norm(d) * rng.uniform(0.06, 0.3)), float(rng.uniform(0.01, 0.06)), nc.K_A, "true"))
    return out


def test_twenty_neighbours_of_2000_features(matcher, oracle):
    rng = np.random.default_rng(20)
    case = nc.make_case(2020, n=1600, nb=_many_neighbours(rng, 20), depth=(4, 9), noise=0.25, vis=0.35, skip1=0.3, skip2=0.3)
    assert len(case["cur"]["keys"]) >= 1900 and len(case["nbs"]) == 20
    want = nc.serial_reference(oracle, case)
    got = run_host(matcher, case)
    assert_equal(got, want, "20 x 2000")
    per = np.bincount(got[0]["neighbour"], minlength=20)
    assert len(got[0]) >= 500 and (per > 0).sum() >= 12, per.tolist()


def test_more_than_8192_features(matcher, oracle):
    case = nc.make_case(8192, n=9000, nb=[(o, a, nc.K_A, "true") for o, a in nc._SIDE[:3]], depth=(4, 9), noise=0.25, vis=0.97,
                        skip1=0.2, skip2=0.2, nnodes=400)
    assert len(case["cur"]["keys"]) > 8192 and min(len(nb["keys"]) for nb in case["nbs"]) > 8192
    want = nc.serial_reference(oracle, case)
    got = run_host(matcher, case)
    assert_equal(got, want, "> 8192 features")
    assert len(got[0]) >= 1000


# ------------------------------------------------------------------------------------------------ device-resident frames
@pytest.fixture(scope="module")
def world(gpu, oracle):
    """one device vocabulary (and the oracle's twin) and one extractor handle, whose device buffers carry the keys and
    descriptors the frames are built from, for all frame tests of the module"""
    from orbslamm_amd import ORBextractor, ORBVocabulary
    from vocab_cases import make_vocab
    voc = make_vocab(np.random.default_rng(3), 10, 4)
    G = ORBVocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
    O = oracle.Vocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1, device=0)
    yield dict(G=G, O=O, gex=gex)
    gex.close()
    G.close()


_NO_FV = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))


class _Frames:
    """the sides of a case as device-resident frames with their BoW computed by the device vocabulary; the case's feature
    vectors are replaced by the oracle vocabulary's, which is what the reference side then searches with"""

    def __init__(self, matcher, world, case):
        from orbslamm_amd import make_grid
        self.m, self.world, self.frames = matcher, world, []
        gex = world["gex"]
        self.mark = len(gex._dev_bufs)
        g = make_grid(0.0, 0.0, nc.W, nc.H)
        for side in [case["cur"]] + case["nbs"]:
            n = len(side["keys"])
            pad = np.zeros((1, 1, 64), np.uint8)            # (a frame without features still gets real addresses)
            dk = gex.upload_frames(np.ascontiguousarray(side["keys"]).view(np.uint8).reshape(1, 1, -1) if n else pad)[0]
            dd = gex.upload_frames(np.ascontiguousarray(side["desc"]).reshape(1, 1, -1) if n else pad)[0]
            self.frames.append(matcher.frame_from_device(dk, dd, n, side["kf"]["K"], [0, 0, 0, 0, 0], g))   # zero distortion: mvKeysUn = mvKeys
            side["fv"] = world["O"].transform(side["desc"], 4)[1] if n else _NO_FV

    def bow(self):
        for F in self.frames:
            self.m.frame_compute_bow(F, self.world["G"], 4)

    def sides(self, case):
        cur = dict(frame=self.frames[0], skip=case["cur"]["skip"], kf=case["cur"]["kf"])
        return cur, [dict(frame=F, skip=nb["skip"], kf=nb["kf"]) for F, nb in zip(self.frames[1:], case["nbs"])]

    def run(self, case):
        cur, nbs = self.sides(case)
        return lm.create_new_map_points(self.m, cur, nbs, case["sf"], case["sigma2"], case["scale_factor"])

    def close(self):
        from orbslamm_amd._lib import check
        for F in self.frames:
            self.m.frame_destroy(F)
        gex = self.world["gex"]             # (every call that read the buffers has returned: the frames were built and searched)
        for d in gex._dev_bufs[self.mark:]:
            check(gex._L.orbx_device_free(gex._h, d))
        del gex._dev_bufs[self.mark:]


def _frames_parity(matcher, oracle, world, case, what):
    fr = _Frames(matcher, world, case)
    fr.bow()
    want = nc.serial_reference(oracle, case)
    got = fr.run(case)
    assert_equal(got, want, what + " (frames)")
    assert_equal(run_host(matcher, case), want, what + " (host arrays, vocabulary nodes)")
    fr.close()
    return got


@pytest.mark.parametrize("name", sorted(nc.FAMILIES))
def test_resident_frames_bit_exact(matcher, oracle, world, name):
    total, codes = 0, np.zeros(12, np.int64)
    for seed in nc.SEEDS:
        got = _frames_parity(matcher, oracle, world, nc.family_case(name, seed), "%s seed %d" % (name, seed))
        total += len(got[0])
        codes += np.bincount(got[1].reshape(-1), minlength=12)
    print(name, dict(zip(lm.STATUS_NAMES, codes.tolist())))
    assert total >= 100
    want = {"short_baseline": (lm.ST_NEIGHBOUR_SKIPPED,), "low_parallax": (lm.ST_PARALLAX,), "scale_inconsistent": (lm.ST_SCALE,),
            "wrong_matches": (lm.ST_Z1, lm.ST_Z2), "already_mapped": (lm.ST_FEATURE_SKIPPED,)}.get(name, ())
    for code in want:
        assert codes[code] > 0, (name, lm.STATUS_NAMES[code])


def test_resident_frames_empty_cases(matcher, oracle, world):
    """zero neighbours, a current keyframe without features, a neighbour without features, and keyframes whose vocabulary
    nodes are disjoint, through the frames entry"""
    for kind in ("no_neighbours", "no_features", "no_neighbour_features"):
        got = _frames_parity(matcher, oracle, world, nc.empty_case(kind), kind)
        if kind != "no_neighbour_features":
            assert len(got[0]) == 0
    # disjoint nodes: the vocabulary decides the node here, so every feature of the current keyframe carries one descriptor and
    # every feature of the neighbours another, from a different node
    rng = np.random.default_rng(9)
    case = nc.empty_case("disjoint_nodes")
    da = rng.integers(0, 256, 32, dtype=np.uint8)
    node = lambda d: world["O"].transform(d.reshape(1, 32), 4)[1][0].tolist()
    for _ in range(100):
        db = rng.integers(0, 256, 32, dtype=np.uint8)
        if node(db) != node(da):
            break
    assert node(db) != node(da)
    case["cur"]["desc"] = np.repeat(da.reshape(1, 32), len(case["cur"]["keys"]), axis=0)
    for nb in case["nbs"]:
        nb["desc"] = np.repeat(db.reshape(1, 32), len(nb["keys"]), axis=0)
    got = _frames_parity(matcher, oracle, world, case, "disjoint nodes")
    assert len(got[0]) == 0 and not (got[1] >= lm.ST_PARALLAX).any() and (got[1] == lm.ST_NO_MATCH).any()


def test_resident_frames_twenty_neighbours_and_large_frames(matcher, oracle, world):
    rng = np.random.default_rng(21)
    case = nc.make_case(2021, n=1600, nb=_many_neighbours(rng, 20), depth=(4, 9), noise=0.25, vis=0.35, skip1=0.3, skip2=0.3)
    got = _frames_parity(matcher, oracle, world, case, "20 x 2000")
    assert len(case["cur"]["keys"]) >= 1900 and len(got[0]) >= 500
    case = nc.make_case(8193, n=9000, nb=[(o, a, nc.K_A, "true") for o, a in nc._SIDE[:3]], depth=(4, 9), noise=0.25, vis=0.97,
                        skip1=0.2, skip2=0.2)
    assert len(case["cur"]["keys"]) > 8192 and min(len(nb["keys"]) for nb in case["nbs"]) > 8192
    got = _frames_parity(matcher, oracle, world, case, "> 8192 features")
    assert len(got[0]) >= 1000


def test_refusals(matcher, oracle, world):
    from orbslamm_amd._lib import ORBX_E_CAPACITY, ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError

    def code(fn):
        with pytest.raises(OrbError) as ei:
            fn()
        return ei.value

    case = nc.family_case("general", 1)
    want = nc.serial_reference(oracle, case)
    assert code(lambda: run_host(matcher, case, check_ori=True)).code == ORBX_E_UNSUPPORTED
    # capacity: the needed count is reported
    e = code(lambda: run_host(matcher, case, capacity=len(want[0]) - 1))
    assert e.code == ORBX_E_CAPACITY and e.needed == len(want[0])
    assert_equal(run_host(matcher, case, capacity=len(want[0])), want, "exact capacity")
    # more than ORBL_MAX_NEIGHBOURS
    many = dict(case, nbs=[case["nbs"][i % len(case["nbs"])] for i in range(lm.MAX_NEIGHBOURS + 1)])
    assert code(lambda: run_host(matcher, many)).code == ORBX_E_UNSUPPORTED
    # a malformed feature vector
    bad = dict(case, cur=dict(case["cur"], fv=(case["cur"]["fv"][0], case["cur"]["fv"][1], case["cur"]["fv"][2] + len(case["cur"]["keys"]))))
    assert code(lambda: run_host(matcher, bad)).code == ORBX_E_INVALID
    # frames: without BoW, repeated, the current keyframe among the neighbours
    fr = _Frames(matcher, world, case)
    cur, nbs = fr.sides(case)
    call = lambda c, n: lm.create_new_map_points(matcher, c, n, case["sf"], case["sigma2"], case["scale_factor"])
    e = code(lambda: call(cur, nbs))
    assert e.code == ORBX_E_INVALID and "orbm_frame_compute_bow" in str(e)
    fr.bow()
    assert code(lambda: call(cur, nbs[:2] + [nbs[0]])).code == ORBX_E_INVALID
    assert code(lambda: call(cur, nbs[:2] + [cur])).code == ORBX_E_INVALID
    assert code(lambda: call(cur, nbs + [nbs[i % len(nbs)] for i in range(lm.MAX_NEIGHBOURS)])).code == ORBX_E_UNSUPPORTED
    assert_equal(call(cur, nbs), nc.serial_reference(oracle, case), "frames after the refusals")
    fr.close()


def test_newpoints_dropin_on_mock_keyframes(gpu, oracle, tmp_path):
    """include/LocalMapping_hip.hpp (CreateNewMapPointsT) on mock keyframes and map points (tests/cpp/newpoints_dropin_gpu.cpp):
    the replay leaves the object graph of the reference loop written out there over the C oracle and the restatement; with
    the CheckNewKeyFrames predicate firing at neighbour 3, exactly neighbours 0..2"""
    scene = str(tmp_path / "scene.bin")
    nc.write_scene(nc.family_case("general", 0), scene)
    dropin.run(dropin.build("newpoints_dropin_gpu", oracle=True), scene, timeout=600, marker="newpoints dropin ok")
