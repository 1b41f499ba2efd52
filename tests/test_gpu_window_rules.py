"""The designed window scenes of tests/window_cases.py (window geometry, thresholds and ties at equality, mode 3's ratio rule per level
pair, serial chains and re-takes, occupancy and assign entries on entry, the stereo gates, steals in SearchForInitialization, the last
of equals in SearchForTriangulation) through every device entry that implements the rule, byte for byte against the same oracle calls
tests/test_matcher_oracle_cpu.py checks the design with (there the census says that every family reaches its branch):
    host arrays: SearchByProjection modes 3 - 6 with and without the stereo gate (k_proj_candidates + k_proj_resolve), GetFeaturesInArea,
                 window_best (k_window_best), SearchForInitialization (k_init_resolve), SearchForTriangulation (k_triangulation_pairs);
    resident:    SearchByProjectionFrame, window_best_frame, SearchForInitializationFrames, FrameSet.track_local_points (mode 3) and
                 FrameSet.track_projected (modes 4 / 5) (k_track_candidates + k_track_resolve)."""
import numpy as np
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu

K, D0 = [500.0, 500.0, 320.0, 240.0], [0, 0, 0, 0, 0]
CAP = 512


class Rig:
    """one extractor handle (it owns the raw device buffers), one matcher per (ratio, ori), made when first asked for"""

    def __init__(self):
        from orbslamm_amd import ORBextractor, make_grid
        self.gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=1, device=0)
        self.grid = make_grid(0.0, 0.0, wc.W, wc.H)
        self.matchers = {}

    def matcher(self, ratio, ori):
        from orbslamm_amd import ORBmatcher
        if (ratio, ori) not in self.matchers:
            self.matchers[ratio, ori] = ORBmatcher(ratio, ori, device=0)
        return self.matchers[ratio, ori]

    def up(self, a):
        return self.gex.upload_frames(np.ascontiguousarray(a).view(np.uint8).reshape(1, 1, -1))[0]

    def frame(self, m, keys, desc):
        return m.frame_from_device(self.up(keys), self.up(desc), len(keys), K, D0, self.grid)

    def frame_set(self, m, c):
        """slot 0: the queries as a frame (LastFrame of track_projected), slot 1: the train frame"""
        keys = np.zeros((2, CAP), dtype=c["tk"].dtype)
        desc = np.zeros((2, CAP, 32), np.uint8)
        keys[0, :c["nq"]], keys[1, :c["nt"]], desc[0, :c["nq"]], desc[1, :c["nt"]] = c["qk"], c["tk"], c["qd"], c["td"]
        fs = m.frame_set(2, CAP, K, D0, self.grid, [0.0, wc.W, 0.0, wc.H], wc.SF)
        fs.build(0, 2, self.up(keys), self.up(desc), self.up(np.array([c["nq"], c["nt"]], np.int32)), CAP)
        return fs

    def close(self):
        for m in self.matchers.values():
            m.close()
        self.gex.close()


@pytest.fixture(scope="module")
def rig(gpu):
    r = Rig()
    yield r
    r.close()


@pytest.fixture(scope="module")
def proj_want(oracle):
    """per run of wc.PROJ_RUNS: (scene, the oracle's answer with the entry's assign table, and with a table of -1) -- computed once"""
    out = []
    for run in wc.PROJ_RUNS:
        c = wc.proj_scene(oracle, run)
        out.append((run, c, wc.proj_oracle(oracle, c, run), wc.proj_oracle(oracle, c, run, entry_assign=False)))
    return out


def _same3(got, want):
    return got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("mode", [3, 4, 5, 6])
def test_designed_scenes_through_search_by_projection(rig, proj_want, mode):
    for run, c, want, _ in proj_want:
        if run["mode"] != mode:
            continue
        m = rig.matcher(run["ratio"], run["ori"])
        st = run["stereo"]
        got = m.SearchByProjection(mode, run["th"], c["uvr"], c["lvl"], c["qd"], c["qa"], c["qv"], c["qo"], rig.grid, c["tk"], c["td"], c["occ"],
                                   c["assign0"], c["q_ur"] if st else None, c["t_ur"] if st else None)
        assert _same3(got, want), (run, got[2], want[2], np.nonzero(got[0] != want[0])[0][:8])


@pytest.mark.parametrize("mode", [3, 4, 5, 6])
def test_designed_scenes_through_search_by_projection_frame(rig, proj_want, mode):
    frames = {}
    for run, c, want, _ in proj_want:
        if run["mode"] != mode or run["stereo"]:   # (a resident frame carries no right coordinates)
            continue
        m = rig.matcher(run["ratio"], run["ori"])
        key = (id(c), run["ratio"], run["ori"])
        if key not in frames:
            frames[key] = (m, rig.frame(m, c["tk"], c["td"]))
        got = m.SearchByProjectionFrame(mode, run["th"], c["uvr"], c["lvl"], c["qd"], c["qa"], c["qv"], c["qo"], frames[key][1], c["occ"], c["assign0"])
        assert _same3(got, want), (run, got[2], want[2])
    for m, f in frames.values():
        m.frame_destroy(f)


def test_designed_scenes_through_a_frame_set(rig, proj_want):
    """track_local_points (mode 3: the queries' descriptors go up) and track_projected (modes 4 / 5: the queries are slot 0's features,
    their descriptors and angles stay resident).  The set starts its table at -1 and takes the occupancy on entry."""
    m = rig.matcher(0.9, True)
    sets = {}
    for run, c, _, want in proj_want:
        if run["stereo"] or run["mode"] == 6:
            continue
        if id(c) not in sets:
            sets[id(c)] = rig.frame_set(m, c)
        fs = sets[id(c)]
        if run["mode"] == 3:
            fs.track_local_points(1, c["uvr"], c["lvl"], c["qd"], c["qv"], c["qo"], c["occ"], th_dist=run["th"], nnratio=run["ratio"], mode=3)
        else:
            fs.track_projected(1, 0, c["uvr"], c["lvl"], c["qv"], c["qo"], c["occ"], th_dist=run["th"], nnratio=run["ratio"], check_ori=run["ori"],
                               mode=run["mode"])
        assign, n = fs.results()
        assert n[0] == want[2] and np.array_equal(assign[0, :c["nt"]], want[0]), (run, int(n[0]), want[2])
    for fs in sets.values():
        fs.close()


def test_designed_windows_through_get_features_in_area(rig, oracle, proj_want):
    """every window of one projection scene, and every level window over each of them that holds anything: same indices, same order"""
    run, c = proj_want[0][:2]
    m = rig.matcher(0.9, True)
    some = 0
    for q in range(c["nq"]):
        x, y, r = (float(v) for v in c["uvr"][q])
        windows = {tuple(int(v) for v in c["lvl"][q])}
        if len(oracle.features_in_area(c["gp"], c["tk"], c["start"], c["idx"], x, y, r, -1, -1)):
            windows |= set(wc.LEVEL_WINDOWS)
        for lo, hi in sorted(windows):
            want = oracle.features_in_area(c["gp"], c["tk"], c["start"], c["idx"], x, y, r, lo, hi)
            got = m.GetFeaturesInArea(rig.grid, c["tk"], x, y, r, lo, hi)
            assert np.array_equal(got, want), (q, lo, hi)
            some += len(want) > 0
    assert some > 100


def test_designed_scenes_through_window_best(rig, oracle):
    m = rig.matcher(0.9, True)
    frame = None
    for run in wc.WINDOW_RUNS:
        c = wc.make_window_scene(oracle, run["stereo"])
        want = wc.window_oracle(oracle, c, run)
        st = run["stereo"]
        got = m.window_best(c["uvr"], c["pred"], c["qd"], c["qv"], rig.grid, c["tk"], c["td"], wc.INV_SIGMA2, run["chi2"],
                            c["q_ur"] if st else None, c["t_ur"] if st else None)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (run, np.nonzero(got[0] != want[0])[0][:8])
        if not st:   # the resident form is mono
            frame = frame or rig.frame(m, c["tk"], c["td"])
            got = m.window_best_frame(c["uvr"], c["pred"], c["qd"], c["qv"], frame, wc.INV_SIGMA2, run["chi2"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (run, "frame")
    m.frame_destroy(frame)


def test_designed_scene_through_search_for_initialization(rig, oracle):
    c = wc.make_init_scene(oracle)
    frames = {}
    for run in wc.INIT_RUNS:
        m = rig.matcher(run["ratio"], run["ori"])
        want = wc.init_oracle(oracle, c, run)
        got = m.SearchForInitialization(c["q_xy"], c["window"], c["qk"], c["qd"], rig.grid, c["tk"], c["td"])
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), (run, got[1], want[1], np.nonzero(got[0] != want[0])[0][:8])
        frames[run["ratio"], run["ori"]] = (m, rig.frame(m, c["qk"], c["qd"]), rig.frame(m, c["tk"], c["td"]))
        got = m.SearchForInitializationFrames(c["q_xy"], c["window"], *frames[run["ratio"], run["ori"]][1:])
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), (run, "frames", got[1], want[1])
    for m, f1, f2 in frames.values():
        m.frame_destroy(f1); m.frame_destroy(f2)
    # no query at all, and no train feature at all
    m = rig.matcher(0.9, True)
    z, zd = np.zeros(0, oracle.KP_DTYPE), np.zeros((0, 32), np.uint8)
    got = m.SearchForInitialization(np.zeros((0, 2), np.float32), 10.0, z, zd, rig.grid, c["tk"], c["td"])
    assert got[1] == 0 and len(got[0]) == 0
    got = m.SearchForInitialization(c["q_xy"], 10.0, c["qk"], c["qd"], rig.grid, z, zd)
    assert got[1] == 0 and (got[0] == -1).all() and len(got[0]) == c["nq"]


def test_designed_scenes_through_search_for_triangulation(rig, oracle):
    for run in wc.TRI_RUNS:
        c = wc.make_tri_scene(oracle, run["stereo"])
        want = wc.tri_oracle(oracle, c, run)
        m = rig.matcher(0.9, run["ori"])
        got = m.SearchForTriangulation(c["k1"], c["d1"], c["skip1"], c["fv1"], c["k2"], c["d2"], c["skip2"], c["fv2"], c["F"], c["ex"], c["ey"], c["sf2"],
                                       c["sigma2"], run["only"], c["ur1"], c["ur2"])
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), (run, got[1], want[1], np.nonzero(got[0] != want[0])[0][:8])
