"""Oracle matcher restatement vs naive numpy re-derivations and hand-built cases
(the matcher arithmetic is fully visible in the reference)."""
import numpy as np

from conftest import random_descriptors
from matcher_cases import make_bow_case, make_proj_case, naive_bruteforce


def test_bruteforce_equals_naive(oracle):
    rng = np.random.default_rng(11)
    base = random_descriptors(rng, 300)
    q = base.copy()
    flips = rng.integers(0, 256, size=(300, 12))
    for i in range(300):  # queries = noisy copies -> plenty of accepted matches
        for b in flips[i]:
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    perm = rng.permutation(300)
    t = base[perm]
    qa = rng.uniform(0, 360, 300).astype(np.float32)
    ta = (qa[perm] + rng.normal(0, 3, 300)).astype(np.float32) % np.float32(360)
    m, n = oracle.match_bruteforce(q, qa, t, ta, 0.7, 50, True)
    m2, n2 = naive_bruteforce(q, qa, t, ta, 0.7, 50, True)
    assert n == n2 and np.array_equal(m, m2)
    assert n > 100
    m3, n3 = oracle.match_bruteforce(q, qa, t, ta, 0.7, 50, False)
    assert n3 >= n and (m3 >= 0).sum() == n3


def test_bruteforce_empty_and_single(oracle):
    rng = np.random.default_rng(12)
    q = random_descriptors(rng, 5)
    m, n = oracle.match_bruteforce(q, np.zeros(5, np.float32), np.zeros((0, 32), np.uint8), np.zeros(0, np.float32))
    assert n == 0 and (m == -1).all()
    # a lone candidate has second = 256 (ORBmatcher.cc:199-201): dist 0 < 0.7*256
    m, n = oracle.match_bruteforce(q[:1], np.zeros(1, np.float32), q[:1], np.zeros(1, np.float32))
    assert n == 1 and m[0] == 0


def test_grid_and_features_in_area(oracle):
    rng = np.random.default_rng(13)
    n = 800
    keys = np.zeros(n, dtype=oracle.KP_DTYPE)
    keys["x"] = rng.uniform(0, 640, n).astype(np.float32)
    keys["y"] = rng.uniform(0, 480, n).astype(np.float32)
    keys["octave"] = rng.integers(0, 8, n)
    gp = oracle.make_grid_params(0.0, 0.0, 640.0, 480.0)
    start, idx = oracle.grid_build(gp, keys)
    assert start[-1] <= n
    for _ in range(50):
        x, y = rng.uniform(-20, 660), rng.uniform(-20, 500)
        r = rng.uniform(3, 80)
        lo, hi = [(-1, -1), (0, 2), (3, 5), (2, -1), (0, -1)][rng.integers(0, 5)]
        got = oracle.features_in_area(gp, keys, start, idx, x, y, r, lo, hi)
        # brute-force re-derivation: window test + level rule + grid membership
        in_grid = set(idx[:start[-1]].tolist())
        check = (lo > 0) or (hi >= 0)
        want = []
        for i in range(n):
            if i not in in_grid:
                continue
            if check and (keys["octave"][i] < lo or (hi >= 0 and keys["octave"][i] > hi)):
                continue
            if abs(np.float32(keys["x"][i] - np.float32(x))) < np.float32(r) and abs(np.float32(keys["y"][i] - np.float32(y))) < np.float32(r):
                want.append(i)
        # same set; order is cell-major (checked separately on the GPU vs this oracle)
        assert sorted(got.tolist()) == sorted(want)


def test_search_by_bow_greedy_exclusion(oracle):
    # two identical queries in one node compete for one train feature: the first wins,
    # the second must fall to the runner-up (ORBmatcher.cc:210-211)
    rng = np.random.default_rng(14)
    t = random_descriptors(rng, 3)
    q = np.stack([t[0], t[0]])
    t[1] = t[0]
    t[1, 0] ^= 1  # distance 1 from t[0]
    fvq = (np.array([5], np.uint32), np.array([0, 2], np.int32), np.array([0, 1], np.int32))
    fvt = (np.array([5], np.uint32), np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32))
    ang = np.zeros(3, np.float32)
    m, n = oracle.search_by_bow(q, ang[:2], None, fvq, t, ang, None, fvt, 0.9, False, True)
    # q0 takes t0 (0 < 0.9*1); q1 sees t1 (1) and t2 (far): 1 < 0.9*far -> takes t1
    assert n == 2 and m.tolist() == [0, 1, -1]
    m2, n2 = oracle.search_by_bow(q, ang[:2], None, fvq, t, ang, None, fvt, 0.9, False, False)
    assert n2 == 2 and m2.tolist() == [0, 1]


def test_search_by_bow_random_consistency(oracle):
    rng = np.random.default_rng(15)
    case = make_bow_case(rng, nq=400, nt=450, nnodes=23)
    for by_train in (True, False):
        m, n = oracle.search_by_bow(case["qd"], case["qa"], case["qv"], case["qfv"], case["td"], case["ta"],
                                    None if by_train else case["tv"], case["tfv"], 0.75, True, by_train)
        assert n == (m >= 0).sum()
        used = m[m >= 0]
        assert len(set(used.tolist())) == len(used)  # a feature is matched at most once


def test_projection_modes_smoke(oracle):
    rng = np.random.default_rng(16)
    c = make_proj_case(rng, nq=300, nt=900)
    for mode, th in ((3, 100), (4, 100), (5, 64), (6, 50)):
        assign, occ, n = oracle.search_by_projection(mode, 0.8, True, th, c["uvr"], c["lvl"], c["qd"], c["qa"], c["qv"],
                                                     c["qo"], c["gp"], c["tk"], c["start"], c["idx"], c["td"],
                                                     c["occ"], np.full(900, -1, np.int32))
        assert n >= 0
        if mode in (5, 6):
            assert n == (assign >= 0).sum()


def test_window_best_and_init_and_triangulation_oracle(oracle):
    from matcher_cases import make_init_case, make_tri_case
    rng = np.random.default_rng(17)
    c = make_proj_case(rng, nq=200, nt=800)
    pred = np.clip(c["lvl"][:, 0] + 1, 0, 7).astype(np.int8)
    inv = (1.0 / (np.float32(1.2) ** np.arange(8)) ** 2).astype(np.float32)
    for chi2 in (False, True):
        bi, bd = oracle.window_best(c["uvr"], pred, c["qd"], c["qv"], c["gp"], c["tk"], c["start"], c["idx"], c["td"], inv, chi2)
        ok = bi >= 0
        assert ok.sum() > 20
        # recompute the distance of the reported best
        for q in np.nonzero(ok)[0][:30]:
            assert bd[q] == oracle.descriptor_distance(c["qd"][q], c["td"][bi[q]])
            assert c["tk"]["octave"][bi[q]] in (pred[q] - 1, pred[q])
    ic = make_init_case(rng, 500, 600)
    m12, n = oracle.search_for_initialization(ic["q_xy"], 100.0, ic["k1"], ic["d1"], ic["gp"], ic["k2"], ic["start"], ic["idx"],
                                              ic["d2"], 0.9, True)
    assert n == (m12 >= 0).sum() and n > 50
    used = m12[m12 >= 0]
    assert len(set(used.tolist())) == len(used)          # a stolen feature un-matches its previous owner
    assert (ic["k1"]["octave"][m12 >= 0] == 0).all()     # only octave-0 queries search
    tc = make_tri_case(rng, 400, 450, 19)
    m, n = oracle.search_for_triangulation(tc["k1"], tc["c"]["qd"], 1 - tc["c"]["qv"], tc["c"]["qfv"], tc["k2"], tc["c"]["td"],
                                           1 - tc["c"]["tv"], tc["c"]["tfv"], tc["F"], tc["ex"], tc["ey"], tc["sf2"], tc["sigma2"],
                                           False, False)
    assert n == (m >= 0).sum()


def test_stereo_from_rgbd_semantics(oracle):
    """Frame.cc:641-663: depth looked up at the truncated distorted position, uRight from the undistorted x (binary32: the
    division first), -1 / -1 for holes; outside the image counts as a hole (the reference reads out of bounds)"""
    k = np.zeros(5, oracle.KP_DTYPE); ku = np.zeros(5, oracle.KP_DTYPE)
    k["x"] = [3.7, 10.2, 0.9, 50.0, 7.99]; k["y"] = [2.2, 5.9, 0.1, 3.0, 7.99]
    ku["x"] = [4.0, 11.0, 1.0, 51.0, 8.5]
    d = (np.arange(20 * 8, dtype=np.float32).reshape(8, 20) - 5)
    ur, dp = oracle.stereo_from_rgbd(k, ku, d, 40.0)
    assert dp.tolist() == [38.0, 105.0, -1.0, -1.0, 142.0]           # d[2,3], d[5,10], d[0,0] = -5 (hole), outside, d[7,7]
    want = [np.float32(4.0) - np.float32(40.0) / np.float32(38.0), np.float32(11.0) - np.float32(40.0) / np.float32(105.0), -1.0, -1.0,
            np.float32(8.5) - np.float32(40.0) / np.float32(142.0)]
    assert ur.tolist() == [float(np.float32(x)) for x in want]


# ------------------------------------------------------------------ the designed window scenes (tests/window_cases.py)
# Each scene family is built to take one branch of oracle/orb_match.c; the census says whether it does.  What is asserted here is a
# condition on the scenes and the oracle alone: tests/test_gpu_window_rules.py sends the same scenes through the device entries.
AREA = ("area_min_x_beyond", "area_max_x_negative", "area_min_y_beyond", "area_max_y_negative", "area_cut_left", "area_cut_right", "area_cut_top",
        "area_cut_bottom", "area_on_edge", "area_outside", "area_inside", "area_empty_cell", "area_cell_over_64")


def _need(cen, names, where):
    missing = [n for n in names if cen[n] < 1]
    assert not missing, (where, missing)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _taken(c, assign, role):
    """(train feature, distance) the query of that role holds in a by-train table, or None"""
    q = c["roles"][role]
    t = np.nonzero(assign == q)[0]
    return (int(t[0]), int(np.unpackbits(c["qd"][q] ^ c["td"][t[0]]).sum())) if len(t) else None


def test_match_branches_are_named_once(oracle):
    assert len(oracle.MATCH_BRANCHES) == len(set(oracle.MATCH_BRANCHES)) == 84   # ORC_MATCH_NBRANCH


def test_window_scenes_keep_their_groups_apart(oracle):
    """the exact distances hold inside a group only: no window may hold a feature of another group"""
    import window_cases as wc
    scenes = [wc.proj_scene(oracle, r) for r in wc.PROJ_RUNS] + [wc.make_window_scene(oracle, True), wc.make_init_scene(oracle)]
    for c in scenes:
        assert c["nq"] <= 512 and c["nt"] <= 512
        for q in range(c["nq"]):
            got = oracle.features_in_area(c["gp"], c["tk"], c["start"], c["idx"], *c["uvr"][q], -1, -1)
            assert (c["tg"][got] == c["qg"][q]).all(), q


def test_projection_census_on_the_designed_scenes(oracle):
    import window_cases as wc
    for run in wc.PROJ_RUNS:
        c = wc.proj_scene(oracle, run)
        plain = wc.proj_oracle(oracle, c, run)
        a, occ, n, cen = wc.proj_oracle(oracle, c, run, census=True)
        assert _same(plain, (a, occ, n)), run                                   # the census changes nothing
        mode, th = run["mode"], run["th"]
        if run["ratio"] < 0.5:   # the run made for one family: at 0.2 the ratio rule rejects most of the others' matches
            assert _taken(c, a, "second at 256")[1] == 60 and cen["proj_ratio_reject"] > 10
            continue
        _need(cen, AREA + ("area_no_level_check", "area_level_below", "area_level_above"), run)
        _need(cen, ("proj_invalid", "proj_no_candidate", "proj_occupied", "proj_new_best", "proj_new_second", "proj_equal_best", "proj_equal_second",
                    "proj_best_at_th", "proj_best_above_th", "proj_none_free", "proj_single", "proj_accept", "proj_blocks", "proj_overwrites_entry"), run)
        if mode == 3:
            _need(cen, ("proj_ratio_reject", "proj_ratio_pass", "proj_ratio_equal", "proj_cross_level_pass"), run)
            # 30/40 at 0.75 is exact; 40/50 at 0.8f and 45/50 at 0.9f round to 40 and 45 in binary32: `>` does not reject
            eq = {0.75: "ratio 30/40 same", 0.8: "ratio 40/50 same", 0.9: "ratio 45/50 same"}[run["ratio"]]
            assert _taken(c, a, eq) is not None, run
            assert _taken(c, a, "second at 256")[1] == min(th, 60), run
            assert _taken(c, a, "tie same level") is None and _taken(c, a, "tie cross level") is not None
        else:
            # unreachable outside mode 3: the ratio rule is mode 3's alone (ORBmatcher.cc:120-121)
            assert cen["proj_ratio_reject"] == cen["proj_ratio_pass"] == cen["proj_ratio_equal"] == cen["proj_cross_level_pass"] == 0
            t = _taken(c, a, "tie same level")
            assert t is not None and c["tk"]["x"][t[0]] < c["uvr"][c["roles"]["tie same level"], 0] and t[0] > 0   # first in cell order, not the lower index
        if mode in (3, 4):
            _need(cen, ("proj_leaves_free", "proj_retaken"), run)
        else:
            assert cen["proj_leaves_free"] == cen["proj_retaken"] == 0             # unreachable: modes 5 / 6 always block (:1557, :375)
        if run["ori"] and mode in (4, 5):
            _need(cen, ("proj_pruned",), run)
            if mode == 4:
                _need(cen, ("proj_pruned_retaken",), run)
                assert n != (a >= 0).sum()                                          # a feature pushed twice is subtracted twice
        else:
            assert cen["proj_pruned"] == 0                                         # unreachable: no rotation check in modes 3 / 6 or without check_ori
        if run["stereo"]:
            _need(cen, ("proj_stereo_beyond", "proj_stereo_at_radius", "proj_stereo_within"), run)
            assert _taken(c, a, "stereo at r")[1] == 10 and _taken(c, a, "stereo beyond r")[1] == 30
            assert _taken(c, a, "stereo uright 0")[1] == 10 and _taken(c, a, "stereo uright -1")[1] == 10
        # what the families say in words
        for k in range(4):
            assert _taken(c, a, "edge %d" % k)[1] == 10                             # neither the feature on the edge (5) nor the far one (40)
        assert _taken(c, a, "dropped 0")[1] == 30 and _taken(c, a, "dropped 1")[1] == 30
        assert _taken(c, a, "at th")[1] == th and _taken(c, a, "at th, both sides flipped")[1] == th and _taken(c, a, "th + 1") is None
        assert _taken(c, a, "invalid") is None and _taken(c, a, "none free") is None
        assert a[np.nonzero(c["assign0"] == 7)[0][0]] == 7 and a[np.nonzero(c["assign0"] == 11)[0][0]] == 11 and a[np.nonzero(c["assign0"] == 9)[0][0]] != 9
        if not (run["ori"] and mode in (4, 5)):
            assert [_taken(c, a, "chain %d" % k)[1] for k in range(5)] == [10, 12, 14, 16, 18]   # each takes the feature after the one it preferred
            if mode in (3, 4):   # nobody blocks: the second takes what the first took, the first's entry is overwritten
                assert _taken(c, a, "free chain 0") is None and _taken(c, a, "free chain 1")[1] == 10 and _taken(c, a, "free chain 2")[1] == 20
            else:
                assert [_taken(c, a, "free chain %d" % k)[1] for k in range(3)] == [10, 20, 40]
        lv = {"levels -1,-1": 6, "levels 0,-1": 6, "levels 0,0": 30, "levels -1,0": 30, "levels 3,5": 18, "levels 7,8": 6}
        for role, d in lv.items():
            got = _taken(c, a, role)
            assert (got[1] == d) if d <= th else (got is None), (run, role)


def test_window_best_census_on_the_designed_scenes(oracle):
    import window_cases as wc
    for run in wc.WINDOW_RUNS:
        c = wc.make_window_scene(oracle, run["stereo"])
        bi, bd, cen = wc.window_oracle(oracle, c, run, census=True)
        assert _same(wc.window_oracle(oracle, c, run), (bi, bd)), run
        _need(cen, AREA + ("area_no_level_check", "win_invalid", "win_none", "win_level_below", "win_level_above", "win_new_best", "win_equal_best"), run)
        assert cen["area_level_below"] == cen["area_level_above"] == 0             # unreachable: the window is gathered with (-1, -1)
        R = c["roles"]
        if run["chi2"]:
            _need(cen, ("win_mono_reject", "win_mono_pass"), run)
            assert all(bd[R["chi2 mono %d" % o]] == 10 for o in range(8))          # the feature one step outside the gate (5) is refused
            if run["stereo"]:
                _need(cen, ("win_stereo_reject", "win_stereo_pass"), run)
                assert all(bd[R["chi2 stereo %d" % o]] == 10 for o in (0, 3, 7))
                assert bd[R["chi2 uright 0"]] == 30 and bd[R["chi2 uright -1"]] == 5   # 0 is a right coordinate, -1 is none
            else:
                assert cen["win_stereo_reject"] == cen["win_stereo_pass"] == 0     # unreachable without t_uright
        else:
            assert cen["win_mono_reject"] == cen["win_mono_pass"] == cen["win_stereo_reject"] == cen["win_stereo_pass"] == 0   # unreachable without chi2
            assert all(bd[R["chi2 mono %d" % o]] == 5 for o in range(8))
        tie = R["tie inside the gate"]
        assert bd[tie] == 20 and c["tk"]["x"][bi[tie]] < c["uvr"][tie, 0] and c["tk"]["x"][bi[tie] - 1] > c["uvr"][tie, 0]   # first in cell order, the higher index
        assert (bi[R["empty window"]], bd[R["empty window"]]) == (-1, 256) and bi[R["no level fits"]] == -1 and bi[R["invalid"]] == -1
        assert bd[R["pred 0"]] == 20 and bd[R["pred 3"]] == 20 and bd[R["pred 7"]] == 20 and bd[R["pred 7, below only"]] == 15
    # the gates' edges really are neighbours in binary32
    for o in range(8):
        p, f = wc.adjacent(lambda tx: wc._chi2_mono(30.0, tx, o), 31.0, 42.0)
        assert np.nextafter(p, np.float32(np.inf)) == f


def test_initialization_census_on_the_designed_scene(oracle):
    import window_cases as wc
    c = wc.make_init_scene(oracle)
    R = c["roles"]
    for run in wc.INIT_RUNS:
        m, n, cen = wc.init_oracle(oracle, c, run, census=True)
        assert _same(wc.init_oracle(oracle, c, run), (m, n)), run
        _need(cen, AREA + ("area_level_above",), run)
        assert cen["area_no_level_check"] == cen["area_level_below"] == 0          # unreachable: the level window is (0, 0) for an octave-0 query
        _need(cen, ("init_octave_skip", "init_no_candidate", "init_held_better", "init_held_equal", "init_new_best", "init_new_second", "init_equal_best",
                    "init_best_at_th", "init_best_above_th", "init_ratio_reject", "init_ratio_equal", "init_accept", "init_steal"), run)
        if run["ori"]:
            _need(cen, ("init_pruned", "init_prune_already_revoked"), run)
            assert m[R["lone pruned"]] == -1 and m[R["victim pruned 0"]] == -1 and m[R["victim pruned 1"]] >= 0 and m[R["victim kept 1"]] == -1
        else:
            assert cen["init_pruned"] == cen["init_prune_already_revoked"] == 0    # unreachable without check_ori
        assert n == (m >= 0).sum()
        assert m[R["steal 0"]] == -1 and m[R["steal 1"]] >= 0
        assert m[R["held better 0"]] >= 0 and m[R["held better 1"]] == -1
        assert m[R["equal 0"]] >= 0 and m[R["equal 1"]] == m[R["equal 0"]] + 1     # skipped at the equal distance: its second choice, at 50
        assert m[R["chain 0"]] == -1 and m[R["chain 1"]] == -1 and m[R["chain 2"]] >= 0
        assert R["stride 1"] - R["stride 0"] > 64 and m[R["stride 0"]] == -1 and m[R["stride 1"]] >= 0
        assert m[R["at 50 0"]] >= 0 and m[R["at 51 0"]] == -1 and m[R["equal best 0"]] == -1
        assert m[R["query octave 2"]] == -1 and c["tk"]["octave"][m[R["train octave 1"]]] == 0 and m[R["moved"]] >= 0
        for k in range(4):
            assert np.unpackbits(c["qd"][R["edge %d" % k]] ^ c["td"][m[R["edge %d" % k]]]).sum() == 10
    z = np.zeros(0, oracle.KP_DTYPE)
    m, n = oracle.search_for_initialization(np.zeros((0, 2), np.float32), 10.0, z, np.zeros((0, 32), np.uint8), c["gp"], c["tk"], c["start"], c["idx"], c["td"], 0.9, True)
    assert n == 0 and len(m) == 0
    s0, i0 = oracle.grid_build(c["gp"], z)
    m, n = oracle.search_for_initialization(c["q_xy"], 10.0, c["qk"], c["qd"], c["gp"], z, s0, i0, np.zeros((0, 32), np.uint8), 0.9, True)
    assert n == 0 and (m == -1).all()


def test_triangulation_census_on_the_designed_scene(oracle):
    import window_cases as wc
    for run in wc.TRI_RUNS:
        c = wc.make_tri_scene(oracle, run["stereo"])
        m, n, cen = wc.tri_oracle(oracle, c, run, census=True)
        assert _same(wc.tri_oracle(oracle, c, run), (m, n)), run
        assert all(cen[k] == 0 for k in cen if not k.startswith("tri_"))           # unreachable: no window is gathered here
        _need(cen, ("tri_node_one_side", "tri_skip1", "tri_match"), run)
        if run["only"]:
            _need(cen, ("tri_only_stereo_1", "tri_only_stereo_2", "tri_no_epipole_test", "tri_line_pass"), run)
            q, t = c["roles"]["only stereo"]
            assert n == 1 and m[q] == t
            continue
        assert cen["tri_only_stereo_1"] == cen["tri_only_stereo_2"] == 0           # unreachable without bOnlyStereo
        _need(cen, ("tri_skip2", "tri_above_th", "tri_above_best", "tri_equal_best", "tri_epipole_near", "tri_epipole_on", "tri_den_zero", "tri_line_fail",
                    "tri_line_pass", "tri_later_pass", "tri_equal_replaces"), run)
        if run["stereo"]:
            _need(cen, ("tri_no_epipole_test",), run)
        else:
            assert cen["tri_no_epipole_test"] == 0                                 # unreachable without a right coordinate on either side
        if run["ori"]:
            _need(cen, ("tri_pruned",), run)
        else:
            assert cen["tri_pruned"] == 0                                          # unreachable without check_ori
        for role, (q, t) in c["roles"].items():
            if role == "only stereo":
                continue
            assert m[q] == (-1 if role == "lone pruned" and run["ori"] else t), (run, role)
