"""The designed rotation-consistency cases of tests/matcher_cases.py (ROT_CLASSES: ties between bins, shifting maxima, the 10 % rule at
and around its threshold, 65 matches in one bin) through every device entry that prunes by ComputeThreeMaxima and takes the caller's
angles, byte for byte against the same oracle calls tests/test_rot_rule_cpu.py checks the design with:
    match_bruteforce (k_match_accept + k_match_prune), SearchByBoW and SearchForTriangulation (k_prune_flat),
    SearchForInitialization (k_init_resolve), SearchByProjection mode 4 (k_proj_resolve),
    FrameSet.search_by_bow (k_bow_prune_set), FrameSet.track_projected (k_track_resolve).
(The stream matcher's k_match_accept_prune takes its angles from the extractor: tests/test_gpu_extractor.py.)"""
import numpy as np
import pytest

from matcher_cases import ROT_CLASSES, assert_rot_case_is_designed, make_rot_case, rot_oracle_entries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rot_cases(oracle):
    """name -> (case, {oracle entry: ((table, n) without the check, (table, n) with it)}): computed once, read by every test"""
    out = {}
    for name in ROT_CLASSES:
        c = make_rot_case(oracle, name)
        out[name] = (c, {e: (call(False), call(True)) for e, call in rot_oracle_entries(oracle, c).items()})
    return out


def _device_entries(c):
    from orbslamm_amd import ORBmatcher, make_grid
    g = make_grid(0.0, 0.0, c["w"], c["h"])
    z8, m1 = np.zeros(c["n"], np.uint8), np.full(c["n"], -1, np.int32)

    def proj(m):
        a, _, n = m.SearchByProjection(4, 100, c["uvr"], c["lvl"], c["qd"], c["qa"], None, None, g, c["k2"], c["td"], z8, m1)
        return a, n
    return {
        "match_bruteforce": (0.7, lambda m: m.match_bruteforce(c["qd"], c["qa"], c["td"], c["ta"])),
        "search_by_bow": (0.7, lambda m: m.SearchByBoW(c["qd"], c["qa"], None, c["fv"], c["td"], c["ta"], None, c["fv"], True)),
        "search_for_triangulation": (0.6, lambda m: m.SearchForTriangulation(c["k1"], c["qd"], z8, c["fv"], c["k2"], c["td"], z8, c["fv"], c["F"], c["ex"], c["ey"],
                                                                             c["sf2"], c["sigma2"])),
        "search_for_initialization": (0.9, lambda m: m.SearchForInitialization(c["q_xy"], 30.0, c["k1"], c["qd"], g, c["k2"], c["td"])),
        "search_by_projection": (0.9, proj),
    }, ORBmatcher


@pytest.mark.parametrize("entry", ["match_bruteforce", "search_by_bow", "search_for_triangulation", "search_for_initialization", "search_by_projection"])
def test_designed_rotation_cases_through_the_host_array_entries(gpu, rot_cases, entry):
    for name, (c, want) in rot_cases.items():
        calls, ORBmatcher = _device_entries(c)
        ratio, call = calls[entry]
        got = []
        for ori in (False, True):
            m = ORBmatcher(ratio, ori, device=0)
            table, n = call(m)
            m.close()
            wt, wn = want[entry][ori]
            assert n == wn and np.array_equal(table[:c["n"]], wt[:c["n"]]), (name, ori, n, wn)
            got.append((table, n))
        assert_rot_case_is_designed(c, *got)


def test_designed_rotation_cases_through_a_frame_set(gpu, oracle, rot_cases):
    """slot 0 holds the frame whose angles are 30 * b (the KeyFrame of SearchByBoW, LastFrame of the projection search), slot 1 its
    twin with angle 0; the FeatureVectors are the vocabulary's (twins share their descriptor, so their node)"""
    from orbslamm_amd import ORBextractor, ORBmatcher, ORBVocabulary, make_grid
    from vocab_cases import make_vocab
    voc = make_vocab(np.random.default_rng(5), 10, 4, stop_fraction=0.0)   # (no stop words: every feature is in its frame's FeatureVector)
    G = ORBVocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
    O = oracle.Vocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=1, device=0)   # (its handle owns the raw device buffers)
    m = ORBmatcher(0.7, True, device=0)
    cap = 320
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    for name, (c, want) in rot_cases.items():
        n, g = c["n"], make_grid(0.0, 0.0, c["w"], c["h"])
        keys = np.zeros((2, cap), dtype=oracle.KP_DTYPE)
        desc = np.zeros((2, cap, 32), np.uint8)
        keys[0, :n], keys[1, :n], desc[0, :n], desc[1, :n] = c["k1"], c["k2"], c["qd"], c["td"]
        dk = gex.upload_frames(keys.view(np.uint8).reshape(1, 1, -1))[0]
        dd = gex.upload_frames(desc.reshape(1, 1, -1))[0]
        dc = gex.upload_frames(np.array([n, n], np.int32).view(np.uint8).reshape(1, 1, -1))[0]
        fs = m.frame_set(2, cap, [500.0, 500.0, 320.0, 240.0], [0, 0, 0, 0, 0], g, [0.0, c["w"], 0.0, c["h"]], sf)
        fs.build(0, 2, dk, dd, dc, cap)
        fs.compute_bow(G, 0, 2, 2)
        fvq, fvt = O.transform(c["qd"], 2)[1], O.transform(c["td"], 2)[1]
        bow, trk = [], []
        for ori in (False, True):
            fs.search_by_bow([0], [1], nnratio=0.7, check_ori=ori)
            match, nm = fs.bow_results()
            wt, wn = oracle.search_by_bow(c["qd"], c["qa"], None, fvq, c["td"], c["ta"], None, fvt, 0.7, ori, True)
            assert nm[0] == wn and np.array_equal(match[0, :n], wt[:n]), (name, "search_by_bow", ori, nm[0], wn)
            bow.append((match[0, :n].copy(), int(nm[0])))
            fs.track_projected(1, 0, c["uvr"], c["lvl"], None, None, None, th_dist=100, nnratio=0.9, check_ori=ori, mode=4)
            assign, nt = fs.results()
            wt, wn = want["search_by_projection"][ori]
            assert nt[0] == wn and np.array_equal(assign[0, :n], wt[:n]), (name, "track_projected", ori, nt[0], wn)
            trk.append((assign[0, :n].copy(), int(nt[0])))
        assert_rot_case_is_designed(c, *bow)
        assert_rot_case_is_designed(c, *trk)
        fs.close()
    m.close(); G.close(); gex.close()
