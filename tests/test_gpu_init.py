"""The device Initializer (orbi_*) against the restatement (tools/init_ref.hpp via tests/init_cases.py): R21, t21, vP3D,
vbTriangulated, the return value and every diagnostic (SH, SF, RH, the winning hypotheses, their iterations and inlier
counts, every candidate's nGood and parallax) equal as bits."""

import numpy as np
import pytest

import dropin
import init_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.9, True, device=0)


def run_both(matcher, keys1, keys2, m12, model="HF", iterations=200, sigma=1.0, sets=None, K=ic.K_TUM):
    from orbslamm_amd.initializer import Initializer, make_sets
    if sets is None:
        sets = make_sets(int((m12 >= 0).sum()), iterations)
    ini = Initializer(matcher, keys1, K, sigma=sigma, iterations=iterations, model=model)
    got = ini.initialize(keys2, m12, sets)
    want = ic.ref_initialize(keys1, keys2, m12, sets, K=K, sigma=sigma, model=model)
    # Normalize of frame 1, cached at creation
    T, _ = ic.ref_normalize(keys1)
    nm = ini.normalization()
    assert nm[2] == T[0, 0] and nm[3] == T[1, 1] and np.float32(-nm[0] * nm[2]) == T[0, 2] and np.float32(-nm[1] * nm[3]) == T[1, 2]
    ini.close()
    return got, want


@pytest.mark.parametrize("model", ["HF", "F"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_general_scene_with_noise_and_outliers(matcher, model, seed):
    rng = np.random.default_rng(100 + seed)
    keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=500, n1=1000, n2=950, noise=0.5, outliers=0.3)
    got, want = run_both(matcher, keys1, keys2, m12, model=model)
    ic.assert_equal_results(got, want)
    assert want["res"]["reconstructed_h"] == 0 and want["res"]["n_candidates"] == 4
    if model == "F":
        assert want["res"]["it_H"] == -1 and want["res"]["SH"] == 0


@pytest.mark.parametrize("model", ["HF", "F"])
def test_planar_scene(matcher, model):
    rng = np.random.default_rng(7)
    keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=400, n1=800, n2=800, planar=True, noise=0.3, outliers=0.2)
    got, want = run_both(matcher, keys1, keys2, m12, model=model)
    ic.assert_equal_results(got, want)
    if model == "HF":
        assert want["res"]["reconstructed_h"] == 1 and want["res"]["n_candidates"] == 8


def test_noiseless_scenes_succeed_bit_exact(matcher):
    for planar, seed in ((False, 11), (True, 12)):
        rng = np.random.default_rng(seed)
        keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=400, n1=700, n2=650, planar=planar, noise=0.0, outliers=0.0)
        got, want = run_both(matcher, keys1, keys2, m12, model="HF")
        ic.assert_equal_results(got, want)
        assert want["ok"] and want["res"]["reconstructed_h"] == int(planar)
        assert want["triangulated"].sum() > 300


def test_all_outliers_is_false(matcher):
    rng = np.random.default_rng(21)
    keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=300, n1=500, n2=500, outliers=1.0)
    for model in ("HF", "F"):
        got, want = run_both(matcher, keys1, keys2, m12, model=model)
        ic.assert_equal_results(got, want)
        assert not want["ok"]


def test_nothing_scores_is_false_with_outputs_untouched(matcher):
    rng = np.random.default_rng(3)
    keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=60, n1=80, n2=70)
    keys2["x"], keys2["y"] = 100.0, 200.0
    for model in ("HF", "F"):
        got, want = run_both(matcher, keys1, keys2, m12, model=model, iterations=50)
        ic.assert_equal_results(got, want)
        assert not want["ok"] and want["res"]["rt_state"] == 0 and want["res"]["n_candidates"] == 0


def test_exactly_eight_matches(matcher):
    for seed in range(4):
        rng = np.random.default_rng(40 + seed)
        keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=8, n1=200, n2=180, noise=0.5, outliers=0.0)
        for model in ("HF", "F"):
            got, want = run_both(matcher, keys1, keys2, m12, model=model, iterations=30)
            ic.assert_equal_results(got, want)
            assert want["res"]["n_matches"] == 8 and not want["ok"]   # (fewer than 50 points can never initialise)


def test_large_frames_above_the_lds_tables(matcher):
    """12 000 keys per frame (above the 8 192-entry LDS tables of the projection searches): 2 000 matches"""
    rng = np.random.default_rng(77)
    keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=2000, n1=12000, n2=12000, w=1241, h=376, noise=0.5, outliers=0.3,
                                            K=np.array([718.856, 718.856, 607.1928, 185.2157], np.float32))
    for model in ("HF", "F"):
        got, want = run_both(matcher, keys1, keys2, m12, model=model, K=np.array([718.856, 718.856, 607.1928, 185.2157], np.float32))
        ic.assert_equal_results(got, want)


def test_refusals(matcher):
    from orbslamm_amd import OrbError, _lib
    from orbslamm_amd.initializer import Initializer, make_sets
    rng = np.random.default_rng(5)
    keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=100, n1=150, n2=150)
    N = int((m12 >= 0).sum())
    ini = Initializer(matcher, keys1, ic.K_TUM, iterations=20)
    few = m12.copy()
    few[np.flatnonzero(few >= 0)[7:]] = -1           # 7 matches
    with pytest.raises(OrbError) as e:
        ini.initialize(keys2, few, np.zeros((20, 8), np.int32))
    assert e.value.code == _lib.ORBX_E_UNSUPPORTED
    bad = m12.copy()
    bad[np.flatnonzero(bad >= 0)[0]] = 150          # outside frame 2
    with pytest.raises(OrbError) as e:
        ini.initialize(keys2, bad, make_sets(N, 20))
    assert e.value.code == _lib.ORBX_E_INVALID
    sets = make_sets(N, 20)
    sets[3, 2] = N                                   # outside the compacted list
    with pytest.raises(OrbError) as e:
        ini.initialize(keys2, m12, sets)
    assert e.value.code == _lib.ORBX_E_INVALID
    sets[3, 2] = -1
    with pytest.raises(OrbError) as e:
        ini.initialize(keys2, m12, sets)
    assert e.value.code == _lib.ORBX_E_INVALID
    big = np.zeros(65536, ini_dtype())
    with pytest.raises(OrbError) as e:
        ini.initialize(big, m12, make_sets(N, 20))
    assert e.value.code == _lib.ORBX_E_UNSUPPORTED
    ini.close()
    with pytest.raises(OrbError) as e:
        Initializer(matcher, keys1, ic.K_TUM, iterations=4097)
    assert e.value.code == _lib.ORBX_E_UNSUPPORTED
    with pytest.raises(OrbError) as e:
        Initializer(matcher, keys1, ic.K_TUM, iterations=0)
    assert e.value.code == _lib.ORBX_E_INVALID
    with pytest.raises(OrbError) as e:
        Initializer(matcher, np.zeros(65536, ini_dtype()), ic.K_TUM)
    assert e.value.code == _lib.ORBX_E_UNSUPPORTED
    # the handle still works after every refusal
    ini = Initializer(matcher, keys1, ic.K_TUM, iterations=20)
    sets = make_sets(N, 20)
    got = ini.initialize(keys2, m12, sets)
    want = ic.ref_initialize(keys1, keys2, m12, sets)
    ic.assert_equal_results(got, want)


def ini_dtype():
    from orbslamm_amd import KP_DTYPE
    return KP_DTYPE


def test_resident_chain_extractor_to_initialize(gpu):
    """extractor -> orbm_frame_create -> orbm_search_for_initialization_frames -> orbi_create_frame /
    orbi_initialize_frame, against the restatement on the downloaded mvKeysUn and matches"""
    from orbslamm_amd import ORBextractor, ORBmatcher, make_grid, synth
    from orbslamm_amd.initializer import Initializer, make_sets
    w, h, nf = 640, 480, 1000
    fr = synth.make_frames(w, h, 2, stream=4)
    gex = ORBextractor(2 * nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2, device=0)
    gex.extract_batch_device(*gex.upload_frames(fr))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    host = [gex.download(f) for f in range(2)]
    g = make_grid(0.0, 0.0, float(w), float(h))
    K, D0 = [517.3, 516.5, 318.6, 255.3], [0, 0, 0, 0, 0]
    m = ORBmatcher(0.9, True, device=0)
    frames = [m.frame_from_device(dk + f * cap * 28, dd + f * cap * 32, len(host[f][0]), K, D0, g) for f in range(2)]
    k0 = m.frame_keys_un(frames[0])
    k1 = m.frame_keys_un(frames[1])
    q_xy = np.stack([k0["x"], k0["y"]], axis=1).astype(np.float32)
    m12, nm = m.SearchForInitializationFrames(q_xy, 100.0, frames[0], frames[1])
    assert nm >= 8
    for model in ("HF", "F"):
        sets = make_sets(nm, 200)
        ini = Initializer(m, frames[0], K, iterations=200, model=model)
        got = ini.initialize(frames[1], m12, sets)
        want = ic.ref_initialize(k0, k1, m12, sets, K=np.array(K, np.float32), model=model)
        ic.assert_equal_results(got, want)
        # the host-array twin gives the same
        ini2 = Initializer(m, k0, K, iterations=200, model=model)
        ic.assert_equal_results(ini2.initialize(k1, m12, sets), want)
        ini.close()
        ini2.close()
    for f in frames:
        m.frame_destroy(f)


def test_initializer_dropin_on_mock_frames(gpu):
    """include/Initializer_hip.hpp (InitializerT) on mock frames (tests/cpp/init_dropin_gpu.cpp) against
    tools/init_ref.hpp, and the process's rand() stream after Initialize"""
    dropin.run(dropin.build("init_dropin_gpu"), timeout=600, marker="init dropin ok")


# ------------------------------------------------------------------------------------------------ scene families, sizes
def _device_case(matcher, case, model, iterations=200, sigma=1.0, seed=0):
    rng = np.random.default_rng(seed)
    sets = ic.random_sets(rng, int((case["m12"] >= 0).sum()), iterations)
    got, want = run_both(matcher, case["keys1"], case["keys2"], case["m12"], model=model, iterations=iterations, sigma=sigma,
                         sets=sets, K=case["K"])
    ic.assert_equal_results(got, want)
    ic.check_result(case, got, sigma=sigma, model=model)
    return got


@pytest.mark.parametrize("model", ["HF", "F"])
@pytest.mark.parametrize("family", ic.FAMILIES)
def test_scene_families_on_the_device(matcher, family, model):
    """every family of init_cases (motions, planes, rotation only, coincident rays, shared keys, keys outside the image,
    collapsed frames), noiseless, noisy and with outliers: bits equal to the restatement, and the float64 check"""
    import zlib
    for variant in ic.VARIANTS:
        rng = np.random.default_rng(zlib.crc32(("%s/%s/%d" % (family, variant, 0)).encode()))
        case = ic.make_case(family, rng, variant)
        _device_case(matcher, case, model, seed=1)


K_ODD = np.array([700.0, 540.0, 330.5, 238.25], np.float32)           # fx != fy


# (matches, iterations, sigma, family, K): the score blocks (256 threads), CheckRT blocks (128), fit blocks (32
# hypotheses), iterations up to ORBI_MAX_ITERATIONS; frame 1 holds a third more keys than matches, frame 2 a quarter
SWEEP = [(8, 1, 1.0, "lateral", ic.K_TUM), (9, 8, 0.5, "plane_slanted", K_ODD), (127, 31, 2.0, "lateral", K_ODD),
         (128, 32, 1.0, "forward", ic.K_TUM), (129, 33, 0.5, "plane_fronto", K_ODD), (255, 257, 1.0, "wide_inward", ic.K_TUM),
         (256, 4096, 2.0, "lateral", K_ODD), (257, 200, 1.0, "plane_slanted", ic.K_TUM), (511, 31, 0.5, "coincident_rays", K_ODD),
         (513, 4096, 1.0, "plane_fronto", ic.K_TUM), (4097, 33, 2.0, "large_rotation", K_ODD), (20000, 257, 1.0, "lateral", ic.K_TUM)]


@pytest.mark.parametrize("n,iterations,sigma,family,K", SWEEP, ids=["%d-%d-%g-%s" % s[:4] for s in SWEEP])
def test_sizes_iterations_sigmas_and_intrinsics(matcher, n, iterations, sigma, family, K):
    rng = np.random.default_rng(n + iterations)
    case = ic.make_case(family, rng, "outliers" if n >= 50 else "noisy", n_match=n, K=K)
    for model in ("HF", "F"):
        _device_case(matcher, case, model, iterations=iterations, sigma=sigma, seed=n)


def test_device_reaches_the_branches_the_mutations_would_break(matcher):
    """the device takes ReconstructH's d1/d2 exit (pure rotation), stores unflagged points (cosParallax >= 0.99998) and
    selects a negative cosParallax (rays more than 90 degrees apart), each bit-equal to the restatement"""
    import zlib
    for family, want in (("rotation", "d1/d2 early exit"), ("coincident_rays", "stored but not flagged"),
                         ("wide_inward", "negative cosParallax selected")):
        rng = np.random.default_rng(zlib.crc32(("%s/%s/%d" % (family, "clean", 0)).encode()))
        got = _device_case(matcher, ic.make_case(family, rng, "clean"), "HF", seed=1)
        assert want in ic.outcomes(got), (family, ic.outcomes(got))
