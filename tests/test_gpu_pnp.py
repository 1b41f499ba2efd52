"""The device PnPsolver (orbp_*) against the restatement (tools/pnp_ref.hpp via tests/pnp_cases.py) as bits: every
hypothesis's inlier count, R and t (binary64, NaNs by their bits), record flag, Refine count, flag and pose, and for each
iterate of a replay every field and the mask -- over the scene families, sizes (LDS-staged and streamed scoring),
iteration counts, batches, hand-made sets, both parameter sets and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dropin
import pnp_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.9, True, device=0)


def run_case(matcher, case, seed=0, step=5, what="", extra=None):
    from orbslamm_amd.pnp import EXTRA_SETS, run_all
    dev = pc.device_solver(matcher, case)
    # iterate(step) entered below mRansacMaxIts can reach hypothesis mRansacMaxIts + step - 2
    sets = pc.case_sets(case, dev.max_iterations + (max(EXTRA_SETS, step) if extra is None else extra), seed)
    run_all([dev], [sets])
    outs = pc.compare_solver(dev, case, sets, step, what)
    dev.close()
    return outs


@pytest.mark.parametrize("name", sorted(pc.FAMILIES))
def test_families_bit_exact(matcher, name):
    returned = 0
    for seed in (0, 1, 2):
        case = pc.family_case(name, seed)
        outs = run_case(matcher, case, seed, what="%s seed %d" % (name, seed))
        returned += sum(r["returned"] for r in outs)
        for r in outs:
            if r["returned"]:
                (rot, te), (outside, share, _) = pc.check64(case, r)
                assert outside == 0 and share <= pc.BAND_SHARE_CAP, (name, seed, outside, share)
                if pc.FAMILIES[name][1]:
                    assert rot <= pc.TOL_ROT and te <= pc.TOL_T, (name, seed, rot, te)
    if pc.FAMILIES[name][1]:
        assert returned >= 3
    if name in ("n_below_min", "wrong_60"):
        assert returned == 0


def test_families_with_the_other_parameter_set(matcher):
    for name in ("general", "wrong_20", "mixed_octaves", "planar"):
        case = pc.family_case(name, 4, ransac=pc.DEFAULTS if pc.FAMILIES[name][0].get("ransac", pc.TRACKING) == pc.TRACKING else pc.TRACKING)
        run_case(matcher, case, 4, what=name + " other parameters")


def test_repeated_and_degenerate_sets(matcher):
    case = pc.family_case("general", 0)
    case["ransac"] = (0.99, 10, 6, 4, 0.5, 5.991)
    dev = pc.device_solver(matcher, case)
    sets = np.array([[5, 5, 5, 5], [3, 3, 9, 9], [9, 3, 3, 1], [7, 8, 7, 2], [1, 2, 3, 4], [4, 4, 4, 6], [10, 20, 30, 40], [11, 21, 31, 41],
                     [12, 22, 32, 42], [13, 23, 33, 43]], np.int32)
    dev.run(sets)
    pc.compare_solver(dev, case, sets, 1, "repeated sets")
    dev.close()


@pytest.mark.parametrize("n,min_inliers,max_its", [(4, 4, 300), (5, 4, 300), (11, 10, 300), (20, 10, 300), (63, 10, 64), (64, 10, 65), (65, 10, 1),
                                                   (100, 10, 300), (500, 10, 300), (2048, 20, 300), (2049, 20, 300), (3000, 50, 1000),
                                                   (20000, 100, 4096), (20000, 10, 40)])
def test_sizes_and_iteration_counts(matcher, n, min_inliers, max_its):
    # epsilon 0.02 lets max_its decide the count for the large cases; the small ones keep Tracking's 0.5
    eps = 0.5 if max_its == 300 else 0.02
    case = pc.family_case("wrong_20" if n >= 20 else "general", 5, n=n, ransac=(0.99, min_inliers, max_its, 4, eps, 5.991))
    dev = pc.device_solver(matcher, case)
    if (n, max_its) in ((20, 300), (100, 300), (500, 300)):
        assert dev.max_iterations == 35
    if max_its == 4096:
        assert dev.max_iterations == 4096
    dev.close()
    run_case(matcher, case, 5, step=max(1, max_its // 7), what="n %d" % n)


@pytest.mark.parametrize("count", [1, 7, 32])
def test_batches_of_unequal_solvers_equal_their_solo_runs(matcher, count):
    from orbslamm_amd.pnp import EXTRA_SETS, run_all
    rng = np.random.default_rng(count)
    names = sorted(pc.FAMILIES)
    cases = []
    for c in range(count):
        name = names[(c * 5 + count) % len(names)]
        over = {} if name.startswith("n_") else dict(n=int(rng.choice([20, 37, 100, 333, 2048, 2500])))
        cases.append(pc.family_case(name, c, **over))
    devs = [pc.device_solver(matcher, case) for case in cases]
    sets = [pc.case_sets(case, d.max_iterations + EXTRA_SETS + (c % 3), seed=c) for c, (case, d) in enumerate(zip(cases, devs))]
    run_all(devs, sets)
    tables = []
    for c, (case, d) in enumerate(zip(cases, devs)):
        tables.append(d.hypotheses().copy())
        pc.compare_solver(d, case, sets[c], 5, "batch of %d, solver %d" % (count, c))
    for c, (case, d) in enumerate(zip(cases, devs)):
        solo = pc.device_solver(matcher, case)
        solo.run(sets[c])
        pc.assert_same_table(solo.hypotheses(), tables[c], "solo %d" % c)
        solo.close()
        d.close()
    assert len({len(t) for t in tables}) > 1 or count == 1


def test_or_loop_overshoot_and_capacity(matcher):
    from orbslamm_amd._lib import ORBX_E_CAPACITY, OrbError
    case = pc.family_case("wrong_60", 1)
    dev = pc.device_solver(matcher, case)
    its = dev.max_iterations
    sets = pc.case_sets(case, its + 3, 1)             # one short of what iterate(5) from its - 1 can reach
    dev.run(sets)
    ref = pc.ref_solve(case, sets=sets)
    g, w = dev.iterate(its - 1), ref.iterate(its - 1)
    # the first call runs to mRansacMaxIts whatever nIterations says (the loop is an OR)
    pc.assert_same_result(g, w, "first call")
    assert g["iterations"] == its and g["no_more"]
    g, w = dev.iterate(3), ref.iterate(3)             # past mRansacMaxIts: three more hypotheses
    pc.assert_same_result(g, w, "overshoot")
    assert g["iterations"] == its + 3
    with pytest.raises(OrbError) as e:
        dev.iterate(1)                                # would read set its + 3
    assert e.value.code == ORBX_E_CAPACITY and ref.iterate(1)["rc"] == -4
    g, w = dev.iterate(0), ref.iterate(0)             # state untouched by the refusal
    pc.assert_same_result(g, w, "after the refusal")
    assert g["iterations"] == its + 3
    dev.close()


def test_refusals(matcher):
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, OrbError
    from orbslamm_amd.pnp import EXTRA_SETS, run_all
    case = pc.family_case("general", 0)

    def code(fn):
        with pytest.raises(OrbError) as e:
            fn()
        return e.value.code
    bad = dict(case)
    bad["idx"] = case["idx"].copy()
    bad["idx"][3] = case["n_all"]
    assert code(lambda: pc.device_solver(matcher, bad)) == ORBX_E_INVALID
    dev = pc.device_solver(matcher, case)
    its = dev.max_iterations
    good = pc.case_sets(case, its + EXTRA_SETS)
    assert code(lambda: dev.iterate(1)) == ORBX_E_INVALID            # no table yet
    for v in (-1, dev.n):
        s = good.copy()
        s[its // 2, 1] = v
        assert code(lambda: run_all([dev], [s])) == ORBX_E_INVALID
    assert code(lambda: run_all([dev, dev], [good, good])) == ORBX_E_INVALID
    assert code(lambda: dev.set_ransac(0.999999999, 10, 5000, 4, 0.01, 5.991)) == ORBX_E_UNSUPPORTED   # above ORBP_MAX_ITERATIONS
    assert code(lambda: dev.set_ransac(0.99, 10, 300, 5, 0.5, 5.991)) == ORBX_E_UNSUPPORTED            # min_set != 4
    assert dev.max_iterations == its                                                                  # (a refusal changes nothing)
    other = __import__("orbslamm_amd").ORBmatcher(0.9, True, device=0)
    dev2 = pc.device_solver(other, case)
    assert code(lambda: run_all([dev, dev2], [good, good])) == ORBX_E_INVALID
    big = pc.family_case("general", 0, n=65536, n_all=65536)
    assert code(lambda: pc.device_solver(matcher, big)) == ORBX_E_UNSUPPORTED
    empty = pc.family_case("general", 0, n=0, n_all=4)
    assert code(lambda: pc.device_solver(matcher, empty)) == ORBX_E_UNSUPPORTED
    # a solver below min_inliers is allowed in a batch and says bNoMore
    few = pc.device_solver(matcher, pc.family_case("n_below_min", 0))
    run_all([few, dev], [None, good])
    assert few.iterate(3)["no_more"] and len(few.hypotheses()) == 0
    pc.compare_solver(dev, case, good, 5)
    dev.set_ransac(*case["ransac"])                                     # drops the table, rewinds nothing
    assert code(lambda: run_all([dev], [good])) == ORBX_E_UNSUPPORTED   # it has iterated and has no table to continue


def test_pnp_dropin_on_mock_frames(gpu):
    """include/PnPsolver_hip.hpp (PnPsolverT, RunAll) on a mock frame (tests/cpp/pnp_dropin_gpu.cpp) through
    Tracking::Relocalization's round-robin loop against tools/pnp_ref.hpp, and the process's rand() position after RunAll"""
    dropin.run(dropin.build("pnp_dropin_gpu"), timeout=600, marker="pnp dropin ok")


def test_soak_slice(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "soak", "fuzz_pnp.py"), "40", "211"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pnp soak: 40 cases" in out.stdout and "equal" in out.stdout


def test_create_frame_equals_create_on_the_same_data(gpu):
    """orbp_create_frame gathers P2D and sigma2 from a device-resident frame's undistorted keys: the same table, bit for
    bit, as orbp_create on the downloaded keys, and as the restatement"""
    from orbslamm_amd import ORBextractor, ORBmatcher, make_grid, synth
    from orbslamm_amd.pnp import EXTRA_SETS, PnPsolver, make_pnp_sets
    w, h, nf = 640, 480, 1000
    rng = np.random.default_rng(77)
    fr = synth.make_frames(w, h, 1, stream=2)
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=1, device=0)
    gex.extract_batch_device(*gex.upload_frames(fr))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    k0, _ = gex.download(0)
    m = ORBmatcher(0.75, True, device=0)
    F = m.frame_from_device(dk, dd, len(k0), pc.K_TUM, [0.1, -0.05, 0.001, 0.0005, 0.0], make_grid(0.0, 0.0, float(w), float(h)))
    ku = m.frame_keys_un(F)
    assert len(ku) == len(k0) > 300 and not np.array_equal(ku["x"], k0["x"])       # (distorted camera: the undistorted keys are the frame's)
    # map points: the matched keys unprojected at seeded depths under a true pose, a fifth of the matches wrong
    idx = np.sort(rng.choice(len(ku), 240, replace=False)).astype(np.int32)
    R, t = pc.rot_axis_angle([0.2, 1, 0.1], 0.3), np.array([0.2, -0.1, 0.5])
    z = rng.uniform(3, 9, len(idx))
    K = pc.K_TUM.astype(np.float64)
    src = idx.copy()
    wrong = rng.uniform(size=len(idx)) < 0.2
    src[wrong] = rng.integers(0, len(ku), int(wrong.sum()))
    Xc = np.stack([(ku["x"][src].astype(np.float64) - K[2]) / K[0] * z, (ku["y"][src].astype(np.float64) - K[3]) / K[1] * z, z], axis=1)
    P3Dw = ((Xc - t) @ R).astype(np.float32)
    lev = pc.SIGMA2
    case = dict(n_all=len(ku), idx=idx, P2D=np.stack([ku["x"][idx], ku["y"][idx]], axis=1), sigma2=lev[ku["octave"][idx]], P3Dw=P3Dw, K=pc.K_TUM,
                ransac=pc.TRACKING)
    a = PnPsolver(m, 0, idx, None, None, P3Dw, pc.K_TUM, frame=F, level_sigma2=lev)
    b = pc.device_solver(m, case)
    assert (a.n, a.n_all) == (b.n, b.n_all) == (240, len(ku))
    a.set_ransac(*pc.TRACKING)
    sets = make_pnp_sets(a.n, a.max_iterations + EXTRA_SETS, seed=9)
    a.run(sets)
    b.run(sets)
    pc.assert_same_table(a.hypotheses(), b.hypotheses(), "frame against arrays")
    outs = pc.compare_solver(a, case, sets, 5, "resident frame")
    assert any(r["returned"] and r["n_inliers"] > 150 for r in outs)
    a.close()
    b.close()
    m.frame_destroy(F)


def test_relocalisation_chain_to_the_projection_search(gpu, oracle):
    """Tracking::Relocalization's chain on device-resident data: extractor -> frame set -> Frame::ComputeBoW ->
    DetectRelocalizationCandidates (orbk) -> SearchByBoW(KF, F) per candidate -> PnPsolver on the matched map points, built
    from the resident frame (orbp_create_frame), all candidates in one orbp_run, iterate(5) in turn -> with the returned
    pose SearchByProjection(F, KF, sFound, 10, 100) on the resident frame.  Against the same chain with the restatements
    and the oracle in every place: kfdb_cases' database, the oracle's SearchByBoW, tools/pnp_ref.hpp, the oracle's
    SearchByProjection fed with the RESTATEMENT's pose."""
    import kfdb_cases as kc
    from vocab_cases import make_vocab
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool, ORBextractor, ORBmatcher, ORBVocabulary, make_grid, synth
    from orbslamm_amd.pnp import EXTRA_SETS, PnPsolver, make_pnp_sets, run_all
    f32, f64 = np.float32, np.float64
    rng = np.random.default_rng(29)
    k, L, levelsup = 10, 4, 2
    v = make_vocab(rng, k, L)
    G = ORBVocabulary(k, L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)
    O = oracle.Vocabulary(k, L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"])
    w, h, nf, B = 640, 480, 1000, 6
    fr = synth.make_frames(w, h, B, stream=4)
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B, device=0)
    gex.extract_batch_device(*gex.upload_frames(fr))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    host = [gex.download(f) for f in range(B)]
    sf = np.array(gex.GetScaleFactors(), f32)
    lev_sigma2 = (sf * sf).astype(f32)
    m = ORBmatcher(0.75, True, device=0)
    g = make_grid(0.0, 0.0, float(w), float(h))
    fs = m.frame_set(B, gex.max_keypoints, pc.K_TUM, [0, 0, 0, 0, 0], g, [0.0, float(w), 0.0, float(h)], sf)
    fs.build_from_extractor(0, gex)
    fs.compute_bow(G, 0, B, levelsup)
    pool = KeyFramePool(G)
    db, ref_db, kfs = KeyFrameDatabase(pool), kc.Database(), []
    for s in range(B - 1):                     # slots 0..4 are keyframes, slot 5 is the lost frame F
        pool.set_bow_from_frameset(s, fs, s)
        kfs.append(kc.KeyFrame(s, *fs.bow_vector(s)))
        db.add(s)
        ref_db.add(kfs[s])
    covis = {s: [j for j in range(B - 1) if j != s][:3] for s in range(B - 1)}
    cands = db.DetectRelocalizationCandidates(3, frameset=fs, fs_slot=B - 1, neighbours=covis.get)
    want_c, _ = ref_db.DetectRelocalizationCandidates(kc.Query(3, *fs.bow_vector(B - 1)), lambda kf: [kfs[j] for j in covis[kf.slot]])
    assert cands and cands == [kf.slot for kf in want_c]
    fs.search_by_bow(cands, [B - 1] * len(cands), nnratio=0.75, check_ori=True)
    match, nm = fs.bow_results()
    kt, dt = host[B - 1]
    nt = len(kt)
    _, fv_t = O.transform(dt, levelsup)
    # the lost frame as a resident frame (zero distortion: its undistorted keys are its keys)
    F = m.frame_from_device(dk + (B - 1) * cap * 28, dd + (B - 1) * cap * 32, nt, pc.K_TUM, [0, 0, 0, 0, 0], g)
    K = pc.K_TUM.astype(f64)
    Rt, tt = pc.rot_axis_angle([0.1, 1, 0.2], 0.25), np.array([0.3, -0.1, 0.4])
    depth = rng.uniform(3, 9, nt)
    XF = np.stack([(kt["x"].astype(f64) - K[2]) / K[0] * depth, (kt["y"].astype(f64) - K[3]) / K[1] * depth, depth], axis=1)
    XFw = ((XF - tt) @ Rt).astype(f32)          # the world point behind every key of F under F's true pose
    m2 = ORBmatcher(0.9, True, device=0)
    gp = oracle.make_grid_params(0.0, 0.0, float(w), float(h))
    start, gidx = oracle.grid_build(gp, kt)
    devs, refs, cases, setss, kfpts = [], [], [], [], []
    for p, c in enumerate(cands):
        kq, dq = host[c]
        _, fv_q = O.transform(dq, levelsup)
        wm, wn = oracle.search_by_bow(dq, kq["angle"], None, fv_q, dt, kt["angle"], None, fv_t, 0.75, True, True)
        assert nm[p] == wn and np.array_equal(match[p, :nt], wm)
        # every key of the keyframe holds a map point: the one behind the F key it matched (a fifth replaced: wrong matches),
        # or behind a random F key where it matched nothing (what SearchByProjection can still find)
        P = XFw[rng.integers(0, nt, len(kq))].copy()
        idx = np.flatnonzero(wm >= 0).astype(np.int32)          # vpMapPointMatches: per key of F, the keyframe's key
        good = rng.uniform(size=len(idx)) >= 0.2
        P[wm[idx[good]]] = XFw[idx[good]]
        kfpts.append(P)
        case = dict(n_all=nt, idx=idx, P2D=np.stack([kt["x"][idx], kt["y"][idx]], axis=1), sigma2=lev_sigma2[kt["octave"][idx]],
                    P3Dw=P[wm[idx]], K=pc.K_TUM, ransac=pc.TRACKING)
        d = PnPsolver(m, 0, idx, None, None, case["P3Dw"], pc.K_TUM, frame=F, level_sigma2=lev_sigma2)
        d.set_ransac(*pc.TRACKING)
        s = make_pnp_sets(d.n, d.max_iterations + EXTRA_SETS, seed=p) if d.n >= d.min_inliers else None
        devs.append(d); cases.append(case); setss.append(s)
        refs.append(pc.ref_solve(case, sets=s))
    run_all(devs, setss)
    found = 0
    for p, c in enumerate(cands):
        kq, dq = host[c]
        got = want = None
        for _ in range(20):                                     # iterate(5) until a pose or bNoMore, as Relocalization does
            got, want = devs[p].iterate(5), refs[p].iterate(5)
            pc.assert_same_result(got, want, "candidate %d" % c)
            if want["returned"] or want["no_more"]:
                break
        if not want["returned"]:
            continue
        found += 1

        def search(res, dev):
            # mvpMapPoints of F from the inliers; sFound; then SearchByProjection(F, KF, sFound, 10, 100) (ORBmatcher.cc:1474-1601):
            # the keyframe's other map points through the pose, radius 10 * scale of the key's level, levels +-1
            T = res["Tcw"]
            inl = np.flatnonzero(res["inliers"])
            wm = match[p, :nt]
            sfound = np.zeros(len(kq), bool)
            sfound[wm[inl]] = True
            Xc = (kfpts[p] @ T[:3, :3].T + T[:3, 3]).astype(f32)
            ok = (Xc[:, 2] > 0) & ~sfound
            invz = f32(1) / np.where(Xc[:, 2] > 0, Xc[:, 2], f32(1))
            u, vv = pc.K_TUM[0] * Xc[:, 0] * invz + pc.K_TUM[2], pc.K_TUM[1] * Xc[:, 1] * invz + pc.K_TUM[3]
            ok &= (u >= 0) & (u < w) & (vv >= 0) & (vv < h)
            lvl = np.clip(kq["octave"], 0, 7)
            uvr = np.stack([u, vv, f32(10) * sf[lvl]], axis=1).astype(f32)[ok]
            ql = np.stack([lvl - 1, lvl + 1], axis=1).astype(np.int8)[ok]
            occ = np.zeros(nt, np.uint8)
            occ[inl] = 1
            asg = np.full(nt, -1, np.int32)
            if dev:
                return m2.SearchByProjectionFrame(5, 100, uvr, ql, dq[ok], kq["angle"][ok], None, None, F, occ, asg), int(ok.sum())
            return oracle.search_by_projection(5, 0.9, True, 100, uvr, ql, dq[ok], kq["angle"][ok], None, None, gp, kt, start, gidx, dt, occ, asg), int(ok.sum())
        (ga, go, gn), nq = search(got, True)
        (wa, wo, wn2), _ = search(want, False)
        assert gn == wn2 and np.array_equal(ga, wa) and np.array_equal(go, wo) and nq > 100
    assert found >= 1
    for d in devs:
        d.close()
    m.frame_destroy(F)
    fs.close()


def test_a_table_is_continued_past_the_sets_drawn_first(matcher):
    """a candidate whose Refine returns the caller rejects stays live past mRansacMaxIts (a Refine return never sets
    bNoMore): orbp_iterate refuses the call that would pass the table, the caller gives more sets, orbp_run continues the
    table with the state kept, and every call equals the restatement's on the concatenated sets"""
    from orbslamm_amd._lib import ORBX_E_CAPACITY, OrbError
    for name, seed in (("wrong_20", 3), ("mixed_octaves", 1), ("behind_camera", 2), ("wrong_60", 0)):
        case = pc.family_case(name, seed)
        dev = pc.device_solver(matcher, case)
        its = dev.max_iterations
        chunks = [pc.case_sets(case, its + 4, seed)] + [pc.case_sets(case, 9, 100 + k) for k in range(12)]
        ref = pc.ref_solve(case, sets=np.concatenate(chunks))
        dev.run(chunks[0])
        have, used, calls = len(chunks[0]), 1, 0
        while used < len(chunks):
            try:
                g = dev.iterate(5)
            except OrbError as e:
                assert e.code == ORBX_E_CAPACITY
                dev.extend(chunks[used])
                have += len(chunks[used])
                used += 1
                continue
            w = ref.iterate(5)
            assert w["rc"] == 0
            pc.assert_same_result(g, w, "%s call %d" % (name, calls))
            calls += 1
        assert g["iterations"] > its + 4 + 9 * 10 and len(dev.sets) == have
        full = pc.ref_solve(case, sets=dev.sets)
        pc.assert_same_table(dev.hypotheses(), full.all_hypotheses(), name + " continued table")
        dev.close()
