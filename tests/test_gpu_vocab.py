"""GPU parity of ORBVocabulary::transform (through the C ABI) against the oracle."""
import numpy as np
import pytest

from vocab_cases import make_vocab, write_text

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scoring,weighting", [(0, 0), (1, 1), (5, 0), (0, 2), (5, 3), (3, 0)])
def test_transform_parity(gpu, oracle, scoring, weighting):
    from orbslamm_amd import ORBVocabulary
    rng = np.random.default_rng(60 + scoring * 4 + weighting)
    for k, L, n in ((10, 3, 2000), (6, 4, 333), (3, 6, 1), (10, 4, 4097)):
        voc = make_vocab(rng, k, L)
        G = ORBVocabulary(k, L, scoring, weighting, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
        O = oracle.Vocabulary(k, L, scoring, weighting, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
        desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        for levelsup in (4, 0, L + 2):
            (gi, gv), (gn, gs, gx) = G.transform(desc, levelsup)
            (oi, ov), (on, os_, ox) = O.transform(desc, levelsup)
            assert np.array_equal(gi, oi)
            assert gv.tobytes() == ov.tobytes()   # double values bit-for-bit
            assert np.array_equal(gn, on) and np.array_equal(gs, os_) and np.array_equal(gx, ox)
        assert len(oi) > 0


def test_text_loader_and_bow_search(gpu, oracle, tmp_path):
    """ORBvoc.txt-format file -> transform -> FeatureVector drives SearchByBoW"""
    from orbslamm_amd import ORBmatcher, ORBVocabulary
    from matcher_cases import noisy_copies
    rng = np.random.default_rng(77)
    voc = make_vocab(rng, 10, 3, ragged=False)
    path = tmp_path / "voc.txt"
    write_text(path, voc, 0, 0)
    G = ORBVocabulary.loadFromTextFile(path)
    O = oracle.Vocabulary(10, 3, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    base = rng.integers(0, 256, size=(800, 32), dtype=np.uint8)
    d1, d2 = noisy_copies(rng, base, 6), noisy_copies(rng, base, 6)[rng.permutation(800)]
    (w1, v1), fv1 = G.transform(d1, 2)
    (w2, v2), fv2 = G.transform(d2, 2)
    (ow1, ov1), ofv1 = O.transform(d1, 2)
    assert np.array_equal(w1, ow1) and v1.tobytes() == ov1.tobytes() and all(np.array_equal(a, b) for a, b in zip(fv1, ofv1))
    ang = np.zeros(800, np.float32)
    m = ORBmatcher(0.8, False, device=0)
    got, n = m.SearchByBoW(d1, ang, None, fv1, d2, ang, None, fv2, True)
    want, nw = oracle.search_by_bow(d1, ang, None, fv1, d2, ang, None, fv2, 0.8, False, True)
    assert n == nw and np.array_equal(got, want) and n > 300


def test_bad_vocabulary_is_rejected(gpu):
    from orbslamm_amd import ORBVocabulary, OrbError
    with pytest.raises(OrbError):
        ORBVocabulary(10, 3, 0, 0, np.array([5], np.int32), np.array([1], np.uint8), np.zeros((1, 32), np.uint8), np.ones(1), device=0)
    with pytest.raises(OrbError):
        ORBVocabulary(99, 3, 0, 0, np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((0, 32), np.uint8), np.zeros(0), device=0)


def test_tracking_front_end_stays_in_hbm(gpu, oracle):
    """SURVEY 8(f).2+3 together: frames extracted on the GPU never leave it -- the matcher builds their Frame state
    from the device pointers, Frame::ComputeBoW runs on the device-resident descriptors, and SearchByBoW (the
    TrackReferenceKeyFrame search) runs between the two device frames.  BowVector, and matches against the oracle
    fed with the downloaded arrays."""
    from orbslamm_amd import ORBextractor, ORBmatcher, ORBVocabulary, make_grid, synth
    w, h, nf = 640, 480, 1000
    rng = np.random.default_rng(91)
    voc = make_vocab(rng, 10, 4)
    G = ORBVocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
    O = oracle.Vocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    fr = synth.make_frames(w, h, 2, stream=4)
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2, device=0)
    gex.extract_batch_device(*gex.upload_frames(fr))
    gex.sync()
    dk, dd, _, cap = gex.device_results()
    host = [gex.download(f) for f in range(2)]
    g = make_grid(0.0, 0.0, float(w), float(h))
    K, D0 = [517.3, 516.5, 318.6, 255.3], [0, 0, 0, 0, 0]
    for ratio, ori, by_train in ((0.7, True, True), (0.75, True, False), (0.9, False, True)):
        m = ORBmatcher(ratio, ori, device=0)
        frames, fvs = [], []
        for f in range(2):
            keys, desc = host[f]
            F = m.frame_from_device(dk + f * cap * 28, dd + f * cap * 32, len(keys), K, D0, g)
            wid, wval = m.frame_compute_bow(F, G, 4)
            (owid, owval), ofv = O.transform(desc, 4)
            assert np.array_equal(wid, owid) and wval.tobytes() == owval.tobytes()
            frames.append(F); fvs.append(ofv)
        (k0, d0), (k1, d1) = host
        qv = (rng.uniform(size=len(k0)) < 0.9).astype(np.uint8)
        tv = None if by_train else (rng.uniform(size=len(k1)) < 0.9).astype(np.uint8)
        got, n = m.SearchByBoWFrames(frames[0], qv, frames[1], tv, by_train)
        want, nw = oracle.search_by_bow(d0, k0["angle"], qv, fvs[0], d1, k1["angle"], tv, fvs[1], ratio, ori, by_train)
        assert n == nw and np.array_equal(got, want) and nw > 50
        # monocular initialisation search between the same two device frames (ORBmatcher.cc:407)
        q_xy = np.stack([k0["x"], k0["y"]], axis=1).astype(np.float32)
        gp = oracle.make_grid_params(0.0, 0.0, float(w), float(h))
        start, idx = oracle.grid_build(gp, k1)
        gi, gni = m.SearchForInitializationFrames(q_xy, 100.0, frames[0], frames[1])
        wi, wni = oracle.search_for_initialization(q_xy, 100.0, k0, d0, gp, k1, start, idx, d1, ratio, ori)
        assert gni == wni and np.array_equal(gi, wi) and wni > 30
        # SearchForTriangulation between the two device frames (ORBmatcher.cc:659): descriptors, keys and FeatureVectors
        # stay in HBM, only the "already has a MapPoint" flags and the fundamental matrix come from the host.
        # F12 of a pure sideways translation: epipolar lines are the rows, the epipole lies at infinity
        sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)
        F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float32)
        s1 = (rng.uniform(size=len(k0)) < 0.3).astype(np.uint8)
        s2 = (rng.uniform(size=len(k1)) < 0.3).astype(np.uint8)
        gt, gnt = m.SearchForTriangulationFrames(frames[0], s1, frames[1], s2, F12, 1.0e6, 240.0, sf, sf * sf)
        wt, wnt = oracle.search_for_triangulation(k0, d0, s1, fvs[0], k1, d1, s2, fvs[1], F12, 1.0e6, 240.0, sf, sf * sf, False, ori)
        assert gnt == wnt and np.array_equal(gt, wt) and wnt > 20
        # the windowed best search of Fuse / SearchBySim3 with the device frame as train side
        nq = 600
        pick = rng.integers(0, len(k1), nq)
        uvr = np.stack([k1["x"][pick] + rng.uniform(-2, 2, nq), k1["y"][pick] + rng.uniform(-2, 2, nq),
                        3.0 * sf[np.clip(k1["octave"][pick], 0, 7)]], axis=1).astype(np.float32)
        pred = np.clip(k1["octave"][pick] + rng.integers(0, 2, nq), 0, 7).astype(np.int8)
        qd = d1[pick].copy()
        flip = rng.integers(0, 32, nq)
        qd[np.arange(nq), flip] ^= np.uint8(5)
        inv = (1.0 / (sf * sf)).astype(np.float32)
        for chi2 in (False, True):
            bi, bd = m.window_best_frame(uvr, pred, qd, None, frames[1], inv, chi2)
            wi_, wd_ = oracle.window_best(uvr, pred, qd, None, gp, k1, start, idx, d1, inv, chi2)
            assert np.array_equal(bi, wi_) and np.array_equal(bd, wd_) and (wi_ >= 0).sum() > 300
        for F in frames:
            m.frame_destroy(F)


# ------------------------------------------------------------------ the branch-forcing frames of vocab_cases.cases()
# (test_vocab_cpu.py proves from the oracle's per-feature stream and a model of the bucket map that each reaches the path it
# is named for: 240 crowded buckets and none at 16 keys, buckets of half a frame, no key at all, the 64-wide sum's borders,
# the borders of the three placements at 4096 | 4097 and 8192 | 8193)
def _equal_transform(got, want, tag):
    (gi, gv), (gn, gs, gx) = got
    (oi, ov), (on, os_, ox) = want
    assert np.array_equal(gi, oi), tag
    assert gv.tobytes() == ov.tobytes(), tag
    assert np.array_equal(gn, on) and np.array_equal(gs, os_) and np.array_equal(gx, ox), tag


def _full_voc_handle(scoring, weighting):
    import vocab_cases as vc
    from orbslamm_amd import ORBVocabulary
    v = vc.full_vocab()
    return ORBVocabulary(vc.FULL_K, vc.FULL_L, scoring, weighting, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)


@pytest.mark.parametrize("scoring,weighting", [(0, 0), (1, 1), (5, 0), (0, 2), (5, 3)])
def test_transform_branch_cases(gpu, oracle, scoring, weighting):
    """ORBVocabulary::transform on every case, one handle, large and small sort sizes in turn"""
    import vocab_cases as vc
    G = _full_voc_handle(scoring, weighting)
    cases = vc.cases()
    order = vc.alternating_order(list(cases))
    assert order.index("all_stopped") < len(order) - 1      # a call follows the frame without a key
    for name in order:
        for levelsup in vc.LEVELSUP:
            got = G.transform(cases[name], levelsup)
            _equal_transform(got, vc.oracle_transform(oracle, name, scoring, weighting, levelsup), (name, levelsup))
            if name == "all_stopped":
                (gi, gv), (gn, gs, gx) = got
                assert len(gi) == 0 and len(gv) == 0 and len(gn) == 0 and len(gx) == 0 and gs.tolist() == [0]
    G.close()


class _Uploads:
    """device copies of host arrays (through an extractor handle's allocator), and keypoints on a lattice for frames
    that are made of given descriptors"""
    W, H = 640, 480
    K = [517.3, 516.5, 318.6, 255.3]
    D0 = [0, 0, 0, 0, 0]

    def __init__(self):
        from orbslamm_amd import ORBextractor
        self.gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=1, device=0)
        self.sf = np.array(self.gex.GetScaleFactors(), np.float32)
        self._dev = []

    def up(self, a):
        import ctypes as C
        from orbslamm_amd._lib import check, ptr
        a = np.ascontiguousarray(a)
        d = C.c_void_p()
        check(self.gex._L.orbx_device_alloc(self.gex._h, C.c_size_t(max(a.nbytes, 16)), C.byref(d)))
        if a.nbytes:
            check(self.gex._L.orbx_upload(self.gex._h, d, ptr(a), C.c_size_t(a.nbytes)))
        self._dev.append(d)
        return d.value

    def close(self):
        from orbslamm_amd._lib import check
        for d in self._dev:
            check(self.gex._L.orbx_device_free(self.gex._h, d))
        self._dev = []
        self.gex.close()

    @staticmethod
    def keys(n, seed):
        """n keypoints of octave 0 on a 5-pixel lattice inside the image, in random order, random angles"""
        from oracle.binding import KP_DTYPE
        rng = np.random.default_rng([seed, n])
        cols, rows = 118, 86
        assert n <= cols * rows
        cell = rng.permutation(cols * rows)[:n]
        k = np.zeros(n, KP_DTYPE)
        k["x"] = 25.0 + 5.0 * (cell % cols)
        k["y"] = 25.0 + 5.0 * (cell // cols)
        k["size"], k["response"], k["class_id"] = 31.0, 1.0, -1
        k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
        return k


def _probe(desc, seed):
    """one feature per distinct descriptor of `desc`, three bits flipped: a frame that a frame of repeated descriptors can
    be matched against with a result that depends on the order of its FeatureVector"""
    rng = np.random.default_rng(seed)
    u = np.unique(desc, axis=0)
    u = u[rng.permutation(len(u))]
    for b in rng.integers(0, 256, (3, len(u))):
        u[np.arange(len(u)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return u


def test_frame_compute_bow_branch_cases(gpu, oracle):
    """Frame::ComputeBoW on device-resident frames: the BowVector as bytes, the FeatureVector (which stays on the device)
    through SearchByBoW of the frame against itself and against a probe frame, held to the oracle's search"""
    import vocab_cases as vc
    from orbslamm_amd import ORBmatcher, make_grid
    G = _full_voc_handle(0, 0)
    up = _Uploads()
    m = ORBmatcher(0.8, True, device=0)
    g = make_grid(0.0, 0.0, float(up.W), float(up.H))
    cases = vc.cases()

    def frame(desc, seed):
        keys = up.keys(len(desc), seed)
        return keys, m.frame_from_device(up.up(keys), up.up(desc), len(desc), up.K, up.D0, g)

    seen = 0
    # levelsup 0: the FeatureVector's nodes are the words, so its sort meets the crowded buckets too -- and only there does the
    # order inside a bucket show (a word's addends are all the same weight)
    for levelsup in (0, 2, vc.FULL_L):
        for name in ("size_border_8193", "one_word", "size_border_4097", "all_stopped", "two_ends", "size_border_4096", "crowd_240",
                     "crowd_240_shuffled"):
            desc = cases[name]
            keys, F = frame(desc, 1)
            (owid, owval), ofv = vc.oracle_transform(oracle, name, 0, 0, levelsup)
            wid, wval = m.frame_compute_bow(F, G, levelsup)
            assert np.array_equal(wid, owid) and wval.tobytes() == owval.tobytes(), (name, levelsup)
            got, n = m.SearchByBoWFrames(F, None, F, None, True)
            want, nw = oracle.search_by_bow(desc, keys["angle"], None, ofv, desc, keys["angle"], None, ofv, 0.8, True, True)
            assert n == nw and np.array_equal(got, want), (name, levelsup, "self")
            pdesc = _probe(desc, 5)
            pkeys, PF = frame(pdesc, 2)
            pfv = vc.oracle_vocabulary(oracle, 0, 0).transform(pdesc, levelsup)[1]
            m.frame_compute_bow(PF, G, levelsup)
            for by_train in (True, False):
                got, n = m.SearchByBoWFrames(F, None, PF, None, by_train)
                want, nw = oracle.search_by_bow(desc, keys["angle"], None, ofv, pdesc, pkeys["angle"], None, pfv, 0.8, True, by_train)
                assert n == nw and np.array_equal(got, want), (name, levelsup, "probe", by_train)
                seen += nw
            m.frame_destroy(F); m.frame_destroy(PF)
    assert seen > 500          # the probe searches do match
    m.close(); G.close(); up.close()


@pytest.mark.parametrize("cap", [4096, 4097, 8193])
def test_frame_set_compute_bow_branch_cases(gpu, oracle, cap):
    """FrameSet.compute_bow: a set's aggregate kernel takes the sort size from the set's CAPACITY -- 4096 | 4097 | 8193 select
    k_voc_aggregate_set<true>, <false> and k_voc_aggregate_set_mem -- whatever a slot holds: the cases, an empty slot and a
    slot filled to capacity in one call, then the ring wrap (slot0 = slots - 1, n = 2)"""
    import vocab_cases as vc
    from orbslamm_amd import ORBmatcher, make_grid
    G = _full_voc_handle(0, 0)
    up = _Uploads()
    m = ORBmatcher(0.8, True, device=0)
    g = make_grid(0.0, 0.0, float(up.W), float(up.H))
    # None: a slot never built.  "probe": one feature per word of crowd_240 with three bits flipped -- searched from the two
    # crowd slots, whose 17 equal features per word compete for it, the match shows the order of their FeatureVector
    names = ["one_word", "two_ends", None, "crowd_240", "probe", "crowd_240_shuffled", "all_stopped", "size_border_%d" % cap]
    S = len(names)
    frames = dict(vc.cases(), probe=_probe(vc.cases()["crowd_240"], 5))
    O = vc.oracle_vocabulary(oracle, 0, 0)

    def transform(name, levelsup):
        return O.transform(frames[name], levelsup) if name == "probe" else vc.oracle_transform(oracle, name, 0, 0, levelsup)
    fs = m.frame_set(S, cap, up.K, up.D0, g, [0.0, float(up.W), 0.0, float(up.H)], up.sf)
    host = []
    for slot, name in enumerate(names):
        if name is None:
            host.append((up.keys(0, slot), np.zeros((0, 32), np.uint8), None))
            continue
        desc = frames[name]
        keys = up.keys(len(desc), slot)
        fs.build(slot, 1, up.up(keys), up.up(desc), up.up(np.array([len(desc)], np.int32)), len(desc))
        host.append((keys, desc, name))
    fs.sync()
    assert len(host[-1][1]) == cap
    empty = ((np.zeros(0, np.uint32), np.zeros(0)), (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32)))

    def check(tag, levelsup_of, kf, cur):
        """every slot's BowVector, and the FeatureVectors through the searches (kf[p], cur[p]); levelsup_of: per slot"""
        want = [empty if name is None else transform(name, levelsup_of[slot]) for slot, name in enumerate(names)]
        for slot in range(S):
            wid, wval = fs.bow_vector(slot)
            assert np.array_equal(wid, want[slot][0][0]) and wval.tobytes() == want[slot][0][1].tobytes(), (tag, slot, names[slot])
        fs.search_by_bow(kf, cur, nnratio=0.8, check_ori=True)
        match, nm = fs.bow_results()
        for p in range(len(kf)):
            (kq, dq, _), (kt, dt, _) = host[kf[p]], host[cur[p]]
            w, wn = oracle.search_by_bow(dq, kq["angle"], None, want[kf[p]][1], dt, kt["angle"], None, want[cur[p]][1], 0.8, True, True)
            assert nm[p] == wn and np.array_equal(match[p, :len(kt)], w), (tag, names[kf[p]], names[cur[p]])
        return nm

    every = np.arange(S)
    # (levelsup 0: the FeatureVector's nodes are the words, so its sort meets the 240 crowded buckets as well)
    for levelsup in (2, 0):
        fs.compute_bow(G, 0, S, levelsup)
        check("whole set, itself", [levelsup] * S, every, every)
        check("whole set, neighbour", [levelsup] * S, every, (every + 1) % S)
        nm = check("whole set, probe", [levelsup] * S, np.array([3, 5]), np.array([4, 4]))
        assert nm.min() > 50            # the crowd frames do match the probe
    fs.compute_bow(G, S - 1, 2, 2)              # the ring wrap: slots S - 1 and 0 go to levelsup 2, the others keep their nodes
    check("wrap", [2] + [0] * (S - 2) + [2], np.array([S - 1, 0, S - 1, 1]), np.array([S - 1, 0, 0, 1]))
    fs.close(); m.close(); G.close(); up.close()
