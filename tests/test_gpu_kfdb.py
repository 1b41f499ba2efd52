"""The device keyframe database (orbk_* / orbv_score) against the restatement (tests/kfdb_cases.py): candidate lists equal
in order, scored lists and the six query fields of every keyframe equal as bits."""
import struct

import numpy as np
import pytest

import dropin
import kfdb_cases as kc
from vocab_cases import make_vocab

pytestmark = pytest.mark.gpu
TUM_K = [517.3, 516.5, 318.6, 255.3]


def make_voc(rng, k=10, L=4, scoring=0):
    from orbslamm_amd import ORBVocabulary
    v = make_vocab(rng, k, L)
    return ORBVocabulary(k, L, scoring, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0), int(v["is_leaf"].sum()), v


def bits(x):
    return struct.pack("<d", float(x))


def test_orbv_score_bit_exact(gpu):
    rng = np.random.default_rng(3)
    G, nw, _ = make_voc(rng, 10, 3)
    sc = kc.make_scene(rng, 40, nw=60, n_words=nw)
    bows = sc["bows"]
    cases = [(bows[i], bows[j]) for i, j in rng.integers(0, 40, (60, 2))]
    empty = (np.zeros(0, np.uint32), np.zeros(0))
    cases += [(empty, empty), (bows[0], empty), (empty, bows[1]), (bows[2], bows[2])]
    a = (np.array([1, 5, 9], np.uint32), np.array([0.2, 0.3, 0.5]))
    b = (np.array([2, 6, 10], np.uint32), np.array([0.5, 0.25, 0.25]))
    cases += [(a, b), (b, a)]
    for v1, v2 in cases:
        want = kc.l1_score((v1[0].tolist(), v1[1].tolist()), (v2[0].tolist(), v2[1].tolist()))
        assert bits(G.score(v1, v2)) == bits(want)
    assert bits(G.score(empty, empty)) == bits(-0.0) and bits(G.score(a, b)) == bits(-0.0)


class Twin:
    """the device pool + databases and the restatement side by side"""

    def __init__(self, rng, n_kf, n_db, nw=60):
        from orbslamm_amd import KeyFrameDatabase, KeyFramePool
        self.rng = rng
        self.G, n_words, _ = make_voc(rng, 10, 4)
        self.sc = kc.make_scene(rng, n_kf, nw=nw, n_words=n_words)
        self.pool = KeyFramePool(self.G, n_kf)
        self.kfs = [kc.KeyFrame(i, *self.sc["bows"][i]) for i in range(n_kf)]
        for i, (ids, vals) in enumerate(self.sc["bows"]):
            self.pool.set_bow(i, ids, vals)
        self.covis = [list(c) for c in self.sc["covis"]]
        self.dbs = [KeyFrameDatabase(self.pool) for _ in range(n_db)]
        self.rdbs = [kc.Database() for _ in range(n_db)]
        self.queries = 0
        self.cands = 0

    def nb_dev(self, s):
        return self.covis[s]

    def nb_ref(self, k):
        return [self.kfs[j] for j in self.covis[k.slot]]

    def add(self, d, s):
        self.dbs[d].add(s)
        self.rdbs[d].add(self.kfs[s])

    def erase(self, d, s):
        self.dbs[d].erase(s)
        self.rdbs[d].erase(self.kfs[s])

    def clear(self, d):
        self.dbs[d].clear()
        self.rdbs[d].clear()

    def check_scored(self, d, rsc, tag):
        sl, sv = self.dbs[d].last_scored()
        assert sl.tolist() == [k.slot for _, k in rsc], tag
        assert sv.tobytes() == np.array([s for s, _ in rsc], np.float32).tobytes(), tag

    def reloc(self, d, qid, bow):
        got = self.dbs[d].DetectRelocalizationCandidates(qid, bow=bow, neighbours=self.nb_dev)
        want, rsc = self.rdbs[d].DetectRelocalizationCandidates(kc.Query(qid, *bow), self.nb_ref)
        assert got == [k.slot for k in want], ("reloc", qid)
        self.check_scored(d, rsc, ("reloc scored", qid))
        self.queries += 1
        self.cands += len(got)

    def loop(self, d, s, qid, conn, ms):
        self.kfs[s].mnId = qid
        got = self.dbs[d].DetectLoopCandidates(s, qid, ms, conn, neighbours=self.nb_dev)
        want, rsc = self.rdbs[d].DetectLoopCandidates(self.kfs[s], ms, {self.kfs[j] for j in conn}, self.nb_ref)
        assert got == [k.slot for k in want], ("loop", qid)
        self.check_scored(d, rsc, ("loop scored", qid))
        self.queries += 1
        self.cands += len(got)

    def check_state(self):
        st = self.pool.state()
        for f in ("mnRelocQuery", "mnRelocWords", "mnLoopQuery", "mnLoopWords"):
            assert st[f].tolist() == [getattr(k, f) for k in self.kfs], f
        for f in ("mRelocScore", "mLoopScore"):
            assert st[f].tobytes() == np.array([getattr(k, f) for k in self.kfs], np.float32).tobytes(), f

    def sizes(self):
        for d in range(len(self.dbs)):
            assert self.dbs[d].size() == self.rdbs[d].size() and self.dbs[d].empty() == self.rdbs[d].empty()


@pytest.mark.parametrize("n_kf,n_db,steps,seed", [(50, 2, 300, 1), (1000, 3, 200, 2), (10000, 4, 60, 3)])
def test_interleaved_sequences_equal_the_restatement(gpu, n_kf, n_db, steps, seed):
    rng = np.random.default_rng(seed)
    T = Twin(rng, n_kf, n_db)
    # most keyframes in some database first (each in one, a few twice)
    for s in range(n_kf):
        if rng.uniform() < 0.8:
            T.add(int(rng.integers(0, n_db)), s)
        if rng.uniform() < 0.03:
            T.add(int(rng.integers(0, n_db)), s)
    T.sizes()
    ids = list(range(1, 9))   # few query ids: same-id re-queries are common
    for step in range(steps):
        d = int(rng.integers(0, n_db))
        s = int(rng.integers(0, n_kf))
        op = rng.uniform()
        if op < 0.15:
            T.add(d, s)
        elif op < 0.22:
            T.erase(d, s)
        elif op < 0.23:
            T.clear(d)
        elif op < 0.28:
            T.covis[s] = [int(j) for j in rng.choice(n_kf, int(rng.integers(0, 11)), replace=False) if j != s][:10]
        elif op < 0.64:
            qid = int(rng.choice(ids)) if rng.uniform() < 0.7 else 100 + step
            bow = kc.query_bow(rng, T.sc) if rng.uniform() < 0.8 else T.sc["bows"][s]
            T.reloc(d, qid, bow)
        else:
            qid = int(rng.choice(ids)) if rng.uniform() < 0.7 else 100 + step
            T.loop(d, s, qid, T.covis[s][:int(rng.integers(0, 6))], np.float32(rng.uniform(0.0, 0.25)))
        if step % 25 == 0:
            T.check_state()
    T.sizes()
    T.check_state()
    assert T.cands > T.queries // 2, (T.cands, T.queries)   # (the scenes do produce candidates)


def test_stale_score_and_requery_on_the_device(gpu):
    """the hand-built cases of tests/test_kfdb_cpu.py, on the device"""
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool
    rng = np.random.default_rng(5)
    G, nw, _ = make_voc(rng, 10, 3)
    pool = KeyFramePool(G)
    pool.set_bow(0, [1, 2], [0.5, 0.5])
    pool.set_bow(1, [1, 3], [0.5, 0.5])
    db = KeyFrameDatabase(pool)
    db.add(0)
    db.add(1)
    nb = {0: [1], 1: [0]}
    assert db.DetectRelocalizationCandidates(4, bow=([1, 3], [0.5, 0.5]), neighbours=nb.get) == [1]
    assert db.DetectRelocalizationCandidates(5, bow=([1, 2, 9], [0.5, 0.25, 0.25]), neighbours=nb.get) == [1]   # stale 1.0 of slot 1
    sl, sv = db.last_scored()
    assert sl.tolist() == [0] and sv.tolist() == [0.75]
    pool.set_bow(2, [1], [1.0])
    db2 = KeyFrameDatabase(pool)
    db2.add(0)
    assert db2.DetectRelocalizationCandidates(7, bow=([1], [1.0])) == [0]
    db2.add(2)
    assert db2.DetectRelocalizationCandidates(7, bow=([1], [1.0])) == [2]   # same id: only what was added since
    st = pool.state()
    assert st["mnRelocWords"][0] == 2 and st["mnRelocQuery"][1] == 5 and st["mRelocScore"][1] == np.float32(1.0)
    db.clear()
    assert db.size() == 2 and not db.empty()


def test_loop_batch_equals_queries_one_at_a_time(gpu):
    """MultiMapper's scan: 200 keyframes of a newer map against a 2000-keyframe database, once as a batch and once as
    single queries on a twin pool, and both against the restatement (minScore from the covisible keyframes)"""
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool
    rng = np.random.default_rng(11)
    G, n_words, _ = make_voc(rng, 10, 4)
    n_old, n_new = 2000, 200
    sc = kc.make_scene(rng, n_old + n_new, nw=60, n_words=n_words, places=(n_old + n_new) // 10)
    pools = [KeyFramePool(G), KeyFramePool(G)]
    for p in pools:
        for i, (ids, vals) in enumerate(sc["bows"]):
            p.set_bow(i, ids, vals)
        for i in range(n_old + n_new):
            p.set_covisibility(i, sc["covis"][i])
    dbs = [KeyFrameDatabase(p) for p in pools]
    kfs = [kc.KeyFrame(i, *sc["bows"][i]) for i in range(n_old + n_new)]
    ref = kc.Database()
    for i in range(n_old):
        for d in dbs:
            d.add(i)
        ref.add(kfs[i])
    slots = list(range(n_old + n_new - 1, n_old - 1, -1))       # (the reference walks the map's keyframes from the back)
    qids = [int(rng.integers(1, 30)) for _ in slots]            # repeated ids: the queries depend on each other
    conn = [sc["covis"][s][:4] for s in slots]
    cov = [sc["covis"][s] for s in slots]
    batch = dbs[0].detect_loop_batch(slots, qids, conn, cov)
    total = 0
    for q, s in enumerate(slots):
        ms = np.float32(pools[1].score(s, cov[q]).min(initial=np.float32(1.0)))
        assert ms == kc.min_score(kfs[s], [kfs[j] for j in cov[q]])
        single = dbs[1].DetectLoopCandidates(s, qids[q], ms, conn[q])   # neighbours: the pool's table
        kfs[s].mnId = qids[q]
        want, _ = ref.DetectLoopCandidates(kfs[s], ms, {kfs[j] for j in conn[q]}, lambda k: [kfs[j] for j in sc["covis"][k.slot]])
        assert batch[q] == single == [k.slot for k in want], q
        total += len(single)
    assert total > 0
    a, b = pools[0].state(), pools[1].state()
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), f


def test_relocalisation_chain_from_a_frame_set(gpu, oracle):
    """Frame::ComputeBoW on a frame set -> DetectRelocalizationCandidates with F->mBowVec copied device to device ->
    SearchByBoW(candidate, F) on the set, against the restatement on the downloaded BowVectors and the oracle's SearchByBoW"""
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool, ORBextractor, ORBmatcher, make_grid, synth
    rng = np.random.default_rng(23)
    k, L, levelsup = 10, 4, 2
    G, nw, voc = make_voc(rng, k, L)
    O = oracle.Vocabulary(k, L, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    w, h, nf, B = 640, 480, 1000, 6
    fr = synth.make_frames(w, h, B, stream=4)
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B, device=0)
    gex.extract_batch_device(*gex.upload_frames(fr))
    host = [gex.download(f) for f in range(B)]
    m = ORBmatcher(0.75, True, device=0)
    g = make_grid(0.0, 0.0, float(w), float(h))
    fs = m.frame_set(B, gex.max_keypoints, TUM_K, [0, 0, 0, 0, 0], g, [0.0, float(w), 0.0, float(h)], np.array(gex.GetScaleFactors(), np.float32))
    fs.build_from_extractor(0, gex)
    fs.compute_bow(G, 0, B, levelsup)
    pool = KeyFramePool(G)
    db = KeyFrameDatabase(pool)
    ref = kc.Database()
    kfs = []
    for s in range(B - 1):                     # slots 0..4 are keyframes, slot 5 is the lost frame
        pool.set_bow_from_frameset(s, fs, s)
        kfs.append(kc.KeyFrame(s, *fs.bow_vector(s)))
        db.add(s)
        ref.add(kfs[s])
    covis = {s: [j for j in range(B - 1) if j != s][:3] for s in range(B - 1)}
    qb = fs.bow_vector(B - 1)
    for qid in (1, 2, 2):
        got = db.DetectRelocalizationCandidates(qid, frameset=fs, fs_slot=B - 1, neighbours=covis.get)
        want, rsc = ref.DetectRelocalizationCandidates(kc.Query(qid, *qb), lambda kf: [kfs[j] for j in covis[kf.slot]])
        assert got == [kf.slot for kf in want]
        sl, sv = db.last_scored()
        assert sl.tolist() == [kf.slot for _, kf in rsc] and sv.tobytes() == np.array([s for s, _ in rsc], np.float32).tobytes()
    st = pool.state()
    assert st["mRelocScore"].tobytes() == np.array([kf.mRelocScore for kf in kfs], np.float32).tobytes()
    # SearchByBoW(candidate KeyFrame, F) for the first query's candidates
    cands = db.DetectRelocalizationCandidates(9, frameset=fs, fs_slot=B - 1, neighbours=covis.get)
    assert cands
    fs.search_by_bow(cands, [B - 1] * len(cands), nnratio=0.75, check_ori=True)
    match, nm = fs.bow_results()
    kt, dt = host[B - 1]
    _, fv_t = O.transform(dt, levelsup)
    for p, c in enumerate(cands):
        kq, dq = host[c]
        _, fv_q = O.transform(dq, levelsup)
        want, wn = oracle.search_by_bow(dq, kq["angle"], None, fv_q, dt, kt["angle"], None, fv_t, 0.75, True, True)
        assert nm[p] == wn and np.array_equal(match[p, :len(kt)], want)
    fs.close()
    m.close()


def test_refusals(gpu):
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool, OrbError
    from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED
    rng = np.random.default_rng(2)
    G2, _, _ = make_voc(rng, 10, 3, scoring=1)            # L2_NORM
    with pytest.raises(OrbError) as e:
        KeyFramePool(G2)
    assert e.value.code == ORBX_E_UNSUPPORTED
    with pytest.raises(OrbError) as e:
        G2.score(([1], [1.0]), ([1], [1.0]))
    assert e.value.code == ORBX_E_UNSUPPORTED
    G, nw, _ = make_voc(rng, 10, 3)
    pool = KeyFramePool(G)
    pool.set_bow(0, [1, 2], [0.5, 0.5])
    db = KeyFrameDatabase(pool)
    db.add(0)
    for bad in (lambda: db.add(5), lambda: db.add(-1), lambda: db.erase(1), lambda: pool.set_bow(-1, [], []),
                lambda: pool.set_bow(1, [nw], [1.0]), lambda: pool.set_bow(1, [3, 2], [0.5, 0.5]),
                lambda: pool.score(0, [7]), lambda: pool.set_covisibility(0, [3]), lambda: pool.set_covisibility(0, [0] * 11),
                lambda: db.DetectLoopCandidates(4, 1, 0.0), lambda: db.DetectLoopCandidates(0, 1, 0.0, connected=[9]),
                lambda: db.DetectRelocalizationCandidates(1, bow=([nw + 5], [1.0])),
                lambda: db.DetectRelocalizationCandidates(1, bow=([1, 2], [0.5, 0.5]), neighbours=lambda s: [42]),
                lambda: db.detect_loop_batch([3], [1], [[]], [[]])):
        with pytest.raises(OrbError) as e:
            bad()
        assert e.value.code == ORBX_E_INVALID
    with pytest.raises(OrbError) as e:                       # the BowVector of a keyframe in a database is fixed
        pool.set_bow(0, [1], [1.0])
    assert e.value.code == ORBX_E_INVALID
    with pytest.raises(ValueError):                           # more than GetBestCovisibilityKeyFrames(10) gives
        db.DetectRelocalizationCandidates(2, bow=([1, 2], [0.5, 0.5]), neighbours=lambda s: [0] * 11)   # (a new id: slot 0 is scored)


def test_mixed_devices_are_refused(gpu):
    from orbslamm_amd import KeyFramePool, ORBmatcher, ORBVocabulary, OrbError, make_grid
    from orbslamm_amd._lib import ORBX_E_INVALID
    if gpu < 2:
        pytest.skip("one device: a frame set on another device than the pool cannot be made")
    rng = np.random.default_rng(8)
    v = make_vocab(rng, 10, 3)
    G0 = ORBVocabulary(10, 3, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)
    G1 = ORBVocabulary(10, 3, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=1)
    m1 = ORBmatcher(0.75, True, device=1)
    fs1 = m1.frame_set(2, 1000, TUM_K, [0, 0, 0, 0, 0], make_grid(0.0, 0.0, 640.0, 480.0), [0.0, 640.0, 0.0, 480.0], np.ones(8, np.float32))
    fs1.compute_bow(G1, 0, 2, 4)
    pool = KeyFramePool(G0)
    with pytest.raises(OrbError) as e:
        pool.set_bow_from_frameset(0, fs1, 0)
    assert e.value.code == ORBX_E_INVALID
    fs1.close()


def test_keyframe_database_dropin_runs(gpu):
    """include/KeyFrameDatabase_hip.hpp on mock keyframes (tests/cpp/kfdb_dropin_gpu.cpp) against tools/kfdb_ref.hpp"""
    dropin.run(dropin.build("kfdb_dropin_gpu"), timeout=600, marker="kfdb_dropin_gpu ok")


def test_loop_batch_returns_more_candidates_than_the_staging_block(gpu):
    """a batch whose candidates outgrow the pinned block its parameters went up in (64 KiB = 16 384 slots): every keyframe
    holds the same words, so every query returns the whole 2 000-keyframe database -- 24 000 candidates in 12 queries"""
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool
    rng = np.random.default_rng(31)
    G, nw, _ = make_voc(rng, 10, 3)
    n_db, n_q = 2000, 12
    words = np.array([3, 17, 40, 41, 99], np.uint32)
    bows = []
    for _ in range(n_db + n_q):
        v = rng.uniform(0.9, 1.1, words.shape[0])
        bows.append((words, v / v.sum()))
    far = (np.array([5, 6], np.uint32), np.array([0.5, 0.5]))   # shares no word: minScore = -0.0
    bows.append(far)
    pool = KeyFramePool(G)                                       # (a fresh pool: its staging block is at its smallest)
    for i, (ids, vals) in enumerate(bows):
        pool.set_bow(i, ids, vals)
    db = KeyFrameDatabase(pool)
    kfs = [kc.KeyFrame(i, *bows[i]) for i in range(len(bows))]
    ref = kc.Database()
    for i in range(n_db):
        db.add(i)
        ref.add(kfs[i])
    slots = list(range(n_db, n_db + n_q))
    qids = [50 + q for q in range(n_q)]
    got = db.detect_loop_batch(slots, qids, [[]] * n_q, [[n_db + n_q]] * n_q)
    total = 0
    for q, s in enumerate(slots):
        ms = kc.min_score(kfs[s], [kfs[n_db + n_q]])
        kfs[s].mnId = qids[q]
        want, _ = ref.DetectLoopCandidates(kfs[s], ms, set(), lambda k: [])
        assert got[q] == [k.slot for k in want], q
        total += len(want)
    assert total > 16384, total


def test_frame_set_slots_of_another_vocabulary_are_refused(gpu):
    """a frame set slot's word ids index the pool's word table: a slot transformed with another vocabulary (here a larger
    one) is refused by both frame set entries; the pool's own vocabulary is accepted"""
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool, ORBextractor, ORBmatcher, OrbError, make_grid, synth
    from orbslamm_amd._lib import ORBX_E_INVALID
    rng = np.random.default_rng(41)
    G_small, nw_small, _ = make_voc(rng, 10, 3)
    G_big, nw_big, _ = make_voc(rng, 10, 4)
    assert nw_big > nw_small
    w, h, nf, B = 640, 480, 1000, 2
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B, device=0)
    gex.extract_batch_device(*gex.upload_frames(synth.make_frames(w, h, B, stream=6)))
    m = ORBmatcher(0.75, True, device=0)
    g = make_grid(0.0, 0.0, float(w), float(h))
    fs = m.frame_set(B, gex.max_keypoints, TUM_K, [0, 0, 0, 0, 0], g, [0.0, float(w), 0.0, float(h)], np.array(gex.GetScaleFactors(), np.float32))
    fs.build_from_extractor(0, gex)
    fs.compute_bow(G_big, 0, B, 2)
    assert int(fs.bow_vector(0)[0].max()) >= nw_small              # (ids the small vocabulary's table does not hold)
    pool = KeyFramePool(G_small)
    pool.set_bow(0, [1, 2], [0.5, 0.5])
    db = KeyFrameDatabase(pool)
    db.add(0)
    for bad in (lambda: pool.set_bow_from_frameset(1, fs, 0), lambda: db.DetectRelocalizationCandidates(3, frameset=fs, fs_slot=1)):
        with pytest.raises(OrbError) as e:
            bad()
        assert e.value.code == ORBX_E_INVALID
    fs.compute_bow(G_small, 0, B, 2)                               # the same slots transformed with the pool's vocabulary
    pool.set_bow_from_frameset(1, fs, 0)
    db.DetectRelocalizationCandidates(3, frameset=fs, fs_slot=1)
    fs.close()
    m.close()
