"""The keyframe database's contract on the CPU: the restatement (tests/kfdb_cases.py) against hand-written expectations,
one case per quirk of src/KeyFrameDatabase.cc; the device algorithm's model (no inverted file: per keyframe its copies,
shared-word count and first-encounter key) against the restatement on random sequences; the C++ drop-in compiles."""
import os
import subprocess
from collections import deque

import numpy as np
import pytest

import kfdb_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def kf(slot, words):
    """words: {id: value}"""
    ids = sorted(words)
    return kc.KeyFrame(slot, ids, [words[i] for i in ids])


def q(mnId, words):
    ids = sorted(words)
    return kc.Query(mnId, ids, [words[i] for i in ids])


def no_neighbours(_kf):
    return []


def test_stale_reloc_score_is_read():
    """a neighbour pushed by this query but not scored (words <= minCommonWords) adds the mRelocScore of an earlier query"""
    A, B = kf(0, {1: 0.5, 2: 0.5}), kf(1, {1: 0.5, 3: 0.5})
    db = kc.Database()
    db.add(A)
    db.add(B)
    nb = {0: [B], 1: [A]}
    cands, scored = db.DetectRelocalizationCandidates(q(4, {1: 0.5, 3: 0.5}), lambda k: nb[k.slot])
    assert [k.slot for k in cands] == [1] and [(float(s), k.slot) for s, k in scored] == [(1.0, 1)]
    assert B.mRelocScore == F32(1.0) and A.mRelocScore == F32(0.0)
    cands, scored = db.DetectRelocalizationCandidates(q(5, {1: 0.5, 2: 0.25, 9: 0.25}), lambda k: nb[k.slot])
    assert [(float(s), k.slot) for s, k in scored] == [(0.75, 0)]       # B shares one word of two: not scored ...
    assert B.mnRelocQuery == 5 and B.mnRelocWords == 1 and B.mRelocScore == F32(1.0)
    assert [k.slot for k in cands] == [1]                               # ... yet its stale 1.0 makes it pBestKF


def test_same_id_requery_returns_only_keyframes_added_since():
    A, C = kf(0, {1: 1.0}), kf(2, {1: 1.0})
    db = kc.Database()
    db.add(A)
    cands, _ = db.DetectRelocalizationCandidates(q(3, {1: 1.0}), no_neighbours)
    assert [k.slot for k in cands] == [0]
    db.add(C)
    cands, scored = db.DetectRelocalizationCandidates(q(3, {1: 1.0}), no_neighbours)
    assert [k.slot for k in cands] == [2] and [k.slot for _, k in scored] == [2]
    assert A.mnRelocWords == 2 and C.mnRelocWords == 1                 # the old one's count keeps growing


def test_connected_keyframes_end_with_one_loop_word():
    Q = kf(0, {1: 1 / 3, 2: 1 / 3, 3: 1 / 3})
    Q.mnId = 10   # (an id of 0 would equal every keyframe's initial mnLoopQuery)
    A, B = kf(1, {1: 1 / 3, 2: 1 / 3, 3: 1 / 3}), kf(2, {1: 0.5, 2: 0.5})
    db = kc.Database()
    db.add(A)
    db.add(B)
    cands, scored = db.DetectLoopCandidates(Q, 0.0, {A}, no_neighbours)
    assert A.mnLoopWords == 1 and A.mnLoopQuery == 0                   # three hits, reset before each; query left alone
    assert B.mnLoopWords == 2 and B.mnLoopQuery == Q.mnId
    assert [k.slot for k in cands] == [2] and scored[0][0] == F32(2 / 3)


def test_double_add_counts_twice_and_erase_removes_one_copy():
    A, B = kf(0, {1: 0.5, 2: 0.5}), kf(1, {1: 1 / 3, 2: 1 / 3, 3: 1 / 3})
    F = {1: 1 / 3, 2: 1 / 3, 3: 1 / 3}
    db = kc.Database()
    db.add(A)
    db.add(A)
    db.add(B)
    assert db.size() == 3
    cands, scored = db.DetectRelocalizationCandidates(q(1, F), no_neighbours)
    assert A.mnRelocWords == 4 and B.mnRelocWords == 3                 # max 4, minCommonWords int(3.2) = 3
    assert [k.slot for _, k in scored] == [0] and [k.slot for k in cands] == [0]
    db.erase(A)
    assert db.size() == 2
    cands, scored = db.DetectRelocalizationCandidates(q(2, F), no_neighbours)
    assert A.mnRelocWords == 2 and B.mnRelocWords == 3                 # one copy of A left; max 3, minCommonWords 2
    assert [k.slot for _, k in scored] == [1] and [k.slot for k in cands] == [1]
    for _ in range(4):
        db.erase(A)
    assert db.size() == 0 and db.empty()


def test_clear_keeps_size():
    A, B = kf(0, {1: 1.0}), kf(1, {2: 1.0})
    db = kc.Database()
    db.add(A)
    db.add(B)
    db.clear()
    assert db.size() == 2 and not db.empty()
    cands, scored = db.DetectRelocalizationCandidates(q(1, {1: 0.5, 2: 0.5}), no_neighbours)
    assert cands == [] and scored == [] and A.mnRelocQuery == 0


def test_min_common_words_truncation_boundary():
    """minCommonWords = (int)(maxCommonWords*0.8f) and the test is strictly greater: max 5 -> 4 (4 words out), max 2 -> 1"""
    words = {i: 0.2 for i in range(1, 6)}
    A, B = kf(0, words), kf(1, {i: 0.25 for i in range(1, 5)})
    db = kc.Database()
    db.add(A)
    db.add(B)
    _, scored = db.DetectRelocalizationCandidates(q(1, words), no_neighbours)
    assert [k.slot for _, k in scored] == [0]
    C, D = kf(2, {1: 0.5, 2: 0.5}), kf(3, {1: 0.5, 7: 0.5})
    db2 = kc.Database()
    db2.add(D)
    db2.add(C)
    _, scored = db2.DetectRelocalizationCandidates(q(2, {1: 0.5, 2: 0.5}), no_neighbours)
    assert [k.slot for _, k in scored] == [2]
    assert int(F32(5) * F32(0.8)) == 4 and int(F32(2) * F32(0.8)) == 1 and int(F32(4) * F32(0.8)) == 3


def test_best_keyframe_is_returned_once():
    A, B, C = kf(0, {1: 0.5, 3: 0.5}), kf(1, {1: 0.5, 2: 0.5}), kf(2, {2: 0.5, 4: 0.5})
    db = kc.Database()
    for k in (A, B, C):
        db.add(k)
    nb = {0: [B], 1: [], 2: [B]}
    cands, scored = db.DetectRelocalizationCandidates(q(9, {1: 0.4, 2: 0.4, 3: 0.1, 4: 0.1}), lambda k: nb[k.slot])
    assert [k.slot for _, k in scored] == [0, 1, 2]                     # first-encounter order: word 1 [A, B], word 2 [B, C]
    assert [k.slot for k in cands] == [1]                               # A and C both point at B: once


def test_l1_score_order_and_sign():
    assert str(kc.l1_score(([], []), ([], []))) == "-0.0"
    assert str(kc.l1_score(([1], [0.5]), ([2], [0.5]))) == "-0.0"
    assert kc.l1_score(([1, 2], [0.5, 0.5]), ([1, 2], [0.5, 0.5])) == 1.0


# ---------------------------------------------------------------- the device algorithm, modelled on the host
class SlotModel:
    """what orbk_kernels.hip computes: per database member (slot) its live copies (insertion sequences, earliest first);
    a query meets a member copies * shared-words times, first at key (smallest shared query word, earliest live copy)"""

    def __init__(self, bows):
        self.bows = bows
        n = len(bows)
        self.relocQ, self.relocW, self.relocS = [0] * n, [0] * n, [F32(0)] * n
        self.loopQ, self.loopW, self.loopS = [0] * n, [0] * n, [F32(0)] * n

    def new_db(self):
        return dict(copies={}, seq=0, n=0)

    @staticmethod
    def add(db, s):
        db["n"] += 1
        db["copies"].setdefault(s, deque()).append(db["seq"])
        db["seq"] += 1

    @staticmethod
    def erase(db, s):
        if db["n"] > 0:
            db["n"] -= 1
        if db["copies"].get(s):
            db["copies"][s].popleft()

    @staticmethod
    def clear(db):
        db["copies"] = {}

    def query(self, db, qid, qbow, loop, conn=(), minScore=0.0, neighbours=None):
        qw = dict(zip(qbow[0], range(len(qbow[0]))))
        Q, W, S = (self.loopQ, self.loopW, self.loopS) if loop else (self.relocQ, self.relocW, self.relocS)
        pushed = []
        for s, cp in db["copies"].items():
            if not cp:
                continue
            hits = [w for w in self.bows[s][0] if w in qw]
            if not hits:
                continue
            c = len(hits) * len(cp)
            if Q[s] != qid:
                if loop and s in conn:
                    W[s] = 1
                else:
                    W[s] = c
                    Q[s] = qid
                    pushed.append(((min(hits), cp[0]), s))
            else:
                W[s] += c
        if not pushed:
            return [], []
        mx = max(W[s] for _, s in pushed)
        mc = int(F32(mx) * F32(0.8))
        sel = []
        for key, s in pushed:
            if W[s] > mc:
                si = F32(kc.l1_score(qbow, self.bows[s]))
                S[s] = si
                if not loop or si >= F32(minScore):
                    sel.append((key, s, si))
        sel.sort()
        accs = []
        for _, s, si in sel:
            acc, best, pb = si, si, s
            for k2 in neighbours(s):
                if Q[k2] == qid and (not loop or W[k2] > mc):
                    acc = F32(acc + S[k2])
                    if S[k2] > best:
                        pb, best = k2, S[k2]
            accs.append((acc, pb))
        bestAcc = max([F32(minScore) if loop else F32(0)] + [a for a, _ in accs])
        thr = F32(0.75) * bestAcc
        out = []
        for a, pb in accs:
            if a > thr and pb not in out:
                out.append(pb)
        return out, [(si, s) for _, s, si in sel]


@pytest.mark.parametrize("seed", range(6))
def test_device_model_equals_restatement_on_random_sequences(seed):
    rng = np.random.default_rng(seed)
    n = 60
    sc = kc.make_scene(rng, n, nw=25, n_words=400)
    kfs = [kc.KeyFrame(i, *sc["bows"][i]) for i in range(n)]
    model = SlotModel([(b[0].tolist(), b[1].tolist()) for b in sc["bows"]])
    dbs = [kc.Database() for _ in range(3)]
    mdbs = [model.new_db() for _ in range(3)]
    covis = sc["covis"]
    for step in range(150):
        d = int(rng.integers(0, 3))
        op = rng.uniform()
        s = int(rng.integers(0, n))
        if op < 0.45:
            dbs[d].add(kfs[s])
            model.add(mdbs[d], s)
        elif op < 0.55:
            dbs[d].erase(kfs[s])
            model.erase(mdbs[d], s)
        elif op < 0.57:
            dbs[d].clear()
            model.clear(mdbs[d])
        else:
            qid = int(rng.integers(1, 12))   # few ids: same-id re-queries are common
            if rng.uniform() < 0.5:
                qb = kc.query_bow(rng, sc) if rng.uniform() < 0.7 else sc["bows"][int(rng.integers(0, n))]
                ref, rsc = dbs[d].DetectRelocalizationCandidates(kc.Query(qid, *qb), lambda k: [kfs[j] for j in covis[k.slot]])
                got, gsc = model.query(mdbs[d], qid, (qb[0].tolist(), qb[1].tolist()), False, neighbours=lambda j: covis[j])
            else:
                conn = set(covis[s][:4])
                ms = F32(rng.uniform(0.0, 0.3))
                kfs[s].mnId = qid
                ref, rsc = dbs[d].DetectLoopCandidates(kfs[s], ms, {kfs[j] for j in conn}, lambda k: [kfs[j] for j in covis[k.slot]])
                got, gsc = model.query(mdbs[d], qid, model.bows[s], True, conn, ms, lambda j: covis[j])
            assert [k.slot for k in ref] == got, step
            assert [(np.float32(a).tobytes(), k.slot) for a, k in rsc] == [(np.float32(a).tobytes(), s2) for a, s2 in gsc], step
        assert dbs[d].size() == mdbs[d]["n"]
    for k in kfs:
        i = k.slot
        assert (k.mnRelocQuery, k.mnRelocWords, k.mRelocScore) == (model.relocQ[i], model.relocW[i], model.relocS[i])
        assert (k.mnLoopQuery, k.mnLoopWords, k.mLoopScore) == (model.loopQ[i], model.loopW[i], model.loopS[i])


def test_keyframe_database_dropin_template_instantiates(tmp_path):
    """KeyFrameDatabaseT<KeyFrame, Frame> with the reference's member signatures compiles against mock types that carry
    the reference's member names (no GPU needed to build; the run is a -m gpu test)"""
    from orbslamm_amd import _lib
    _lib.build()
    exe = str(tmp_path / "kfdb_dropin")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "kfdb_dropin_gpu.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "orbslamm_amd"), "-lorbslamm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "orbslamm_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    syms = subprocess.check_output(["nm", "-C", exe]).decode()
    for member in ("add", "erase", "clear", "DetectLoopCandidates", "DetectRelocalizationCandidates", "size", "empty"):
        assert "KeyFrameDatabaseT<kfmock::KeyFrame, kfmock::Frame>::" + member + "(" in syms, member
    assert "ORBVocabularyScoreT<std::map<unsigned int, double" in syms and "U orbv_score" in syms
