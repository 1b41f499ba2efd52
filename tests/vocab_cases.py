"""Synthetic DBoW2 vocabularies (the real ORBvoc.txt is absent from the reference checkout,
SURVEY.md F9): a k-ary tree of random ORB-like descriptors in loadFromTextFile order."""
import numpy as np


def make_vocab(rng, k, L, stop_fraction=0.05, ragged=True):
    """returns dict(parent, is_leaf, desc, weight) with nodes in breadth-first file order"""
    parent, is_leaf, desc, weight = [], [], [], []
    frontier = [(0, 0, rng.integers(0, 256, 32, dtype=np.uint8))]  # (node id, level, descriptor)
    next_id = 1
    while frontier:
        nxt = []
        for pid, lvl, pd in frontier:
            nchild = k if not ragged or lvl == 0 else int(rng.integers(2, k + 1))
            for _ in range(nchild):
                d = pd.copy()
                for b in rng.integers(0, 256, max(4, 60 >> lvl)):  # children = perturbed parents
                    d[b // 8] ^= np.uint8(1 << (b % 8))
                leaf = lvl + 1 == L or (ragged and lvl + 1 >= 2 and rng.uniform() < 0.1)
                parent.append(pid)
                is_leaf.append(leaf)
                desc.append(d)
                w = 0.0 if (leaf and rng.uniform() < stop_fraction) else float(rng.uniform(0.1, 9.0))
                weight.append(w)
                if not leaf:
                    nxt.append((next_id, lvl + 1, d))
                next_id += 1
        frontier = nxt
    return dict(parent=np.array(parent, np.int32), is_leaf=np.array(is_leaf, np.uint8), desc=np.stack(desc),
                weight=np.array(weight, np.float64), k=k, L=L)


def write_text(path, voc, scoring, weighting):
    """saveToTextFile format (TemplatedVocabulary.h:1430-1460): 'k L scoring weighting' then
    'parent is_leaf b0..b31 weight' per node"""
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (voc["k"], voc["L"], scoring, weighting))
        for i in range(len(voc["parent"])):
            f.write("%d %d %s %r\n" % (voc["parent"][i], int(voc["is_leaf"][i]), " ".join(str(int(b)) for b in voc["desc"][i]),
                                      float(voc["weight"][i])))


def naive_transform(voc, scoring, weighting, desc, levelsup, memo=None):
    """independent Python re-derivation of DBoW2's transform (ordered dicts = std::map).  memo: a dict the caller keeps
    for ONE vocabulary; the path of a descriptor seen before is taken from it (the frames of cases() repeat a few
    hundred descriptors thousands of times)"""
    n = len(voc["parent"])
    children = {i: [] for i in range(n + 1)}
    word = {}
    for i in range(n):
        children[int(voc["parent"][i])].append(i + 1)
        if voc["is_leaf"][i]:
            word[i + 1] = len(word)
    lut = np.array([bin(i).count("1") for i in range(256)], np.uint8)
    bow, fv = {}, {}
    nid_level = voc["L"] - levelsup
    for fi, f in enumerate(desc):
        key = f.tobytes() if memo is not None else None
        path = memo.get(key) if memo is not None else None
        if path is None:
            path, node = [], 0
            while True:
                ch = children[node]
                ds = [int(lut[np.bitwise_xor(f, voc["desc"][c - 1])].sum()) for c in ch]
                node = ch[int(np.argmin(ds))]  # argmin = first minimum
                path.append(node)
                if not children[node]:
                    break
            if memo is not None:
                memo[key] = path
        node = path[-1]
        nid = path[nid_level - 1] if 1 <= nid_level <= len(path) else 0
        w = float(voc["weight"][node - 1])
        if w > 0:
            wid = word[node]
            if weighting in (0, 1):
                bow[wid] = bow.get(wid, 0.0) + w if wid in bow else w
            else:
                bow.setdefault(wid, w)
            fv.setdefault(nid, []).append(fi)
    ids = sorted(bow)
    vals = [bow[i] for i in ids]
    must = scoring != 5
    if weighting in (0, 1) and vals and not must:
        vals = [v / float(len(vals)) for v in vals]
    if must:
        norm = 0.0
        if scoring != 1:
            for v in vals:
                norm += abs(v)
        else:
            for v in vals:
                norm += v * v
            norm = float(np.sqrt(np.float64(norm)))
        if norm > 0:
            vals = [v / norm for v in vals]
    nodes = sorted(fv)
    start = [0]
    idx = []
    for nd in nodes:
        idx.extend(fv[nd])
        start.append(len(idx))
    return (np.array(ids, np.uint32), np.array(vals, np.float64)), (np.array(nodes, np.uint32), np.array(start, np.int32), np.array(idx, np.int32))


# ------------------------------------------------------------------ frames with a prescribed word histogram
# On a full tree every leaf's own descriptor descends to that leaf (test_vocab_cpu.py confirms it with the oracle's
# transform_one), so a frame with a prescribed histogram is a list of leaf descriptors, repeated as often as wanted.
FULL_K, FULL_L = 10, 4
PAIRS = ((0, 0), (1, 1), (5, 0), (0, 2), (5, 3))      # (scoring, weighting): L1, L2, no normalisation with the division by the
#                                                      word count, addIfNotExist with and without normalisation
LEVELSUP = (0, 2, FULL_L, FULL_L + 2)
_full = {}


def full_vocab():
    """the full 10-ary tree of depth 4: 11 110 nodes, 10 000 words (ids 0 .. 9999 = the last 10 000 nodes), ~5 % stop words"""
    if "voc" not in _full:
        voc = make_vocab(np.random.default_rng(1004), FULL_K, FULL_L, ragged=False)
        leaves = np.flatnonzero(voc["is_leaf"])
        assert len(leaves) == FULL_K ** FULL_L
        _full.update(voc=voc, leaves=leaves, stop=np.flatnonzero(voc["weight"][leaves] == 0), live=np.flatnonzero(voc["weight"][leaves] > 0))
    return _full["voc"]


def stop_words():
    full_vocab()
    return _full["stop"]


def live_words():
    full_vocab()
    return _full["live"]


def frame_for_histogram(voc, words, counts, order=None):
    """descriptors of a frame in which word words[i] has counts[i] features: grouped by word in the order given, or
    permuted by `order` (feature j of the frame is feature order[j] of the grouped one)"""
    leaves = np.flatnonzero(voc["is_leaf"])
    desc = np.repeat(voc["desc"][leaves[np.asarray(words, np.int64)]], np.asarray(counts, np.int64), axis=0)
    return desc if order is None else desc[np.asarray(order)]


def sort_P(n):
    P = 2
    while P < n:
        P <<= 1
    return P


def bucket_model(ids, P):
    """the bucket map of bucket_sort_lds (orbv_kernels.hip) on keys (ids[j], feature = position j in the frame); ids < 0
    are left out (stopped features).  Returns the key count of every bucket.  Only ever used to prove that a case reaches
    the path it is named for, never to compute an expected value."""
    ids = np.asarray(ids, np.int64)
    feat = np.flatnonzero(ids >= 0)
    cnt = np.zeros(P, np.int64)
    if len(feat) == 0:
        return cnt
    v = ids[feat]
    lo, hi = int(v.min()), int(v.max())
    scale = float(P) / (float(hi - lo + 1) * 8192.0)
    b = np.minimum((((v - lo) * 8192 + feat).astype(np.float64) * scale).astype(np.int64), P - 1)
    np.add.at(cnt, b, 1)
    return cnt


K_CROWD = 16            # bucket_sort_lds: a bucket of more keys is rank-sorted by the whole workgroup
CROWD_START = None      # set by _crowd_words


def _crowd_words():
    """240 live words about 41 ids apart: word i is the first live word at or after start + 41 i, the start chosen as the
    first for which the model gives 240 crowded buckets at 17 grouped features per word and none at 16"""
    global CROWD_START
    live = live_words()
    is_live = np.zeros(FULL_K ** FULL_L, bool)
    is_live[live] = True
    for start in range(0, 200):
        words = np.array([live[np.searchsorted(live, start + 41 * i)] for i in range(240)])
        if len(set(words.tolist())) != 240:
            continue
        c17 = bucket_model(np.repeat(words, 17), 4096)
        c16 = bucket_model(np.repeat(words, 16), 4096)
        if (c17 > K_CROWD).sum() == 240 and (c16 > K_CROWD).sum() == 0:
            CROWD_START = start
            return words
    raise AssertionError("no start gives 240 crowded buckets")


def _size_border(n):
    """half the features on five heavy words, the rest spread over the tree (stop words among them), shuffled"""
    rng = np.random.default_rng(8000 + n)
    live = live_words()
    heavy = live[[7, len(live) // 4, len(live) // 2, 3 * len(live) // 4, len(live) - 3]]
    words = np.concatenate([heavy[rng.integers(0, 5, n // 2)], rng.integers(0, FULL_K ** FULL_L, n - n // 2)])
    return frame_for_histogram(full_vocab(), words[rng.permutation(n)], np.ones(n, np.int64))


def _nw_border(nw):
    rng = np.random.default_rng(7000 + nw)
    live = live_words()
    words = live[rng.permutation(len(live))[:nw]]
    counts = rng.integers(1, 4, nw)
    return frame_for_histogram(full_vocab(), words, counts, rng.permutation(int(counts.sum())))


def _build_cases():
    voc, live, stop = full_vocab(), live_words(), stop_words()
    cw = _crowd_words()
    cases = {
        "one_word": frame_for_histogram(voc, [live[len(live) // 3]], [4096]),
        "two_ends": frame_for_histogram(voc, [live[0], live[-1]], [2048, 2048]),
        "crowd_240": frame_for_histogram(voc, cw, [17] * 240),
        "crowd_240_of_16": frame_for_histogram(voc, cw, [16] * 240),
        "crowd_240_shuffled": frame_for_histogram(voc, cw, [17] * 240, np.random.default_rng(240).permutation(4080)),
        "all_stopped": frame_for_histogram(voc, stop[:100], [3] * 100),
    }
    one = cases["all_stopped"].copy()
    one[137] = voc["desc"][np.flatnonzero(voc["is_leaf"])[live[len(live) // 2]]]
    cases["one_survivor"] = one
    for nw in (1, 63, 64, 65, 127, 128, 129):
        cases["nw_border_%d" % nw] = _nw_border(nw)
    for n in (2, 3, 4095, 4096, 4097, 8191, 8192, 8193):
        cases["size_border_%d" % n] = _size_border(n)
    return cases


def cases():
    """name -> descriptors (n x 32) of every case, built once"""
    if "cases" not in _full:
        _full["cases"] = _build_cases()
    return _full["cases"]


def alternating_order(names):
    """the cases ordered so that large and small sort sizes P alternate on one handle"""
    by_p = sorted(names, key=lambda k: (sort_P(len(cases()[k])), k))
    out = []
    while by_p:
        out.append(by_p.pop())
        if by_p:
            out.append(by_p.pop(0))
    return out


_oracle_vocs = {}


def oracle_vocabulary(ob, scoring, weighting):
    """the full tree on the oracle, one object per (scoring, weighting)"""
    if (scoring, weighting) not in _oracle_vocs:
        v = full_vocab()
        _oracle_vocs[(scoring, weighting)] = ob.Vocabulary(FULL_K, FULL_L, scoring, weighting, v["parent"], v["is_leaf"], v["desc"], v["weight"])
    return _oracle_vocs[(scoring, weighting)]


def oracle_transform(ob, name, scoring, weighting, levelsup):
    """the oracle's transform of a case on the full tree, computed once per (case, scoring, weighting, levelsup)"""
    key = (name, scoring, weighting, levelsup)
    res = _full.setdefault("want", {})
    if key not in res:
        res[key] = oracle_vocabulary(ob, scoring, weighting).transform(cases()[name], levelsup)
    return res[key]
