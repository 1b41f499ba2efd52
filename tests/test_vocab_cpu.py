"""Vocabulary-tree descent: the oracle against an independent Python re-derivation of DBoW2's
transform (the DBoW2 source is vendored in the reference, so this arithmetic is pinned by source).

The vocabulary cases of vocab_cases.py reach the paths they are named for -- proved with the oracle's transform_one
and a model of the kernel's bucket map -- and the oracle agrees with naive_transform on them too.  No GPU;
test_gpu_vocab.py compares the kernels' bytes on the same frames."""
import numpy as np
import pytest

import vocab_cases as vc
from vocab_cases import make_vocab, naive_transform


@pytest.mark.parametrize("scoring,weighting", [(0, 0), (1, 1), (5, 0), (0, 2), (5, 3), (2, 1)])
def test_oracle_transform_equals_naive(oracle, scoring, weighting):
    rng = np.random.default_rng(40 + scoring * 4 + weighting)
    voc = make_vocab(rng, 6, 4)
    V = oracle.Vocabulary(6, 4, scoring, weighting, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    desc = rng.integers(0, 256, size=(300, 32), dtype=np.uint8)
    for levelsup in (0, 2, 4, 6):
        (wi, wv), (fn, fs, fi) = V.transform(desc, levelsup)
        (ni, nv), (nn, ns, nx) = naive_transform(voc, scoring, weighting, desc, levelsup)
        assert np.array_equal(wi, ni) and np.array_equal(wv, nv)          # doubles bit-for-bit
        assert np.array_equal(fn, nn) and np.array_equal(fs, ns) and np.array_equal(fi, nx)
    if scoring == 0:
        assert abs(wv.sum() - 1.0) < 1e-12


NAIVE_CASES = ("one_word", "two_ends", "crowd_240", "crowd_240_of_16", "crowd_240_shuffled", "all_stopped", "one_survivor",
               "nw_border_1", "nw_border_63", "nw_border_64", "nw_border_65", "nw_border_127", "nw_border_128", "nw_border_129",
               "size_border_2", "size_border_3", "size_border_4095")     # (the larger size_border frames are too slow in Python)


_memo = {}     # naive_transform's paths on the full tree


@pytest.fixture(scope="module")
def streams(oracle):
    """name -> (word, weight) of every feature, from the oracle's transform_one: what the frames really are"""
    v = vc.full_vocab()
    O = oracle.Vocabulary(vc.FULL_K, vc.FULL_L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"])
    return {name: O.transform_one(desc, 2)[:2] for name, desc in vc.cases().items()}


def _crowded(word, weight, n):
    ids = np.where(weight > 0, word.astype(np.int64), -1)
    return vc.bucket_model(ids, vc.sort_P(n))


def test_every_leaf_descends_to_itself(oracle):
    v = vc.full_vocab()
    assert len(v["parent"]) == 11110 and 300 < len(vc.stop_words()) < 700
    O = oracle.Vocabulary(vc.FULL_K, vc.FULL_L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"])
    word, w, _ = O.transform_one(v["desc"][np.flatnonzero(v["is_leaf"])], 0)
    assert np.array_equal(word, np.arange(10000)) and np.array_equal(w, v["weight"][np.flatnonzero(v["is_leaf"])])


def test_case_preconditions(streams):
    word, w = streams["one_word"]
    assert len(word) == 4096 and len(set(word.tolist())) == 1 and np.all(w > 0)

    word, w = streams["two_ends"]
    live = vc.live_words()
    assert np.all(word[:2048] == live[0]) and np.all(word[2048:] == live[-1]) and np.all(w > 0)
    b = _crowded(word, w, 4096)
    assert sorted(b[b > 0].tolist()) == [2048, 2048]                  # two buckets of half a frame each

    for name in ("crowd_240", "crowd_240_of_16", "crowd_240_shuffled"):
        word, w = streams[name]
        per = 16 if name.endswith("16") else 17
        assert len(set(word.tolist())) == 240 and np.all(np.bincount(word)[np.unique(word)] == per) and np.all(w > 0)
        assert np.all(np.diff(np.unique(word)) >= 38) and np.all(np.diff(np.unique(word)) <= 44)   # "41 ids apart", moved off stop words
    b = _crowded(*streams["crowd_240"], 4080)
    assert (b > vc.K_CROWD).sum() == 240 and b.max() == 17            # the crowd list's argued maximum, exactly
    assert (_crowded(*streams["crowd_240_of_16"], 3840) > vc.K_CROWD).sum() == 0   # the 16 | 17 border from below
    b = _crowded(*streams["crowd_240_shuffled"], 4080)
    print("crowded buckets, shuffled:", int((b > vc.K_CROWD).sum()))
    # a word's 17 keys now differ in the feature term, which moves a key by less than 4080 / (2 * 9800) = 0.21 buckets:
    # no more than about a fifth of the words can straddle a bucket border, so well over half stay crowded
    assert (b > vc.K_CROWD).sum() >= 120

    word, w = streams["all_stopped"]
    assert len(word) == 300 and np.all(w == 0)
    word, w = streams["one_survivor"]
    assert (w > 0).sum() == 1 and w[137] > 0

    for nw in (1, 63, 64, 65, 127, 128, 129):
        word, w = streams["nw_border_%d" % nw]
        assert len(set(word.tolist())) == nw and np.all(w > 0) and np.bincount(word).max() <= 3
    for n in (2, 3, 4095, 4096, 4097, 8191, 8192, 8193):
        word, w = streams["size_border_%d" % n]
        assert len(word) == n
        if n > 1000:
            assert np.sort(np.bincount(word[w > 0]))[-5] > 300      # five words of hundreds of addends each
    # the three placements' borders, exactly: P <= 4096 (word values in LDS), <= 8192 (keys in LDS), beyond (memory)
    assert [vc.sort_P(n) for n in (4095, 4096, 4097, 8191, 8192, 8193)] == [4096, 4096, 8192, 8192, 8192, 16384]


@pytest.mark.parametrize("name", ("one_word", "crowd_240"))
def test_repeated_sum_is_not_the_product(oracle, name):
    """addWeight's sequential += (BowVector.cpp:34-46) is what the kernel has to reproduce: if count * weight gave the
    same bits, the cases could not tell the two apart"""
    (ids, vals), _ = vc.oracle_transform(oracle, name, 5, 0, 2)     # TF-IDF, no normalisation: value = sum / number of words
    v = vc.full_vocab()
    wt = v["weight"][np.flatnonzero(v["is_leaf"])][ids]
    count = 4096 if name == "one_word" else 17
    product = (count * wt) / float(len(ids))
    assert np.any(vals.view(np.uint64) != product.view(np.uint64))
    assert np.allclose(vals, product, rtol=1e-12)


@pytest.mark.parametrize("scoring,weighting", vc.PAIRS)
def test_oracle_equals_naive_transform(oracle, scoring, weighting):
    v = vc.full_vocab()
    for levelsup in vc.LEVELSUP:
        for name in NAIVE_CASES:
            (oi, ov), (on, os_, ox) = vc.oracle_transform(oracle, name, scoring, weighting, levelsup)
            (ni, nv), (nn, ns, nx) = vc.naive_transform(v, scoring, weighting, vc.cases()[name], levelsup, _memo)
            assert np.array_equal(oi, ni) and ov.tobytes() == nv.tobytes(), (name, levelsup)
            assert np.array_equal(on, nn) and np.array_equal(os_, ns) and np.array_equal(ox, nx), (name, levelsup)
            for a, b in zip(os_[:-1], os_[1:]):
                assert np.all(np.diff(ox[a:b]) > 0)                 # feature indices ascend within a node


def test_empty_results_of_the_stopped_frame(oracle):
    for scoring, weighting in vc.PAIRS:
        (oi, ov), (on, os_, ox) = vc.oracle_transform(oracle, "all_stopped", scoring, weighting, 2)
        assert len(oi) == 0 and len(ov) == 0 and len(on) == 0 and len(ox) == 0 and os_.tolist() == [0]
        (oi, ov), (on, os_, ox) = vc.oracle_transform(oracle, "one_survivor", scoring, weighting, 2)
        assert len(oi) == 1 and ox.tolist() == [137] and os_.tolist() == [0, 1]
