"""The rotation-consistency check of the matchers (ORBmatcher.cc:238-287) has one statement, orbm::three_maxima next to rot_bin in
orbslamm_amd/csrc/orbm_kernels.hip, and every pruning kernel calls it.  No GPU here: (a) its host instantiation
(tests/cpp/rot_rule_check.hip) against the oracle's orc_three_maxima on designed histograms -- ties, shifting indices, the 10 % rule at
and around its threshold -- and on seeded random ones with small counts; (b) each shared piece of the matcher has one definition;
(c) the designed match cases of tests/matcher_cases.py do what they claim through every oracle entry, which is what keeps the GPU
tests on the same cases (tests/test_gpu_rot_rule.py) from passing vacuously."""
import os
import re
import subprocess

import numpy as np
import pytest

from matcher_cases import ROT_CLASSES, assert_rot_case_is_designed, make_rot_case, oracle_three_maxima, rot_oracle_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbslamm_amd", "csrc")


def _hist(counts):
    h = np.zeros(30, np.int32)
    for b, c in counts.items():
        h[b] = c
    return h


def _designed_histograms():
    """class -> histograms.  The classes of ROT_CLASSES where they lie and moved to the last bins, and what a match case of a few
    hundred features cannot hold: a first maximum of 1000, every bin equal, the threshold met by the third bin alone."""
    out = {}
    for name, (counts, _, _) in ROT_CLASSES.items():
        out[name] = [_hist(counts), _hist({b + 17: c for b, c in counts.items()})]
    for m in (10, 100, 1000):
        t = m // 10
        out["threshold: second at a tenth of %d" % m] = [_hist({4: m, 9: t}), _hist({9: m, 4: t}), _hist({0: m, 29: t, 15: t}), _hist({29: m, 0: t})]
        out["threshold: second one below a tenth of %d" % m] = [_hist({4: m, 9: t - 1, 20: t - 1}), _hist({20: m, 4: t - 1})] if t > 1 else [_hist({4: 11, 9: 1}), _hist({9: 21, 4: 2, 5: 1})]
        out["threshold: third at or below a tenth of %d, second above" % m] = [_hist({4: m, 9: t + 1, 20: t}), _hist({4: m, 9: m, 20: t - 1}), _hist({20: m, 9: m - 1, 4: t})]
    out["all bins equal"] = [np.full(30, v, np.int32) for v in (1, 7)]
    out["four equal, a later fifth larger"] = [_hist({2: 20, 5: 20, 7: 20, 9: 20, 25: 21}), _hist({2: 20, 5: 20, 25: 20, 28: 20, 0: 19})]
    out["rising"] = [np.arange(30, dtype=np.int32), np.arange(1, 31, dtype=np.int32)]
    out["falling"] = [np.arange(30, 0, -1).astype(np.int32)]
    return out


def test_host_instantiation_equals_the_oracle_on_designed_and_random_histograms(oracle, tmp_path):
    exe = str(tmp_path / "rot_rule_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rot_rule_check.hip")])
    classes = _designed_histograms()
    rng = np.random.default_rng(238)
    # small counts over few or many bins: ties between bins are the rule here, and max1 <= 10 puts a tenth of it at or below 1
    classes["random, counts 0..3"] = list(rng.integers(0, 4, (2000, 30)).astype(np.int32))
    classes["random, counts 0..12, sparse"] = list((rng.integers(0, 13, (2000, 30)) * (rng.random((2000, 30)) < 0.2)).astype(np.int32))
    classes["random, one large bin over small ones"] = [np.where(np.arange(30) == rng.integers(0, 30), rng.integers(5, 60), rng.integers(0, 5, 30)).astype(np.int32)
                                                        for _ in range(2000)]
    names = [n for n, hs in classes.items() for _ in hs]
    hists = [h for hs in classes.values() for h in hs]
    assert all(len(hs) > 0 for hs in classes.values()) and all(h.shape == (30,) for h in hists)
    text = "\n".join(" ".join(str(int(v)) for v in h) for h in hists) + "\n"
    run = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in run.stdout.decode().splitlines()]
    assert len(got) == len(hists)
    want = [oracle_three_maxima(oracle, h) for h in hists]
    for n, h, g, w in zip(names, hists, got, want):
        assert g == w, (n, h.tolist(), g, w)
    by = {n: [w for m, w in zip(names, want) if m == n] for n in classes}
    # the classes are what their names say, read off the oracle
    assert by["empty"] == [(-1, -1, -1)] * 2 and by["one bin"] == [(4, -1, -1), (21, -1, -1)]
    assert by["four equal"] == [(2, 5, 7), (19, 22, 24)] and by["later larger"] == [(8, 6, 3), (25, 23, 20)]
    assert by["all bins equal"] == [(0, 1, 2)] * 2 and by["rising"] == [(29, 28, 27)] * 2 and by["falling"] == [(0, 1, 2)]
    assert by["four equal, a later fifth larger"] == [(25, 2, 5), (2, 5, 25)]
    for m in (10, 100, 1000):
        at = by["threshold: second at a tenth of %d" % m]
        assert len({w[1] >= 0 for w in at}) == 1, at                 # the float compare takes one side, whichever the oracle says
        assert all(w[1] < 0 and w[2] < 0 for w in by["threshold: second one below a tenth of %d" % m])
        assert all(w[1] >= 0 for w in by["threshold: third at or below a tenth of %d, second above" % m])
        assert by["threshold: third at or below a tenth of %d, second above" % m][1][2] < 0
    assert by["second below a tenth"][0] == (0, -1, -1) and by["third below, second above"][0] == (0, 3, -1)
    ties = sum(1 for h in classes["random, counts 0..3"] if len(set(np.sort(h)[-4:].tolist())) < 4)
    dropped = sum(1 for w in by["random, one large bin over small ones"] if w[2] < 0)
    assert ties > 1900 and 100 < dropped < 1900, (ties, dropped)


def test_each_shared_piece_of_the_matcher_is_defined_once():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".inc", ".h"))}
    once = {"the three-maxima walk": (r"s > max1", "orbm_kernels.hip"), "area_window": (r"bool area_window\(", "orbm_kernels.hip"),
            "AreaWin": (r"struct AreaWin\b", "orbm_kernels.hip"), "the undistort iteration": (r"double icdist\b", "orbm_kernels.hip"),
            "RotShared": (r"struct RotShared\b", "orbm_kernels.hip"), "block_scan_excl": (r"int block_scan_excl\(", "orbx_common.hpp"),
            "hamming256": (r"int hamming256\(", "orbx_common.hpp")}
    for what, (pat, home) in once.items():
        where = [f for f, t in text.items() for _ in re.findall(pat, t)]
        assert where == [home], (what, where)
    # one call site keeps the eight popcounts written out: the BoW search's register form, where both descriptors are register arrays and
    # the call compiles to a slower kernel (docs/experiments.md); it says so, and it is the only one
    written_out = [f for f, s in text.items() for _ in re.findall(r"for \(int i = 0; i < 8; i\+\+\) d \+= __popc\(", s)]
    assert sorted(written_out) == ["orbm_kernels.hip", "orbx_common.hpp"], written_out
    assert "// hamming256, written out" in text["orbm_kernels.hip"]
    for gone in (r"\bham256\b", r"\bwg_scan_excl\b"):
        assert [f for f, t in text.items() if re.search(gone, t)] == [], gone
    # the dead histogram is gone: no global bins behind the two flat searches
    assert "int32_t* hist" not in re.search(r"struct BowArgs \{.*?\};", text["orbm_kernels.hip"], re.S).group(0)
    assert "hist" not in re.search(r"struct TriArgs \{.*?\};", text["orbm_kernels.hip"], re.S).group(0)
    assert "hist" not in re.search(r"k_prune_flat\((.*?)\)", text["orbm_kernels.hip"], re.S).group(1)


@pytest.fixture(scope="module")
def rot_cases(oracle):
    return {name: make_rot_case(oracle, name) for name in ROT_CLASSES}


@pytest.mark.parametrize("entry", ["match_bruteforce", "search_by_bow", "search_for_triangulation", "search_for_initialization", "search_by_projection"])
def test_designed_cases_prune_what_they_were_designed_to(oracle, rot_cases, entry):
    pruning = keeping = 0
    for name, c in rot_cases.items():
        assert c["n"] <= 300
        call = rot_oracle_entries(oracle, c)[entry]
        free, checked = call(False), call(True)
        assert_rot_case_is_designed(c, free, checked)
        if checked[1] < free[1]:
            pruning += 1
        else:
            keeping += 1
    assert pruning >= 4 and keeping >= 3   # (no class is empty: both kinds are there)
