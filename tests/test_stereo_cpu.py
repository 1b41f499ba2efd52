"""The scenes of stereo_cases.py reach the branches they are built for: the oracle's census of
Frame::ComputeStereoMatches (binding.STEREO_BRANCHES) is held to floors, so that the byte comparison of
test_gpu_stereo.py on the same scenes is a comparison of those branches.  No GPU."""
import numpy as np
import pytest

import stereo_cases as sc

# branches a scene can reach, and the floor of their count over all scenes
REACHED = {"row_empty": 10, "octave_gate": 10, "ur_below_minu": 10, "ur_above_maxu": 10, "no_descriptor": 10, "bestinc_at_end": 10,
           "disparity_negative": 10, "disparity_ge_maxd": 10, "clamp": 17, "median_removed": 10, "accepted": 10}
# branches that must stay at zero, with the reason:
#  - the three window checks, both row clips, row_outside, maxu_negative: orbx_compute_stereo_matches only ever sees the
#    extractor's own keypoints, which sit at least EDGE_THRESHOLD = 19 px inside every level (the windows need 16, a
#    row band 2 * 1.2^7 < 8 px); minD = -3 makes maxU = uL + 3 >= 3;
#  - delta_nan, delta_beyond_one: the chosen dist2 is strictly below dist1 (strict < in ascending shift order) and not
#    above dist3, so the denominator (d1 - d2) + (d3 - d2) is positive and at least |d1 - d3|: |deltaR| <= 0.5.
UNREACHABLE = ("row_outside", "maxu_negative", "window_left", "window_ref_right", "window_right", "delta_nan", "delta_beyond_one",
               "minr_clipped", "maxr_clipped")

ALL_SCENES = tuple(sc.SCENES) + tuple("small_sets:%d" % nf for nf in sc.SMALL_SETS)


def test_the_census_names_every_branch(oracle):
    assert set(REACHED) | set(UNREACHABLE) == set(oracle.STEREO_BRANCHES)
    assert not set(REACHED) & set(UNREACHABLE)


def test_every_reachable_branch_is_taken(oracle):
    total = dict.fromkeys(oracle.STEREO_BRANCHES, 0)
    for name in sc.SCENES:
        for b, c in sc.scene(oracle, name)["census"].items():
            total[b] += c
    print(total)
    for b, floor in REACHED.items():
        assert total[b] >= floor, (b, total[b])


@pytest.mark.parametrize("name", ALL_SCENES)
def test_unreachable_branches_stay_at_zero(oracle, name):
    census = sc.scene(oracle, name)["census"]
    for b in UNREACHABLE:
        assert census[b] == 0, (name, b, census[b])


@pytest.mark.parametrize("name", ALL_SCENES)
def test_the_census_changes_no_output(oracle, name):
    r = sc.scene(oracle, name)
    oex = oracle.Extractor(r["nf"], *sc.EXTRACTOR)
    sf = oex.scale_factors()
    u, d, accepted = oracle.compute_stereo_matches(r["oL"]["kps"], r["oL"]["desc"], r["oR"]["kps"], r["oR"]["desc"], sc.levels_of(oex, r["oL"]["pyramid"]),
                                                   sc.levels_of(oex, r["oR"]["pyramid"]), sf, (1.0 / sf).astype(np.float32), r["mb"], r["mbf"])
    assert u.tobytes() == r["u"].tobytes() and d.tobytes() == r["d"].tobytes() and accepted == r["accepted"]
    assert r["census"]["accepted"] == accepted
    assert (r["u"] >= 0).sum() == accepted - r["census"]["median_removed"]


def test_near_crosses_the_far_end_of_the_range(oracle):
    r = sc.scene(oracle, "near")
    assert np.float32(r["mbf"]) / np.float32(r["mb"]) == 14.0
    c = r["census"]
    print(c)
    assert c["disparity_ge_maxd"] >= 10 and c["ur_below_minu"] >= 10 and c["accepted"] >= 100


def test_zero_keeps_its_clamped_matches(oracle):
    """the clamp is only observed if the median filter leaves the clamped matches in"""
    r = sc.scene(oracle, "zero")
    uL = r["oL"]["kps"]["x"]
    clamped = r["d"] == np.float32(r["mbf"]) / np.float32(0.01)
    print(r["census"], int(clamped.sum()))
    assert r["census"]["clamp"] >= 17 and clamped.sum() >= 17
    assert np.array_equal(r["u"][clamped], (uL[clamped].astype(np.float64) - 0.01).astype(np.float32))
    # (a binary32 `uL - 0.01f` gives the same bytes at every coordinate a keypoint of these frames can have: 0.01f is
    # 2.2e-10 off 0.01 and an ulp of uL >= 19 is 1.9e-6.  The value is pinned; the two forms cannot be told apart.)
    assert (r["u"][~clamped] >= 0).sum() >= 100          # the textured half keeps the median above 0


def test_blank_sides(oracle):
    r = sc.scene(oracle, "right_blank")
    n = len(r["oL"]["kps"])
    assert n >= 400 and len(r["oR"]["kps"]) == 0 and r["census"]["row_empty"] == n
    assert np.all(r["u"] == -1) and np.all(r["d"] == -1) and r["accepted"] == 0
    l = sc.scene(oracle, "left_blank")
    assert len(l["oL"]["kps"]) == 0 and len(l["oR"]["kps"]) >= 400 and len(l["u"]) == 0 and sum(l["census"].values()) == 0


def test_sparse_right_mixes_empty_rows_and_matches(oracle):
    c = sc.scene(oracle, "sparse_right")["census"]
    print(c)
    assert c["row_empty"] >= 10 and c["accepted"] - c["median_removed"] >= 10


def test_small_sets_counts(oracle):
    """k_stereo_median takes the key of rank n / 2: one element, even and odd counts, and no more than 3"""
    got = {nf: sc.scene(oracle, "small_sets:%d" % nf)["accepted"] for nf in sc.SMALL_SETS}
    assert got == sc.SMALL_SETS
    counts = set(got.values())
    assert 1 in counts and any(c % 2 == 0 for c in counts) and any(c % 2 == 1 and c > 1 for c in counts) and min(counts) <= 3
