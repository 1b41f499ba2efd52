"""Rectified stereo pairs built to force the branches of Frame::ComputeStereoMatches (src/Frame.cc:466-638) that a
plausible scene never reaches: the far end of the disparity range, the clamp of a zero disparity, empty frames on either
side, rows without a candidate and accepted sets of one to three.  The oracle's census (binding.STEREO_BRANCHES) counts
the branches; test_stereo_cpu.py holds the counts to floors, test_gpu_stereo.py compares the kernels' bytes on the same
scenes.  Everything is 320 x 240, 8 levels, 1.2 -- an oracle run takes well under a second."""
import numpy as np

W, H, NF, NLEVELS = 320, 240, 500, 8
EXTRACTOR = (1.2, NLEVELS, 20, 7)


def _texture(stream):
    from orbslamm_amd import synth
    return synth.make_frames(W, H, 1, stream=stream)[0]


def _shift(left, bands, seed, noise=3):
    """right(x) = left(x + d) by horizontal band (y0, y1, d), fresh sensor noise of +-`noise` on the right image"""
    right = np.empty_like(left)
    for y0, y1, d in bands:
        right[y0:y1] = np.roll(left[y0:y1], -d, axis=1)
    rng = np.random.default_rng(seed)
    return np.clip(right.astype(np.int16) + rng.integers(-noise, noise + 1, size=right.shape), 0, 255).astype(np.uint8)


def _near():
    left = _texture(3)
    return left, _shift(left, [(0, H // 2, 6), (H // 2, H, 14)], seed=14)


def _zero():
    """top half: texture at 9 px; bottom half: flat 40 with single pixels of 220 on a 26 px lattice, the same bytes in
    both images.  A single pixel is a level-0 FAST corner whose 11 SADs are mirror-symmetric about shift 0, so deltaR is
    0 and the disparity exactly 0.  maxD = 20 < 26 keeps the lattice neighbour to the left out of the candidates (all
    lattice descriptors are equal, so it would win on its lower index)."""
    left = _texture(5).copy()
    right = _shift(left, [(0, H, 9)], seed=9)
    for img in (left, right):
        img[H // 2:] = 40
        img[H // 2 + 22:H - 19:26, 23:W - 19:26] = 220
    return left, right


def _right_blank():
    return _texture(3), np.full((H, W), 128, np.uint8)


def _left_blank():
    return np.full((H, W), 128, np.uint8), _texture(3)


def _sparse_right():
    left = _texture(7)
    right = np.full((H, W), 128, np.uint8)
    right[96:150] = _shift(left, [(0, H, 6)], seed=6)[96:150]
    return left, right


def _small():
    """the right image is textured in rows 40-59 only: a sweep of nfeatures alone never gets below ~30 accepted matches
    (the octree keeps at least four or five keypoints per level), the band brings the counts down to 1"""
    left = _texture(11)
    right = np.full((H, W), 128, np.uint8)
    right[40:60] = _shift(left, [(0, H, 6)], seed=11)[40:60]
    return left, right


# name -> (builder, nfeatures, mb, mbf); maxD = mbf / mb
SCENES = {
    "near": (_near, NF, 0.5, 7.0),                    # maxD exactly 14: the 14 px band straddles `disparity < maxD`
    "zero": (_zero, NF, 0.5, 10.0),
    "right_blank": (_right_blank, NF, 0.5, 40.0),
    "left_blank": (_left_blank, NF, 0.5, 40.0),
    "sparse_right": (_sparse_right, NF, 0.5, 40.0),
}
# the order the GPU test feeds one pair of handles: N and Nr fall to 0 and rise again
SCENE_ORDER = ("near", "right_blank", "zero", "left_blank", "sparse_right", "near")

# small_sets: one pair, the extractor's nfeatures swept; nfeatures -> accepted count before the median filter, as the
# oracle gave them.  k_stereo_median indexes its sorted keys at n / 2: an even n, an odd one, and n <= 3.
SMALL_SETS = {20: 1, 29: 2, 33: 3, 50: 5, 65: 6}
SMALL_MB, SMALL_MBF = 0.5, 40.0

_cache = {}


def levels_of(oex, pyr):
    out, o = [], 0
    for l in range(NLEVELS):
        lw, lh = oex.level_size(W, H, l)
        out.append(pyr[o:o + lw * lh].reshape(lh, lw))
        o += lw * lh
    return out


def run_oracle(ob, left, right, nf, mb, mbf):
    """-> dict(left, right, oL, oR, u, d, accepted, census) of one pair through the oracle's extractor and stereo matcher"""
    oex = ob.Extractor(nf, *EXTRACTOR)
    oL, oR = oex(left, want_pyramid=True), oex(right, want_pyramid=True)
    sf = oex.scale_factors()
    u, d, accepted, census = ob.compute_stereo_matches(oL["kps"], oL["desc"], oR["kps"], oR["desc"], levels_of(oex, oL["pyramid"]),
                                                       levels_of(oex, oR["pyramid"]), sf, (1.0 / sf).astype(np.float32), mb, mbf, census=True)
    return dict(left=left, right=right, nf=nf, mb=mb, mbf=mbf, oL=oL, oR=oR, u=u, d=d, accepted=accepted, census=census)


def scene(ob, name):
    """the oracle's result on a named scene ("small_sets:<nfeatures>" for one step of the sweep), computed once"""
    if name not in _cache:
        if name.startswith("small_sets:"):
            left, right = _small()
            _cache[name] = run_oracle(ob, left, right, int(name.split(":")[1]), SMALL_MB, SMALL_MBF)
        else:
            build, nf, mb, mbf = SCENES[name]
            left, right = build()
            _cache[name] = run_oracle(ob, left, right, nf, mb, mbf)
    return _cache[name]
