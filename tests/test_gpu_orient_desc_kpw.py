"""k_orient_desc with eight keypoints per wave (the throughput path: calls of more than two frames) against the CPU oracle:
keypoint records and descriptor bytes, bit for bit, on per-level counts that leave eighths, waves and whole blocks of the
kernel idle; the same frames through the four-keypoint form (a call of one frame); and the stream matcher, which reads the
+-1 descriptors and the angle array the kernel writes.  Batches of 3 so that the throughput kernel runs."""
import numpy as np
import pytest

from conftest import frames_for

pytestmark = pytest.mark.gpu
W, H = 324, 240
PRM = (1.2, 8, 20, 7)   # scale factor, levels, iniThFAST, minThFAST

# bright rectangles (x, y, w, h, value) on a flat frame: a handful of corners per level
SPARSE = (
    ((218, 33, 12, 14, 144), (215, 159, 25, 7, 132), (101, 89, 27, 22, 155)),
    ((183, 148, 6, 33, 183), (145, 120, 15, 39, 127), (87, 81, 25, 19, 137), (31, 20, 7, 11, 254), (66, 124, 31, 13, 158)),
    ((135, 101, 31, 38, 124), (55, 151, 38, 14, 162)),
)


def sparse_frames():
    out = np.full((len(SPARSE), H, W), 60, np.uint8)
    for img, rects in zip(out, SPARSE):
        for x, y, w, h, v in rects:
            img[y:y + h, x:x + w] = v
    return out


def mixed_frames():
    """one textured, one all-zero and one half-flat frame"""
    tex = frames_for(W, H, 2, stream=3)
    half = tex[1].copy()
    half[:, W // 2:] = 90
    return np.stack([tex[0], np.zeros((H, W), np.uint8), half])


def gpu_extractor(nf, B=3):
    from orbslamm_amd import ORBextractor
    return ORBextractor(nf, *PRM, max_width=W, max_height=H, max_batch=B, device=0)


_REF = {}


def reference(oracle, key, nf, frames):
    """the oracle's result per frame, computed once per case and shared"""
    if key not in _REF:
        oex = oracle.Extractor(nf, *PRM)
        _REF[key] = [oex(f) for f in frames]
    return _REF[key]


def level_counts(ref):
    return [np.bincount(r["kps"]["octave"], minlength=PRM[1]).tolist() for r in ref]


def assert_same(ref, kps, desc):
    assert len(ref["kps"]) == len(kps)
    for name in ref["kps"].dtype.names:
        assert np.array_equal(ref["kps"][name], kps[name]), "field " + name
    assert ref["kps"].tobytes() == kps.tobytes()
    assert np.array_equal(ref["desc"], desc)


def test_500_features_counts_off_the_wave_and_block_sizes(gpu, oracle):
    fr = frames_for(W, H, 3, stream=0)
    ref = reference(oracle, "tex500", 500, fr)
    counts = level_counts(ref)
    print("per-level counts", counts)
    flat = [c for fc in counts for c in fc]
    assert all(c > 16 for c in flat)                                # every level: more than one block
    assert sum(c % 8 != 0 for c in flat) >= 20                      # a last wave with idle eighths on almost every level
    assert {c % 16 for c in flat} >= {1, 5, 6, 10, 12, 13, 14, 15}  # block tails of one and of two waves, (nearly) full and nearly empty
    assert 64 in flat                                               # and a level that fills its last block exactly
    kps, desc = gpu_extractor(500).extract_batch(fr)
    for f in range(3):
        assert_same(ref[f], kps[f], desc[f])


@pytest.mark.parametrize("nf,occurred", [(20, {4, 8}), (37, {4, 7, 8, 10})])
def test_few_features(gpu, oracle, nf, occurred):
    """the quadtree's floor: levels of 4 keypoints (half a wave), of exactly 8 (one wave, the block's second one idle), 7 and 10"""
    fr = frames_for(W, H, 3, stream=0)
    ref = reference(oracle, "tex%d" % nf, nf, fr)
    counts = level_counts(ref)
    print("per-level counts", counts)
    assert {c for fc in counts for c in fc} == occurred
    kps, desc = gpu_extractor(nf).extract_batch(fr)
    for f in range(3):
        assert_same(ref[f], kps[f], desc[f])


def test_sparse_frames_levels_of_one_to_three_and_wave_edges(gpu, oracle):
    """levels of 0, 1, 2 and 3 keypoints and of exactly 8, 9, 16 and 17 (the textured frames above never give those)"""
    fr = sparse_frames()
    ref = reference(oracle, "sparse", 500, fr)
    counts = level_counts(ref)
    print("per-level counts", counts)
    assert {c for fc in counts for c in fc} >= {0, 1, 2, 3, 8, 9, 16, 17}
    kps, desc = gpu_extractor(500).extract_batch(fr)
    for f in range(3):
        assert_same(ref[f], kps[f], desc[f])


def test_textured_zero_and_half_flat_frame_in_one_batch(gpu, oracle):
    """waves and whole blocks with no active keypoint, and a frame of count 0 between live ones"""
    fr = mixed_frames()
    ref = reference(oracle, "mixed", 500, fr)
    n = [len(r["kps"]) for r in ref]
    print("keypoints per frame", n, "per-level counts", level_counts(ref))
    assert n[0] > 400 and n[1] == 0 and n[2] > 400
    kps, desc = gpu_extractor(500).extract_batch(fr)
    for f in range(3):
        assert_same(ref[f], kps[f], desc[f])


def test_one_frame_calls_equal_the_batch_of_three(gpu, oracle):
    """a call of one frame runs four keypoints per wave, the call of three runs eight: identical bytes, and the oracle's"""
    fr = mixed_frames()
    ref = reference(oracle, "mixed", 500, fr)
    gex = gpu_extractor(500)
    single = [gex.extract_batch(fr[f:f + 1]) for f in range(3)]
    kps, desc = gex.extract_batch(fr)
    for f in range(3):
        k1, d1 = single[f][0][0], single[f][1][0]
        assert k1.tobytes() == kps[f].tobytes() and np.array_equal(d1, desc[f])
        assert_same(ref[f], kps[f], desc[f])


def test_two_batches_and_the_stream_matcher(gpu, oracle):
    """the consumer of the +-1 descriptors and the angle array: every frame of two consecutive calls of three against its
    predecessor, the second call's first frame against the first call's last"""
    fr = frames_for(W, H, 6, stream=2)
    ref = reference(oracle, "tex500x6", 500, fr)
    gex = gpu_extractor(500)
    prev = None
    for b in range(2):
        gex.extract_batch_device(*gex.upload_frames(fr[3 * b:3 * b + 3]))
        gex.match_prev_batch_device(0.7, 50, True)
        for f in range(3):
            r = ref[3 * b + f]
            k, d = gex.download(f)
            assert_same(r, k, d)
            m, nm = gex.download_matches(f)
            if prev is None:
                assert nm == 0 and (m[:len(k)] == -1).all()   # no previous frame in a fresh stream
            else:
                mr, nr = oracle.match_bruteforce(r["desc"], r["kps"]["angle"], prev["desc"], prev["kps"]["angle"], 0.7, 50, True)
                assert nr > 50
                assert nm == nr and np.array_equal(m[:len(k)], mr)
            prev = r
