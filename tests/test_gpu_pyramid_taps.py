"""k_pyramid's row loop (a dword group's eight taps of a source row read as one 8-byte LDS window, a byte permute and an
unsigned 16-bit dot per horizontal sum): every pyramid level byte for byte against the oracle's pyramid, on the shapes
where a window can go wrong -- every residue of the first tap with both tap spans, the wider spans of scale 1.5, tail
groups (level widths that are no multiple of four), the XCD block map (eight frames and more) and the latency grid
(max_batch = 1).  Five frames per case: a pseudo-random one, all 0, all 255, columns alternating 0 / 255 (the largest
horizontal sums beside the smallest) and a horizontal ramp."""
import numpy as np
import pytest

from conftest import frames_for

pytestmark = pytest.mark.gpu

_ORACLE_LEVELS = {}


def case_frames(w, h):
    x = np.arange(w)
    return np.stack([
        frames_for(w, h, 1, stream=5)[0],
        np.zeros((h, w), np.uint8),
        np.full((h, w), 255, np.uint8),
        np.broadcast_to(((x & 1) * 255).astype(np.uint8), (h, w)),
        np.broadcast_to((x * 255 // max(w - 1, 1)).astype(np.uint8), (h, w)),
    ]).copy()


def oracle_levels(oracle, w, h, nl, scale):
    """[frame][level] of the oracle's pyramid for the case's five frames; computed once per shape, never modified"""
    key = (w, h, nl, scale)
    if key not in _ORACLE_LEVELS:
        oex = oracle.Extractor(300, scale, nl, 20, 7)
        per_frame = []
        for fr in case_frames(w, h):
            pyr, off, lv = oex(fr, want_pyramid=True)["pyramid"], 0, []
            for l in range(nl):
                lw, lh = oex.level_size(w, h, l)
                a = pyr[off:off + lw * lh].reshape(lh, lw)
                a.flags.writeable = False
                lv.append(a)
                off += lw * lh
            per_frame.append(lv)
        _ORACLE_LEVELS[key] = per_frame
    return _ORACLE_LEVELS[key]


def check(oracle, w, h, nl, scale, max_batch, order):
    """extract the case's frames in the given order (indices into the five frames, max_batch of them per call) and
    compare every level of every frame of every call"""
    from orbslamm_amd import ORBextractor
    frames, ref = case_frames(w, h), oracle_levels(oracle, w, h, nl, scale)
    gex = ORBextractor(300, scale, nl, 20, 7, max_width=w, max_height=h, max_batch=max_batch, device=0)
    for c0 in range(0, len(order), max_batch):
        call = order[c0:c0 + max_batch]
        gex.extract_batch(frames[call])
        for slot, f in enumerate(call):
            assert np.array_equal(ref[f][0], frames[f])
            for lvl in range(1, nl):
                got = gex.pyramid_level(slot, lvl)
                want = ref[f][lvl]
                assert got.shape == want.shape
                bad = np.argwhere(got != want)
                assert len(bad) == 0, "%dx%d scale %.1f batch %d frame %d level %d (%dx%d): %d bytes differ, first at row %d column %d: %d, want %d" % (
                    w, h, scale, max_batch, f, lvl, want.shape[1], want.shape[0], len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("w,h,nl,scale", [
    (121, 33, 8, 1.2),     # the block grid collapses; the tables hold all eight combinations of sx[0] & 3 with sx[3] - sx[0] in {3, 4}
    (640, 480, 5, 1.5),    # offsets 4 and 5 of the last pixel's first tap
    (640, 480, 12, 1.1),   # twelve levels
])
def test_levels_equal_the_oracles(gpu, oracle, w, h, nl, scale):
    check(oracle, w, h, nl, scale, 5, [0, 1, 2, 3, 4])


def test_workload_shape_batch_of_three(gpu, oracle):
    """1241 x 376: level widths 1034, 862, ... are no multiples of four, so tail groups occur; the plain (block, frame) grid"""
    check(oracle, 1241, 376, 8, 1.2, 3, [0, 1, 2, 3, 4, 0])


def test_workload_shape_batch_of_nine(gpu, oracle):
    """nine frames in one call: a frame's blocks go to one XCD (the block map of eight frames and more)"""
    check(oracle, 1241, 376, 8, 1.2, 9, [4, 3, 2, 1, 0, 1, 2, 3, 4])


def test_workload_shape_latency_grid(gpu, oracle):
    """max_batch = 1: the latency handle's finer block grid runs the same kernel"""
    check(oracle, 1241, 376, 8, 1.2, 1, [0, 1, 2, 3, 4])
