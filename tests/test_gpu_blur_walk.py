"""k_blur_walk, the throughput path's Gaussian (a workgroup walks a 120-pixel tile column in 32-row steps and carries
the previous step's horizontal product in registers): every blurred level byte for byte against the oracle's
GaussianBlur of the same level, on the shapes where a walk can go wrong.  Batches of three frames -- a pseudo-random
one, an all-0 and an all-255 one (saturation, the +-128 byte split) -- so that the throughput path runs and the frame
index matters."""
import ctypes as C

import numpy as np
import pytest

from conftest import frames_for

pytestmark = pytest.mark.gpu


def run_length():
    from orbslamm_amd import _lib
    k = C.c_int()
    ops = np.zeros((4, 64, 4), np.uint32)
    assert _lib.lib().orbx_debug_blur_ops(1, ops.ctypes.data_as(C.c_void_p), C.byref(k)) == 0
    return k.value


def check_shape(oracle, w, h, nl, nf=300):
    from orbslamm_amd import ORBextractor
    fr = np.stack([frames_for(w, h, 1, stream=3)[0], np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)])
    gex = ORBextractor(nf, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=3, device=0)
    gex.extract_batch(fr)
    for f in range(3):
        for lvl in range(nl):
            src = fr[f] if lvl == 0 else gex.pyramid_level(f, lvl)
            got = gex.pyramid_level(f, lvl, blurred=True)
            ref = oracle.gaussian7(src)
            assert got.shape == ref.shape
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, "%dx%d frame %d level %d (%dx%d): %d bytes differ, first at row %d column %d" % (
                w, h, f, lvl, src.shape[1], src.shape[0], len(bad), bad[0][0], bad[0][1])


@pytest.mark.parametrize("w,h,nl", [
    (121, 33, 8),     # two columns, the right one a pixel wide; a second step whose input is one row
    (120, 32, 1),     # exactly one tile: the flush step has no row of its own
    (128, 70, 8),     # three steps, the last partial: the carry crosses two boundaries
    (250, 38, 8),     # h - 32 = 6: the flush step's input is as tall as the halo
    (64, 13, 1),      # the single-reflection loader (h >= 12) ...
    (40, 11, 1),      # ... and the looping one (h < 12)
    (64, 59, 1),      # the last step emits exactly one row
    (1241, 376, 8),   # the workload's shape: every level, the real columns and run cut
])
def test_walk_equals_the_oracles_gaussian(gpu, oracle, w, h, nl):
    check_shape(oracle, w, h, nl)


def test_run_boundary_one_row_before_the_end(gpu, oracle):
    """columns taller than one run of k steps: 32k + 1 rows (k + 1 steps, two runs) and 32k + 27 (k + 2 steps)"""
    k = run_length()
    check_shape(oracle, 250, 32 * k + 1, 1)
    check_shape(oracle, 250, 32 * k + 27, 1)
