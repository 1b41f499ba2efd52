"""The constant matrix-core operands of the Gaussian (orbx_kernels.hip make_blur_ops) rebuilt in numpy from the tap list
and the slot mapping the comment above them states -- no device needed."""
import ctypes as C

import numpy as np

W = [18, 34, 49, 55, 49, 34, 18]


def device_tables(walk):
    from orbslamm_amd import _lib
    ops = np.zeros((4, 64, 4), np.uint32)
    k = C.c_int()
    assert _lib.lib().orbx_debug_blur_ops(int(walk), ops.ctypes.data_as(C.c_void_p), C.byref(k)) == 0
    assert k.value >= 1
    # byte b of a lane's 16-byte fragment = contraction slot (half, b)
    return ops.view(np.uint8).reshape(4, 64, 16)


def tap(t):
    return W[t] if 0 <= t <= 6 else 0


def slot_row(hh, b):
    """the tile row that accumulator element b = 4g + j of the horizontal product holds in lane half hh"""
    return 8 * (b >> 2) + 4 * hh + (b & 3)


def expected(walk):
    e = np.zeros((4, 64, 16), np.uint8)
    for lane in range(64):
        i, hh = lane & 31, lane >> 5
        for b in range(16):
            for op in (0, 1):   # output column i reads strip columns i+1 .. i+7; slot = strip column 16 hh + b of the op-th 32
                e[op, lane, b] = tap(32 * op + 16 * hh + b - (i + 1))
            if walk:            # output row i lies six rows above tile row i: previous rows i+26 .. 31, these rows i-6 .. i
                e[2, lane, b] = tap(slot_row(hh, b) - i - 26)
                e[3, lane, b] = tap(slot_row(hh, b) - i + 6)
            else:               # output row i reads tile rows i .. i+6 of a 38-row tile; [3] holds rows 32 ..
                e[2, lane, b] = tap(slot_row(hh, b) - i)
                e[3, lane, b] = tap(32 + slot_row(hh, b) - i)
    return e


def test_tables_follow_the_slot_mapping():
    for walk in (0, 1):
        assert np.array_equal(device_tables(walk), expected(walk)), "walk = %d" % walk


def test_walk_tables_are_the_banded_filter():
    """as matrices: [previous | these] rows times the two vertical operands = the seven taps on rows o-6 .. o of the stacked H,
    every output row with all seven taps (the presets rely on their sum, 257)"""
    t = device_tables(1).astype(np.int64)
    V = np.zeros((32, 64), np.int64)   # output row x (previous tile rows 0..31, this step's 0..31)
    for lane in range(64):
        for b in range(16):
            V[lane & 31, slot_row(lane >> 5, b)] += t[2, lane, b]
            V[lane & 31, 32 + slot_row(lane >> 5, b)] += t[3, lane, b]
    ref = np.zeros_like(V)
    for o in range(32):
        for k in range(7):
            ref[o, 32 + o - 6 + k] = W[k]
    assert np.array_equal(V, ref)
    assert (V.sum(axis=1) == 257).all()


def test_horizontal_tables_are_the_banded_filter():
    """operands [0] and [1] as one matrix: 64 strip columns (the tile starts 4 px left of the outputs) times 32 output
    columns; output column n carries the seven taps on strip columns n+1 .. n+7 and nothing else -- for both kernels"""
    for walk in (0, 1):
        t = device_tables(walk).astype(np.int64)
        K = np.zeros((64, 32), np.int64)   # strip column x output column
        for op in (0, 1):
            for lane in range(64):
                for b in range(16):
                    K[32 * op + 16 * (lane >> 5) + b, lane & 31] += t[op, lane, b]
        ref = np.zeros_like(K)
        for n in range(32):
            for k in range(7):
                ref[n + 4 - 3 + k, n] = W[k]   # centred on strip column n + 4
        assert np.array_equal(K, ref), "walk = %d" % walk
