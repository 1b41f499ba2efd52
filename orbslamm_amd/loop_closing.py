"""LoopClosing::SearchAndFuse (src/LoopClosing.cc:601-627) and MultiMapper::SearchAndFuse (src/MultiMapper.cc:668-694) on
the device (orbc_search_and_fuse*, include/orbslamm_loopfuse.h): one call runs the searches of
ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of every point against every corrected keyframe and returns the
hits (best_idx >= 0 and best_dist <= max_dist) as an ordered list.

    tg = [fuse_target(Rcw, tcw, Ow, K, (0, 640, 0, 480), grid, keys=mvKeysUn, desc=descriptors), ...]   # or frame=F
    hits, hit_start, status = search_and_fuse(matcher, tg, fuse_points(pos, normal, min_d, max_d, desc), scale_factors,
                                              level_breaks(np.log(np.float32(1.2)), 8), th=4.0)

Rcw, tcw, Ow are the caller's decomposition of Scw (decompose_sim3).  Replace / AddObservation stay the caller's
(include/LoopClosing_hip.hpp replays them in the reference's order)."""
import ctypes as C

import numpy as np

from ._lib import ORBX_E_CAPACITY, OrbError, check, lib, ptr
from .local_mapping import FUSE_POINT_DTYPE, _fuse_levels, _fuse_targets

MAX_TARGETS = 8192
MAX_PAIRS = 1 << 26
TH_LOW = 50
HIT_DTYPE = np.dtype([("target", "<i4"), ("point", "<i4"), ("best_idx", "<i4"), ("best_dist", "<i4")])
assert HIT_DTYPE.itemsize == 16


def decompose_sim3(Scw):
    """ORBmatcher.cc:987-992 in OpenCV's forms: (Rcw, tcw, Ow) as float32 from a 4x4 (or 3x4) float32 Scw"""
    S = np.asarray(Scw, dtype=np.float32)
    sR = S[:3, :3]
    scw = np.float32(np.sqrt(np.sum(sR[0].astype(np.float64) ** 2)))            # Mat::dot is a double sum; sqrt of a double, then float
    inv = np.float64(1.0) / np.float64(scw)
    R = (sR.astype(np.float64) * inv).astype(np.float32)                          # sRcw / scw: convertTo with a double scale
    t = (S[:3, 3].astype(np.float64) * inv).astype(np.float32)
    Ow = np.array([-(np.float64(R[0, i]) * np.float64(t[0]) + np.float64(R[1, i]) * np.float64(t[1]) + np.float64(R[2, i]) * np.float64(t[2]))
                   for i in range(3)]).astype(np.float32)                         # -Rcw.t()*tcw: the generic gemm, a double sum in k order
    return R, t, Ow


def search_and_fuse(matcher, targets, points, scale_factors, breaks, th=4.0, max_dist=TH_LOW, capacity=None, want_status=False):
    """Every point of the pool against every target in one call.  targets: local_mapping.fuse_target(...) dicts, all with host
    arrays or all with frames; points: a FUSE_POINT_DTYPE pool.  Returns (hits, hit_start, status): hits a HIT_DTYPE array,
    target-major with points ascending; hit_start (n_targets + 1) each target's stretch; status the (n_targets, n_points)
    table of FUSE_ST_* codes (None unless want_status).  capacity None: room for every pair's hit is not reserved, the call is
    repeated once with the needed count when the first guess was short.  A capacity given and too small raises OrbError
    (ORBX_E_CAPACITY, e.needed = the count)."""
    L = lib()
    T = len(targets)
    pts = np.ascontiguousarray(points, dtype=FUSE_POINT_DTYPE)
    P = pts.shape[0]
    sf, br, _ = _fuse_levels(scale_factors, breaks)
    frames, head = _fuse_targets(matcher, targets)
    hit_start = np.zeros(T + 1, dtype=np.int32)
    status = np.zeros((T, P), dtype=np.uint8) if want_status else None
    n_hits = C.c_int(0)
    fn = L.orbc_search_and_fuse_frames if frames else L.orbc_search_and_fuse

    def call(cap):
        hits = np.empty((max(cap, 1), 4), dtype=np.int32)        # (plain words: numpy fills and copies record arrays element by element)
        rc = fn(*head, ptr(pts), P, C.c_float(th), int(max_dist), ptr(sf), sf.shape[0], ptr(br), ptr(hits), int(cap), C.byref(n_hits), ptr(hit_start),
                ptr(status))
        return rc, hits

    guess = int(capacity) if capacity is not None else min(T * P, max(4096, 2 * P))
    rc, hits = call(guess)
    if rc == ORBX_E_CAPACITY and capacity is None:
        rc, hits = call(n_hits.value)
    if rc == ORBX_E_CAPACITY:
        e = OrbError(rc, L.orbx_last_error().decode(errors="replace"))
        e.needed = n_hits.value
        raise e
    check(rc)
    return hits[:n_hits.value].copy().view(HIT_DTYPE).reshape(-1), hit_start, status
