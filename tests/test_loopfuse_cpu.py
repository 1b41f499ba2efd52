"""SearchAndFuse on the host, no GPU: the ABI of include/orbslamm_loopfuse.h, the drop-in header against the mocks, the
refusals that need no GPU, the restatement (tools/loopfuse_ref.hpp) against the oracle's window walk and against a float64
recount that shares no code with it, `1.0/z` against the float division over a sweep of float bit patterns, the serial map
model on two hand-made scenes, and the parallel rule (device hits + survivor set + host re-score) against the serial loop."""
import ctypes as C
import os

import numpy as np
import pytest

import dropin
import fuse_cases as fc
import loopfuse_cases as lc
import ref_shim
from orbslamm_amd import local_mapping as lm
from orbslamm_amd import loop_closing as lo
from orbslamm_amd._lib import KP_DTYPE, ORBX_E_INVALID, ORBX_E_UNSUPPORTED
from ref_shim import p as _p

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_loopfuse_block():
    """include/orbslamm_loopfuse.h declares the two orbc_ entries and nothing else, include/orbslamm_hip.h brings it along, the library and
    the package export the entries, and the ceilings are the mirror's and at least what the issue asks"""
    from orbslamm_amd import _lib
    src = open(os.path.join(ROOT, "include", "orbslamm_loopfuse.h")).read()
    assert "ORBC_MAX_TARGETS %d" % lo.MAX_TARGETS in src and "ORBC_MAX_PAIRS (1 << 26)" in src
    assert lo.MAX_TARGETS >= 4096 and lo.MAX_PAIRS == 1 << 26
    declared = ref_shim.declared("orbslamm_loopfuse.h", "orbc_")
    assert len(declared) == 2
    assert declared == ref_shim.declared("orbslamm_loopfuse.h")          # nothing of the other blocks is declared here
    assert '#include "orbslamm_loopfuse.h"' in open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    import orbslamm_amd
    assert orbslamm_amd.search_and_fuse is lo.search_and_fuse
    assert lo.HIT_DTYPE.itemsize == 16 and lo.HIT_DTYPE.names == ("target", "point", "best_idx", "best_dist")
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "loopfuse_ref.hpp"))
    for name in ("orbc_kernels.hip", "orbc_host.inc"):
        assert "loopfuse_ref" not in open(os.path.join(ROOT, "orbslamm_amd", "csrc", name)).read()


def test_dropin_header_compiles_against_the_mocks():
    """include/LoopClosing_hip.hpp instantiated on the mocks of tests/cpp/mock_loopfuse.hpp (the GPU test runs it)"""
    dropin.syntax_only("loopfuse_dropin_gpu")
    hdr = open(os.path.join(ROOT, "include", "LoopClosing_hip.hpp")).read()
    for member in ("SearchAndFuseT", "Run(", "rescored"):
        assert member in hdr, member


def test_refusals_that_need_no_gpu():
    """the argument checks come before the handle's: with a NULL handle every refusal still names its own reason"""
    from orbslamm_amd import _lib
    L = _lib.lib()
    case = lc.family_case("general", 0)
    T, P = len(case["targets"]), len(case["points"])
    recs = np.array([t["rec"] for t in case["targets"]], dtype=lm.FUSE_TARGET_DTYPE)
    keys = lm._ptr_array([t["keys"] for t in case["targets"]])
    desc = lm._ptr_array([t["desc"] for t in case["targets"]])
    n = np.array([len(t["keys"]) for t in case["targets"]], np.int32)
    breaks = lm.level_breaks(fc.LOG_SF, fc.NLEVELS)
    hits = np.zeros(16, lo.HIT_DTYPE)
    nh = C.c_int(-7)

    def call(h=None, recs=recs, T=T, pts=case["points"], P=P, max_dist=50, sf=case["sf"], nlevels=fc.NLEVELS, br=breaks, hits=hits, cap=16, nh=nh,
             keys=keys, n=n):
        rc = L.orbc_search_and_fuse(h, _p(recs), keys, desc, _p(n), T, _p(pts), P, C.c_float(4.0), max_dist, _p(sf), nlevels, _p(br), _p(hits), cap,
                                    C.byref(nh) if nh is not None else None, None, None)
        return rc, L.orbx_last_error().decode()

    assert call()[0] == ORBX_E_INVALID and "null handle" in call()[1] and nh.value == 0
    assert call(nh=None)[0] == ORBX_E_INVALID
    rc, msg = call(T=lo.MAX_TARGETS + 1)
    assert rc == ORBX_E_UNSUPPORTED and "targets" in msg
    rc, msg = call(T=lo.MAX_TARGETS, P=lo.MAX_PAIRS // lo.MAX_TARGETS + 1)
    assert rc == ORBX_E_UNSUPPORTED and "pairs" in msg
    for bad in (-1, 257):
        rc, msg = call(max_dist=bad)
        assert rc == ORBX_E_INVALID and "max_dist" in msg
    for nl in (0, 17):
        assert call(nlevels=nl)[0] == ORBX_E_INVALID
    for b in (breaks[::-1].copy(), np.r_[breaks[:3], breaks[2], breaks[4:]].astype(f32), np.r_[breaks[:3], np.nan, breaks[4:]].astype(f32)):
        rc, msg = call(br=b)
        assert rc == ORBX_E_INVALID and "break" in msg
    assert call(recs=None)[0] == ORBX_E_INVALID and call(pts=None)[0] == ORBX_E_INVALID and call(sf=None)[0] == ORBX_E_INVALID
    assert call(br=None)[0] == ORBX_E_INVALID and call(T=-1)[0] == ORBX_E_INVALID and call(P=-1)[0] == ORBX_E_INVALID
    assert call(cap=-1)[0] == ORBX_E_INVALID and call(hits=None, cap=4)[0] == ORBX_E_INVALID and call(keys=None)[0] == ORBX_E_INVALID
    big = n.copy()
    big[1] = 65536
    rc, msg = call(n=big)
    assert rc == ORBX_E_INVALID and "65535" in msg
    bad = recs.copy()
    bad["grid"]["cols"][0] = 0
    rc, msg = call(recs=bad)
    assert rc == ORBX_E_INVALID and "grid" in msg
    # the frames entry: the same checks, and a null frame list
    rc = L.orbc_search_and_fuse_frames(None, _p(recs), None, T, _p(case["points"]), P, C.c_float(4.0), 50, _p(case["sf"]), fc.NLEVELS, _p(breaks), _p(hits),
                                       16, C.byref(nh), None, None)
    assert rc == ORBX_E_INVALID and "frame" in L.orbx_last_error().decode()
    rc = L.orbc_search_and_fuse_frames(None, _p(recs), None, lo.MAX_TARGETS + 1, _p(case["points"]), P, C.c_float(4.0), 50, _p(case["sf"]), fc.NLEVELS,
                                       _p(breaks), _p(hits), 16, C.byref(nh), None, None)
    assert rc == ORBX_E_UNSUPPORTED


def test_invz_as_written_equals_the_float_division():
    """:1021 writes 1.0/z rounded to float; the device divides in float.  Equal as bits over every 97th float pattern of the
    positive and the negative range (44 million of each, zeros, subnormals, infinities and NaNs included) and over every
    pattern of [0.25, 64], where depths live"""
    L = lc.ref_lib()
    first = np.zeros(1, np.uint32)
    for lo_, hi_, step in ((0x00000000, 0x7FFFFFFF, 97), (0x80000000, 0xFFFFFFFF, 97), (0x3E800000, 0x42800000, 1), (0x00000000, 0x00010000, 1),
                           (0x7F7F0000, 0x7F800010, 1)):
        bad = L.loopref_invz_sweep(lo_, hi_, step, _p(first))
        assert bad == 0, (hex(lo_), hex(hi_), bad, hex(int(first[0])))


@pytest.mark.parametrize("name", sorted(lc.FAMILIES))
def test_restatement_against_float64_and_the_oracle(oracle, name):
    """outside the measured bands every gate decision and level of the restatement is the float64 recount's, at most 2 % of a
    case's pairs lie inside a band (the measured shares are far below), the restatement's own grid and window walk give what
    the oracle's window_best gives without chi-square, and the family shows its status code and clears its floor on hits"""
    codes, hits_total, passing, pairs = np.zeros(7, np.int64), 0, 0, 0
    for seed in lc.SEEDS:
        case = lc.family_case(name, seed)
        outside, share, total = lc.check64(case)
        print(name, seed, "pairs", total, "outside the bands", outside, "share inside", share)
        assert outside == 0 and share <= lc.BAND_SHARE_CAP, (name, seed, outside, share)
        assert share <= 2 * lc.MEASURED_SHARE.get(name, 0.0) + 1e-12, (name, seed, share)
        hits, start, status = lc.reference(oracle, case)
        own = lc.reference_own(case)
        assert hits.tobytes() == own[0].tobytes() and start.tobytes() == own[1].tobytes() and status.tobytes() == own[2].tobytes(), (name, seed)
        assert start[-1] == len(hits) and np.all(np.diff(start) >= 0)
        order = hits["target"].astype(np.int64) * len(case["points"]) + hits["point"]
        assert np.all(np.diff(order) > 0)                                  # target-major, points ascending
        codes += np.bincount(status.reshape(-1), minlength=7)
        hits_total += len(hits)
        pairs += total
    print(name, dict(zip(lm.FUSE_STATUS_NAMES, codes.tolist())), "hits", hits_total)
    assert hits_total >= lc.HIT_FLOOR[name], (name, hits_total)
    if name in lc.FAMILY_CODES:
        assert codes[lc.FAMILY_CODES[name]] > 0, (name, lm.FUSE_STATUS_NAMES[lc.FAMILY_CODES[name]])
    if name == "sparse_survivors":
        assert (codes[lm.FUSE_ST_NO_CANDIDATE] + codes[lm.FUSE_ST_FOUND]) / pairs < lc.SPARSE_SHARE_CAP
    if name == "scaled_sim3":
        case = lc.family_case(name, 0)
        assert set(case["scales"]) == {0.5, 2.0, 1.0}
        for t in case["targets"]:                                          # the caller's decomposition took the scale out
            assert abs(np.linalg.det(t["rec"]["Rcw"].astype(np.float64)) - 1) < 1e-5


def test_no_chi_square_in_this_fuse(oracle):
    """the restatement's window keeps a candidate the chi-square test of Fuse(pKF, vpMapPoints) would drop: the two references
    differ on the same scene, and ours is the one without the test"""
    seed = 1000 * (sorted(fc.FAMILIES).index("chi2_edge") + 1)             # fuse_cases.family_case("chi2_edge", 0)'s scene
    case = lc.make_dense(seed, th=fc.TH, **fc.FAMILIES["chi2_edge"])
    mine = lc.reference_own(case, max_dist=256)[0]
    with_chi2 = fc.make_case(seed, **fc.FAMILIES["chi2_edge"])
    T, P = len(case["targets"]), len(case["points"])
    kept = 0
    for k in range(T):
        theirs = fc.ref_target(with_chi2, k, np.arange(P))
        found = theirs["status"] == lm.FUSE_ST_FOUND
        ours = np.zeros(P, bool)
        ours[mine["point"][mine["target"] == k]] = True
        assert not (found & ~ours).any()                                   # without the test nothing is lost
        kept += int((ours & ~found).sum())
    assert kept >= 50, kept


# ------------------------------------------------------------------------------------------------ the serial map model
def _flip(d, bits_):
    d = d.copy()
    for b in bits_:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _keys(xy, octave):
    k = np.zeros(len(xy), dtype=KP_DTYPE)
    for i, (x, y) in enumerate(xy):
        k["x"][i], k["y"][i] = x, y
    k["octave"], k["size"], k["response"], k["class_id"] = octave, 31.0, 50.0, -1
    return k


def _rec(O):
    return lm.fuse_target(np.eye(3), -np.asarray(O, float), O, fc.K_A, (0.0, fc.W, 0.0, fc.H), fc.grid_tuple(), keys=np.zeros(0, KP_DTYPE),
                          desc=np.zeros((0, 32), np.uint8))["rec"]


def _point(pos, d):
    maxd = float(np.linalg.norm(pos) * 1.2 ** 2.5)                        # level 3 from about that distance, well inside its step
    return lm.fuse_points([pos], [np.asarray(pos) / np.linalg.norm(pos)], maxd / float(fc.SF[7]), maxd, [d])[0]


def _proj(rec, point):
    tmp = dict(targets=[dict(rec=rec)], points=np.array([point], lm.FUSE_POINT_DTYPE), th=lc.TH, sf=fc.SF, log_sf=fc.LOG_SF)
    r = lc.ref_project(tmp, 0)[0][0]
    assert r["status"] == lm.FUSE_ST_NO_CANDIDATE and r["level"] == 3, r
    return float(r["u"]), float(r["v"])


def test_serial_model_scene_1_a_replace_changes_what_the_next_target_picks():
    """Loop point A (observed by the loop keyframes L1, L2) and three corrected keyframes T0, T1, T2; bystanders X, Y of the
    current side.
      T0: A lands on the feature that holds B (observed by T0, X, Y): vpReplacePoints[0] = B, and after the loop B->Replace(A).
          A survives with the observations (L1, L2, T0, X, Y), and ComputeDistinctiveDescriptors moves its descriptor from dL
          to d0 (T0's, X's and Y's descriptors are 2 bits apart, the loop side's 40 away).
      T1: A's window holds g1 (5 bits from dL, 45 from d0) and g2 (5 bits from d0, 45 from dL): with its NEW descriptor A takes
          g2; the old one would have taken g1.
      T2: nothing of A's lands on a feature.
    The rule without the re-score takes g1 and ends with another map."""
    rng = np.random.default_rng(43)
    dL = rng.integers(0, 256, 32, dtype=np.uint8)
    d0 = _flip(dL, range(0, 40))
    dX, dY = _flip(d0, (100, 101)), _flip(d0, (102, 103))
    g1, g2 = _flip(dL, range(200, 205)), _flip(d0, range(210, 215))
    far = rng.integers(0, 256, 32, dtype=np.uint8)
    centre = {"T0": (0.15, 0.0, 0.0), "T1": (-0.2, 0.1, 0.0), "T2": (0.0, -0.25, 0.1)}
    recs = {k: _rec(v) for k, v in centre.items()}
    pA = _point((0.0, 0.0, 5.0), dL)
    aT0, aT1 = _proj(recs["T0"], pA), _proj(recs["T1"], pA)
    t1_keys, t1_desc = _keys([(aT1[0] - 1.0, aT1[1]), (aT1[0] + 1.0, aT1[1])], 3), np.stack([g1, g2])
    # the scene cannot pass by accident: at T1 the old descriptor and the new one pick different features
    t1 = dict(targets=[dict(rec=recs["T1"], keys=t1_keys, desc=t1_desc)], points=np.array([pA, pA], lm.FUSE_POINT_DTYPE), th=lc.TH, sf=fc.SF,
              log_sf=fc.LOG_SF)
    t1["points"]["desc"][1] = d0
    old, new = lc.ref_target(t1, 0)
    assert (old["status"], new["status"]) == (lm.FUSE_ST_FOUND, lm.FUSE_ST_FOUND)
    assert (int(old["best_idx"]), int(old["best_dist"])) == (0, 5) and (int(new["best_idx"]), int(new["best_dist"])) == (1, 5)
    assert old["best_idx"] != new["best_idx"]

    def build():
        m = lc.Model()
        g = fc.grid_tuple()
        T0 = m.keyframe(g, _keys([aT0, (50.0, 50.0)], 3), np.stack([d0, far]))
        T1 = m.keyframe(g, t1_keys, t1_desc)
        T2 = m.keyframe(g, _keys([(600.0, 40.0)], 3), np.stack([far]))
        X, Y = m.keyframe(g, _keys([(100.0, 100.0)], 3), np.stack([dX])), m.keyframe(g, _keys([(100.0, 100.0)], 3), np.stack([dY]))
        L1, L2 = m.keyframe(g, _keys([(100.0, 100.0)], 3), np.stack([dL])), m.keyframe(g, _keys([(100.0, 100.0)], 3), np.stack([_flip(dL, (7,))]))
        A, B = m.point(pA), m.point(_point((0.001, 0.0, 5.0), d0))
        for mp, kf in ((A, L1), (A, L2), (B, T0), (B, X), (B, Y)):
            m.observe(mp, kf, 0)
        return m, (T0, T1, T2, X, Y, L1, L2), (A, B)

    results = {}
    for mode in (0, 1, 2):
        m, (T0, T1, T2, X, Y, L1, L2), (A, B) = build()
        fused, events, rescored = m.search_and_fuse(mode, [T0, T1, T2], [recs["T0"], recs["T1"], recs["T2"]], [A])
        results[mode] = (fused, events, m.state(), rescored)
        if mode == 0:
            assert fused == 2 and events == [(1, B, A, 0), (2, A, T1, 1)], events
            assert m.slots(T0) == [A, -1] and m.slots(T1) == [-1, A] and m.slots(X) == [A] and m.slots(Y) == [A]
            badA, _, descA, obsA = m.map_point(A)
            badB, repB, _, obsB = m.map_point(B)
            assert not badA and descA == d0.tobytes()
            assert obsA == [(L1, 0), (L2, 0), (T0, 0), (X, 0), (Y, 0), (T1, 1)]
            assert badB and repB == A and obsB == []
        m.close()
    assert results[1][:3] == results[0][:3] and results[1][3] == 2        # A at T1 and at T2, scored again
    assert results[2][1] == [(1, B, A, 0), (2, A, T1, 0)] and results[2][:3] != results[0][:3]


def test_serial_model_scene_2_two_loop_points_on_one_feature():
    """Two loop points A1, A2 whose projections share one free feature f of T0.  A1 (first in the list) takes it
    (AddObservation); A2 then finds A1 there: vpReplacePoints[1] = A1, and after the loop A1->Replace(A2): A1, a loop point
    itself, turns bad, and A2 holds T0's feature.  At T1 the bad A1 is skipped by the isBad() read and A2 is searched (as a
    survivor: on the host) and added."""
    rng = np.random.default_rng(44)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    recs = [_rec((0.15, 0.0, 0.0)), _rec((-0.2, 0.1, 0.0))]
    p1, p2 = _point((0.0, 0.0, 5.0), _flip(d, (1, 2))), _point((0.002, 0.0, 5.0), _flip(d, (3, 4, 5)))
    f0, f1 = _proj(recs[0], p1), _proj(recs[1], p1)
    results = {}
    for mode in (0, 1):
        m = lc.Model()
        g = fc.grid_tuple()
        T0, T1 = m.keyframe(g, _keys([f0], 3), np.stack([d])), m.keyframe(g, _keys([f1, (30.0, 30.0)], 3), np.stack([_flip(d, (9,)), d]))
        L1 = m.keyframe(g, _keys([(100.0, 100.0), (200.0, 200.0)], 3), np.stack([p1["desc"], p2["desc"]]))
        A1, A2 = m.point(p1), m.point(p2)
        m.observe(A1, L1, 0)
        m.observe(A2, L1, 1)
        fused, events, rescored = m.search_and_fuse(mode, [T0, T1], recs, [A1, A2])
        assert fused == 3 and events == [(2, A1, T0, 0), (1, A1, A2, 0), (2, A2, T1, 0)], events
        assert m.slots(T0) == [A2] and m.slots(T1) == [A2, -1] and m.slots(L1) == [-1, A2]      # (A2 was in L1 already: A1's slot there is erased)
        bad1, rep1, _, obs1 = m.map_point(A1)
        assert bad1 and rep1 == A2 and obs1 == [] and m.map_point(A2)[3] == [(L1, 1), (T0, 0), (T1, 0)]
        results[mode] = (fused, events, m.state())
        assert rescored == (1 if mode else 0)
        m.close()
    assert results[0] == results[1]


@pytest.mark.parametrize("name", sorted(lc.FAMILIES))
def test_parallel_rule_equals_the_serial_loop(name):
    """device hits + survivor set + host re-score (tools/loopfuse_ref.hpp, searchAndFuseByRule) leave the map, the counts and
    the Replace / AddObservation sequence of the serial loop, on a map made from every family and seed; over the seeds the
    rule without the re-score goes wrong somewhere in the scene built for it"""
    replaced = rescored_total = 0
    for seed in lc.SEEDS:
        scene = lc.map_scene(seed, case=lc.family_case(name, seed))
        nt = len(scene["case"]["targets"])
        recs = np.array([t["rec"] for t in scene["case"]["targets"]], dtype=lm.FUSE_TARGET_DTYPE)
        out = []
        for mode in (0, 1):
            m = lc.load_model(scene)
            fused, events, rescored = m.search_and_fuse(mode, np.arange(nt), recs, scene["loop"])
            out.append((fused, events, m.state()))
            m.close()
        assert out[0] == out[1], (name, seed)
        replaced += sum(e[0] == 1 for e in out[0][1])
        rescored_total += rescored
    print(name, "Replace calls", replaced, "pairs re-scored", rescored_total)
    assert replaced >= 20 and rescored_total > 0, (name, replaced, rescored_total)


def test_the_rule_without_the_rescore_is_wrong_on_the_dropin_scene():
    scene = lc.map_scene(0)
    nt = len(scene["case"]["targets"])
    recs = np.array([t["rec"] for t in scene["case"]["targets"]], dtype=lm.FUSE_TARGET_DTYPE)
    out = []
    for mode in (0, 1, 2):
        m = lc.load_model(scene)
        fused, events, rescored = m.search_and_fuse(mode, np.arange(nt), recs, scene["loop"])
        out.append((fused, events, m.state()))
        pairs = nt * len(scene["loop"])
        print("mode", mode, "fused", fused, "events", len(events), "re-scored", rescored, "of", pairs, "pairs: share %.4f" % (rescored / pairs))
        m.close()
    assert out[0] == out[1] and out[2] != out[0]
    assert sum(e[0] == 1 for e in out[0][1]) >= 20 and sum(e[0] == 2 for e in out[0][1]) >= 50
