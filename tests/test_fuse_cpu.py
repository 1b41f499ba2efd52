"""SearchInNeighbors on the host, no GPU: orbl_level_breaks against PredictScale's direct formula over every float of
[2^-8, 2^12], the restatement (tools/fuse_ref.hpp) against a float64 recount that shares no code with it, the
restatement's own window walk against the oracle's, and the serial map model on a hand-made three-target scene in which a
Replace changes a surviving point's descriptor and with it the feature it picks at the next target."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fuse_cases as fc
import ref_shim
from orbslamm_amd import local_mapping as lm
from orbslamm_amd._lib import KP_DTYPE, ORBX_E_INVALID, OrbError
from ref_shim import p as _p

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_fuse_block():
    """include/orbslamm_fuse.h declares the three orbl_ entries with the status codes of the mirror, include/orbslamm_hip.h
    brings it along, and the library and the package export the entries"""
    from orbslamm_amd import _lib
    src = open(os.path.join(ROOT, "include", "orbslamm_fuse.h")).read()
    assert "ORBL_FUSE_MAX_TARGETS 128" in src and "ORBL_FUSE_MAX_JOBS (1 << 22)" in src
    assert lm.FUSE_MAX_TARGETS == 128 and lm.FUSE_MAX_JOBS == 1 << 22 >= 1048576
    for code, name in enumerate(lm.FUSE_STATUS_NAMES):
        assert re.search(r"#define ORBL_FUSE_ST_%s %d\b" % (name.upper(), code), src), name
    declared = ref_shim.declared("orbslamm_fuse.h", "orbl_")
    assert len(declared) == 3
    assert '#include "orbslamm_fuse.h"' in open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    import orbslamm_amd
    assert orbslamm_amd.fuse_batch is lm.fuse_batch and orbslamm_amd.level_breaks is lm.level_breaks
    ref_shim.assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "fuse_ref.hpp"))


def bits(x):
    return int(np.array([x], f32).view(np.uint32)[0])


def sweep(lsf, nlevels, breaks, lo, hi):
    first = np.zeros(1, np.uint32)
    bad = fc.ref_lib().fuseref_level_sweep(C.c_float(lsf), nlevels, _p(breaks), lo, hi, _p(first))
    return bad, int(first[0])


def test_level_breaks_equal_the_direct_formula_over_every_float():
    """1.2 / 8 levels: the break table + count against ceil(log(ratio)/logScaleFactor) for all 167 772 160 floats of [2^-8, 2^12]"""
    breaks = lm.level_breaks(fc.LOG_SF, fc.NLEVELS)
    assert breaks.shape == (fc.NLEVELS + 1,) and np.all(np.diff(breaks) > 0)
    want = np.array([0.833333254, 1.0, 1.20000005, 1.44000006], f32)
    assert breaks[:4].tobytes() == want.tobytes(), breaks[:4]
    lo, hi = bits(2.0 ** -8), bits(2.0 ** 12)
    assert hi - lo == 167772160
    bad, first = sweep(fc.LOG_SF, fc.NLEVELS, breaks, lo, hi)
    assert bad == 0, (bad, hex(first))


@pytest.mark.parametrize("factor,nlevels", [(1.1, 8), (1.5, 8), (1.2, 16), (1.2, 1)])
def test_level_breaks_around_the_breaks_of_other_factors(factor, nlevels):
    lsf = f32(np.log(f32(factor)))
    breaks = lm.level_breaks(lsf, nlevels)
    for b in breaks:
        bad, first = sweep(lsf, nlevels, breaks, bits(b) - (1 << 16), bits(b) + (1 << 16))
        assert bad == 0, (factor, float(b), hex(first))
    # the ends of the float range, zero, and what is not a ratio
    for lo, hi in ((0, 1 << 12), (0x7F7FF000, 0x7F800001), (0x7FC00000, 0x7FC00000), (0x80000000, 0x80001000), (0xBF800000, 0xBF800000)):
        assert sweep(lsf, nlevels, breaks, lo, hi)[0] == 0, (hex(lo), hex(hi))


def test_level_breaks_with_the_trees_own_predict_scale():
    """a tree whose log resolves to the double overload passes its own function"""
    lsf = float(fc.LOG_SF)
    double_form = lambda ratio, l: int(np.ceil(np.log(np.float64(ratio)) / np.float64(l)))
    breaks = lm.level_breaks(lsf, fc.NLEVELS, double_form)
    for L, b in enumerate(breaks, start=-1):
        nxt = np.nextafter(b, f32(np.inf), dtype=f32)
        assert double_form(b, lsf) <= L < double_form(nxt, lsf), (L, float(b))


def test_level_breaks_refuses_bad_arguments():
    def code(*a):
        with pytest.raises(OrbError) as ei:
            lm.level_breaks(*a)
        return ei.value.code
    assert code(fc.LOG_SF, 0) == ORBX_E_INVALID
    assert code(fc.LOG_SF, 17) == ORBX_E_INVALID
    assert code(0.0, 8) == ORBX_E_INVALID
    assert code(-0.2, 8) == ORBX_E_INVALID
    assert code(float("nan"), 8) == ORBX_E_INVALID
    assert code(float("inf"), 8) == ORBX_E_INVALID
    assert code(fc.LOG_SF, 8, lambda r, l: 3) == ORBX_E_INVALID                                     # no break at all
    assert code(fc.LOG_SF, 8, lambda r, l: -int(np.ceil(np.log(r) / l))) == ORBX_E_INVALID          # descending
    L = lm.lib()
    assert L.orbl_level_breaks(C.c_float(fc.LOG_SF), 8, None, None) == ORBX_E_INVALID


@pytest.mark.parametrize("name", sorted(fc.FAMILIES))
def test_restatement_against_float64_and_the_oracle(oracle, name):
    """outside the measured bands every gate decision and level of the restatement is the float64 recount's, at most 2 % of a
    case's pairs lie inside a band, the restatement's own grid and window walk give what the oracle's window_best gives, and
    the family shows its status code and clears its floor on FOUND"""
    found, codes = 0, np.zeros(7, np.int64)
    for seed in fc.SEEDS:
        case = fc.family_case(name, seed)
        outside, share, total = fc.check64(case)
        print(name, seed, "pairs", total, "outside the bands", outside, "share inside", share)
        assert outside == 0 and share <= fc.BAND_SHARE_CAP, (name, seed, outside, share)
        want = fc.reference(oracle, case)
        js, jp = case["jobs"]
        own = np.concatenate([fc.ref_target(case, k, jp[js[k]:js[k + 1]]) for k in range(len(case["targets"]))])
        assert own.tobytes() == want.tobytes(), (name, seed, np.flatnonzero(own != want)[:5].tolist())
        codes += np.bincount(want["status"], minlength=7)
    found = int(codes[lm.FUSE_ST_FOUND])
    print(name, dict(zip(lm.FUSE_STATUS_NAMES, codes.tolist())))
    assert found >= fc.FOUND_FLOOR[name], (name, found)
    if name in fc.FAMILY_CODES:
        assert codes[fc.FAMILY_CODES[name]] > 0, (name, lm.FUSE_STATUS_NAMES[fc.FAMILY_CODES[name]])
    if name == "level_range":
        # above the last level.  Below level 0 no finite record can end: ratio <= 1/1.2 means dist3D >= 1.2 max, which the
        # distance gate (1.2f * max, the float 1.2f above 1.2) takes first; only a NaN maximum distance gets there
        case = fc.family_case(name, 0)
        res = fc.reference(oracle, case)
        assert (res["level"][res["status"] == lm.FUSE_ST_LEVEL_RANGE] == fc.NLEVELS).all()
        case["points"]["max_distance"][:7] = np.nan
        res = fc.reference(oracle, case)
        hit = res[np.isin(case["jobs"][1], np.arange(7)) & (res["status"] == lm.FUSE_ST_LEVEL_RANGE)]
        assert len(hit) and (hit["level"] == -1).all()


def test_crowded_ties_are_ties(oracle):
    """the family means what it says: windows that hold the best distance more than once, where the first in walk order wins"""
    case = fc.family_case("crowded_ties", 0)
    want = fc.reference(oracle, case)
    js, jp = case["jobs"]
    tied = 0
    for k, t in enumerate(case["targets"]):
        res = want[js[k]:js[k + 1]]
        for r, pi in zip(res, jp[js[k]:js[k + 1]]):
            if r["status"] != lm.FUSE_ST_FOUND:
                continue
            d = np.unpackbits(t["desc"] ^ case["points"]["desc"][pi], axis=1).sum(axis=1)
            near = (np.abs(t["keys"]["x"] - r["u"]) < 3.0) & (np.abs(t["keys"]["y"] - r["v"]) < 3.0) & (d == r["best_dist"])
            tied += int(near.sum() > 1)
    assert tied >= 50, tied


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


class _Model:
    def __init__(self):
        self.L = fc.ref_lib()
        self.h = self.L.fuseref_model_new(C.c_float(fc.TH), _p(fc.SF), _p(fc.INV_SIGMA2), fc.NLEVELS, C.c_float(fc.LOG_SF))
        self.n = []

    def keyframe(self, rec, keys, desc):
        rec = np.ascontiguousarray(rec, dtype=lm.FUSE_TARGET_DTYPE)
        keys, desc = np.ascontiguousarray(keys, dtype=KP_DTYPE), np.ascontiguousarray(desc, dtype=np.uint8)
        self.n.append(len(keys))
        return self.L.fuseref_add_keyframe(self.h, _p(rec), _p(keys), _p(desc), len(keys))

    def point(self, rec):
        rec = np.ascontiguousarray(rec, dtype=lm.FUSE_POINT_DTYPE)
        return self.L.fuseref_add_map_point(self.h, _p(rec))

    def observe(self, mp, kf, idx):
        self.L.fuseref_add_observation(self.h, mp, kf, idx)

    def covisibles(self, kf, ids):
        ids = np.array(ids, np.int32)
        self.L.fuseref_set_covisibles(self.h, kf, _p(ids), len(ids))

    def run(self, cur):
        targets, events = np.zeros(64, np.int32), np.zeros((64, 4), np.int32)
        nt, ne = C.c_int(0), C.c_int(0)
        self.L.fuseref_search_in_neighbors(self.h, cur, _p(targets), 64, C.byref(nt), _p(events), 64, C.byref(ne))
        return targets[:nt.value].tolist(), [tuple(e) for e in events[:ne.value].tolist()]

    def slots(self, kf):
        out = np.zeros(max(self.n[kf], 1), np.int32)
        self.L.fuseref_keyframe_slots(self.h, kf, _p(out))
        return out[:self.n[kf]].tolist()

    def map_point(self, mp):
        bad, rep = C.c_int(0), C.c_int(0)
        desc, obs = np.zeros(32, np.uint8), np.zeros((16, 2), np.int32)
        n = self.L.fuseref_map_point(self.h, mp, C.byref(bad), C.byref(rep), _p(desc), _p(obs), 16)
        return bool(bad.value), rep.value, desc, [tuple(o) for o in obs[:n].tolist()]

    def close(self):
        self.L.fuseref_model_free(self.h)


def test_serial_model_on_a_hand_made_three_target_scene():
    """Current keyframe C with the points A and D; targets T0, T1, T2; bystanders X, Y that only hold observations.
      T0: A lands on the feature of B (two observations each: B is replaced by A).  A's observations become (C, Y, T0, X), and
          ComputeDistinctiveDescriptors moves its descriptor from dC to d0 (T0's and X's descriptors are 2 bits apart, C's and
          Y's 30).
      T1: A's window holds g1 (5 bits from dC, 45 from d0) and g2 (5 bits from d0, 45 from dC): with its NEW descriptor A
          takes g2; the old one would have taken g1.  D takes the free feature h.
      T2: nothing of C's lands on a feature.  Phase 2: T2's point F lands on C's free feature c1."""
    rng = np.random.default_rng(42)
    dC = rng.integers(0, 256, 32, dtype=np.uint8)
    d0 = _flip(dC, range(0, 40))
    dX = _flip(d0, (100, 101))
    dY = _flip(dC, range(128, 158))
    g1, g2 = _flip(dC, range(200, 205)), _flip(d0, range(210, 215))
    dD, dF = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    far = rng.integers(0, 256, 32, dtype=np.uint8)
    grid, bounds, eye = fc.grid_tuple(), (0.0, fc.W, 0.0, fc.H), np.eye(3)
    rec = lambda O: lm.fuse_target(eye, -np.asarray(O, float), O, fc.K_A, bounds, grid, keys=np.zeros(0, KP_DTYPE), desc=np.zeros((0, 32), np.uint8))["rec"]
    pos = {"A": (0.0, 0.0, 5.0), "B": (0.001, 0.0, 5.0), "D": (0.8, -0.5, 6.0), "F": (-0.9, 0.6, 5.5)}
    centre = {"C": (0.0, 0.0, 0.0), "T0": (0.15, 0.0, 0.0), "T1": (-0.2, 0.1, 0.0), "T2": (0.0, -0.25, 0.1), "X": (0.5, 0.5, 0.0), "Y": (-0.5, 0.5, 0.0)}
    recs = {k: rec(v) for k, v in centre.items()}
    maxd = lambda p: float(np.linalg.norm(p) * 1.2 ** 2.5)          # level 3 from about that distance, well inside its step
    pts = {k: lm.fuse_points([v], [np.asarray(v) / np.linalg.norm(v)], maxd(v) / float(fc.SF[7]), maxd(v), [d])[0]
           for (k, v), d in zip(pos.items(), (dC, d0, dD, dF))}

    def proj(kf, point):
        tmp = dict(targets=[dict(rec=recs[kf])], points=np.array([point], lm.FUSE_POINT_DTYPE), th=fc.TH, sf=fc.SF, log_sf=fc.LOG_SF)
        r = fc.ref_project(tmp, 0, [0])[0][0]
        assert r["status"] == lm.FUSE_ST_NO_CANDIDATE and r["level"] == 3, (kf, r)
        return float(r["u"]), float(r["v"])

    aT0, aT1, dT1, fC, aC, dCc = proj("T0", pts["A"]), proj("T1", pts["A"]), proj("T1", pts["D"]), proj("C", pts["F"]), proj("C", pts["A"]), proj("C", pts["D"])
    m = _Model()
    C_ = m.keyframe(recs["C"], _keys([aC, dCc, fC], 3), np.stack([dC, dD, _flip(dF, (3, 9))]))
    T0 = m.keyframe(recs["T0"], _keys([aT0, (50.0, 50.0)], 3), np.stack([d0, far]))
    T1 = m.keyframe(recs["T1"], _keys([(aT1[0] - 1.0, aT1[1]), (aT1[0] + 1.0, aT1[1]), dT1], 3), np.stack([g1, g2, _flip(dD, (1, 2, 3))]))
    T2 = m.keyframe(recs["T2"], _keys([(600.0, 40.0)], 3), np.stack([_flip(dF, (7,))]))
    X = m.keyframe(recs["X"], _keys([(100.0, 100.0)], 3), np.stack([dX]))
    Y = m.keyframe(recs["Y"], _keys([(100.0, 100.0)], 3), np.stack([dY]))
    A, B, D, F = (m.point(pts[k]) for k in "ABDF")
    for mp, kf, idx in ((A, C_, 0), (A, Y, 0), (B, T0, 0), (B, X, 0), (D, C_, 1), (F, T2, 0)):
        m.observe(mp, kf, idx)
    m.covisibles(C_, [T0, T1, T2])
    # the scene cannot pass by accident: at T1 the old descriptor and the new one pick different features
    t1 = dict(targets=[dict(rec=recs["T1"], keys=_keys([(aT1[0] - 1.0, aT1[1]), (aT1[0] + 1.0, aT1[1]), dT1], 3),
                            desc=np.stack([g1, g2, _flip(dD, (1, 2, 3))]))],
              points=np.array([pts["A"], pts["A"]], lm.FUSE_POINT_DTYPE), th=fc.TH, sf=fc.SF, inv_sigma2=fc.INV_SIGMA2, log_sf=fc.LOG_SF)
    t1["points"]["desc"][1] = d0
    old, new = fc.ref_target(t1, 0, [0, 1])
    assert (old["status"], new["status"]) == (lm.FUSE_ST_FOUND, lm.FUSE_ST_FOUND)
    assert (int(old["best_idx"]), int(old["best_dist"])) == (0, 5) and (int(new["best_idx"]), int(new["best_dist"])) == (1, 5)
    assert old["best_idx"] != new["best_idx"]

    targets, events = m.run(C_)
    assert targets == [T0, T1, T2]
    assert events == [(1, B, A, T0), (2, A, T1, 1), (2, D, T1, 2), (2, F, C_, 2)], events
    assert m.slots(T0) == [A, -1] and m.slots(T1) == [-1, A, D] and m.slots(C_) == [A, D, F] and m.slots(X) == [A]
    badA, _, descA, obsA = m.map_point(A)
    badB, repB, _, obsB = m.map_point(B)
    assert not badA and descA.tobytes() == d0.tobytes()
    assert obsA == [(C_, 0), (Y, 0), (T0, 0), (X, 0), (T1, 1)]
    assert badB and repB == A and obsB == []
    assert m.map_point(F)[3] == [(T2, 0), (C_, 2)]
    m.close()
