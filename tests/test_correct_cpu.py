"""The correction of LoopClosing::CorrectLoop / MultiMapper::UpdatePosesAndAdd without a GPU (orbe_*): the
restatement (tools/correct_ref.hpp) against an independent model -- Python floats for binary64 and numpy float32 scalars, one
operation at a time, the quaternion formulas written out again, ownership and the centres as RULES where the restatement runs the
sequence -- by bytes over every scene family and seeds 1..10; every family forcing its branch; the record layouts against the
mirror; the refusals that need no GPU, the outputs untouched; the drop-in compiled against its mocks.

What the issue's mixed-rank family was to show cannot be shown, and the opposite is asserted instead: a listed keyframe that
observes a point holds it, so its rank is never below the owner's (header, rule 5's consequence).  The rule's reading of the
centres and the all-old reading therefore give the SAME bytes in every scene (asserted), the all-new reading different ones
(asserted), and the restatement's counter of re-posed observers stays zero (asserted)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import correct_cases as cs
import dropin
from orbslamm_amd import _lib
from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_OK, lib, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the model.  A Sim3 is (q = [x, y, z, w], t, s) of Python floats
def quat_of_matrix(R):
    """Eigen's Quaterniond(Matrix3d)"""
    q = [0.0] * 4
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
        return q
    i = 1 if R[1][1] > R[0][0] else 0
    if R[2][2] > R[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3], q[j], q[k] = (R[k][j] - R[j][k]) * t, (R[j][i] + R[i][j]) * t, (R[k][i] + R[i][k]) * t
    return q


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def rotate(q, v):
    """QuaternionBase::_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv"""
    uv = cross(q, v)
    uv = [u + u for u in uv]
    c = cross(q, uv)
    return [(v[i] + q[3] * uv[i]) + c[i] for i in range(3)]


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def to_matrix(q):
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def sim3_of_pose(T):
    """T: 3 x 4 float32"""
    return quat_of_matrix([[float(T[i, j]) for j in range(3)] for i in range(3)]), [float(T[i, 3]) for i in range(3)], 1.0


def sim3_map(S, pt):
    q, t, s = S
    r = rotate(q, pt)
    return [s * r[i] + t[i] for i in range(3)]


def sim3_mul(A, B):
    r = rotate(A[0], B[1])
    return quat_mul(A[0], B[0]), [A[2] * r[i] + A[1][i] for i in range(3)], A[2] * B[2]


def sim3_inverse(S):
    q, t, s = S
    c = [-q[0], -q[1], -q[2], q[3]]
    f = -1.0 / s
    return c, rotate(c, [f * t[0], f * t[1], f * t[2]]), 1.0 / s


def gemm(terms, alpha):
    """gemm's small-matrix branch for one element: float products summed left to right, then (float)(t*alpha + 0*0)"""
    t = terms[0][0] * terms[0][1]
    for a, b in terms[1:]:
        t = t + a * b
    assert t.dtype == np.float32
    return f32(float(t) * alpha + 0.0 * 0.0)


def set_pose(T):
    """KeyFrame::SetPose: Rwc = Rcw.t(), Ow = -Rwc*tcw -> (Twc 4 x 4, Ow)"""
    Rwc = T[:, :3].T
    Ow = np.array([gemm([(Rwc[i, k], T[k, 3]) for k in range(3)], -1.0) for i in range(3)], f32)
    Twc = np.eye(4, dtype=f32)
    Twc[:3, :3], Twc[:3, 3] = Rwc, Ow
    return Twc, Ow


def norm3(v):
    s = 0.0
    for c in range(3):
        s = s + float(v[c]) * float(v[c])
    return math.sqrt(s)


def model(c, centres="rule", slots=None, anchor=None):
    """-> (kf records in the caller's order, moved points in visiting order).  centres: how an observation's keyframe answers
    GetCameraCenter(): "rule" (new when listed with a rank below the owner's), "all_old", "all_new" """
    r, s = c.r, c.s
    slots = c.slots if slots is None else np.asarray(slots, np.int32)
    anchor = c.anchor if anchor is None else anchor
    K = len(slots)
    order = np.argsort(slots, kind="stable")                         # rule 1
    rank_of = {int(slots[i]): n for n, i in enumerate(order)}
    Scw = ([float(x) for x in c.Scw[:4]], [float(x) for x in c.Scw[4:7]], float(c.Scw[7]))
    Twc, _ = set_pose(c.poses[slots[anchor]].reshape(3, 4))
    kf = np.zeros(K, cs.KF_DTYPE)
    cor, non, new_ctr = {}, {}, {}
    for i in range(K):                                               # rule 2
        T = c.poses[slots[i]].reshape(3, 4)
        non[i] = sim3_of_pose(T)
        if i == anchor:
            cor[i] = Scw
        else:
            T4 = np.vstack([T, np.array([[0, 0, 0, 1]], f32)])
            Tic = np.array([[gemm([(T4[a, k], Twc[k, b]) for k in range(4)], 1.0) for b in range(4)] for a in range(3)], f32)
            cor[i] = sim3_mul(sim3_of_pose(Tic), Scw)
        q, t, sc = cor[i]
        R, inv = to_matrix(q), 1.0 / sc
        Tn = np.array([[f32(R[a][b]) for b in range(3)] + [f32(t[a] * inv)] for a in range(3)], f32)
        _, Ow = set_pose(Tn)
        new_ctr[int(slots[i])] = Ow
        kf[i]["corrected"], kf[i]["non_corrected"] = q + t + [sc], non[i][0] + non[i][1] + [1.0]
        kf[i]["Tiw"], kf[i]["Ow"] = Tn.reshape(12), Ow
    voting = (s.entries >= 0) & ((s.entries & cs.NO_VOTE) == 0) & ((s.kf_flags & cs.KF_SET) != 0)[:, None]
    obs = {}
    for k, i in np.argwhere(voting):
        obs.setdefault(int(s.entries[k, i]), []).append((int(k), int(i)))
    skip = set(int(x) for x in c.skip)
    owner = {}                                                       # rule 3: the lowest rank, then the lowest index
    for n, i in enumerate(order):
        row = s.entries[slots[i]]
        for idx in np.flatnonzero(row >= 0):
            pt = int(row[idx] & ~cs.NO_VOTE)
            if (s.pt_bad[pt] & 1) or pt in skip or pt in owner:
                continue
            owner[pt] = (n, int(i), int(idx))
    moved = sorted(owner.items(), key=lambda kv: (kv[1][0], kv[1][2]))
    pts = np.zeros(len(moved), cs.POINT_DTYPE)
    nlevels = len(cs.SF)
    for n, (pt, (rk, i, idx)) in enumerate(moved):
        P = sim3_map(sim3_inverse(cor[i]), sim3_map(non[i], [float(x) for x in r.pos[pt]]))      # rule 4
        P = np.array([f32(x) for x in P], f32)
        kf[i]["n_points"] += 1

        def centre(k):                                               # rule 5
            new = {"rule": k in rank_of and rank_of[k] < rk, "all_old": False, "all_new": k in rank_of}[centres]
            return new_ctr[k] if new else r.centres[k]

        o = pts[n]
        o["id"], o["owner_slot"], o["owner_idx"], o["pos"] = pt, slots[i], idx, P
        o["normal"], o["min_distance"], o["max_distance"] = r.normal[pt], r.min_d[pt], r.max_d[pt]
        lst, ref = obs.get(pt, []), int(r.ref_kf[pt])
        o["n_obs"] = len(lst)
        refq = [q for k, q in lst if k == ref]
        if not lst:
            o["status"] = cs.ST_NO_OBSERVATION
        elif ref < 0 or not refq:
            o["status"] = cs.ST_NO_REF
        elif int(s.octaves[ref, refq[0]]) >= nlevels:
            o["status"] = cs.ST_LEVEL_RANGE
        else:
            normal = np.zeros(3, f32)
            for k, _ in lst:
                v = P - centre(k)
                a = f32(1.0 / norm3(v))
                for d in range(3):
                    normal[d] = v[d] * a + normal[d]
            alpha = 1.0 / len(lst)
            for d in range(3):
                normal[d] = normal[d] + f32(0) if alpha == 1.0 else f32(float(normal[d]) * alpha)
            dist = f32(norm3(P - centre(ref)))
            mx = dist * cs.SF[int(s.octaves[ref, refq[0]])]
            o["status"], o["normal"], o["max_distance"], o["min_distance"] = cs.ST_DONE, normal, mx, mx / cs.SF[nlevels - 1]
    return kf, pts


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_ref_is_model(c, tag):
    br = np.zeros(len(cs.BRANCHES), np.int32)
    kf, pts, _ = cs.ref_correct(c, branches=br)
    mkf, mpts = model(c)
    for n in cs.KF_DTYPE.names:
        assert same(kf[n], mkf[n]), (tag, "kf", n, np.flatnonzero((kf[n] != mkf[n]).reshape(len(kf), -1).any(axis=1))[:8])
    assert len(pts) == len(mpts), (tag, len(pts), len(mpts))
    for n in cs.POINT_DTYPE.names:
        assert same(pts[n], mpts[n]), (tag, "point", n, np.flatnonzero((pts[n] != mpts[n]).reshape(len(pts), -1).any(axis=1))[:8])
    assert not np.isnan(pts["pos"]).any() and not np.isnan(pts["normal"]).any() and not np.isnan(kf["Tiw"]).any()
    return cs.seen(br), kf, pts


@pytest.mark.parametrize("family", sorted(cs.FAMILIES))
def test_the_restatement_equals_the_model_and_the_family_forces_its_branch(family):
    for seed in range(1, 11):
        c = cs.family_scene(family, seed)
        seen, kf, pts = assert_ref_is_model(c, (family, seed))
        for b in cs.FAMILIES[family]:
            assert seen[b] > 0, (family, seed, b, seen)
        assert seen["obs_reposed"] == 0, (family, seed)              # no observer of a rank below the owner's: rule 5's consequence
        assert seen["moved"] == len(pts) == kf["n_points"].sum() and len(np.unique(pts["id"])) == len(pts)      # every point once


def test_every_named_branch_is_forced_by_some_family():
    forced = set(b for v in cs.FAMILIES.values() for b in v)
    assert sorted(forced | {"obs_reposed", "anchor_kf", "other_kf"}) == sorted(cs.BRANCHES)


def test_what_the_families_must_show_beyond_their_counters():
    def one(family, name="p", seed=1):
        c = cs.family_scene(family, seed)
        _, pts, _ = cs.ref_correct(c)
        hit = pts[pts["id"] == c.named[name]]
        return c, hit[0] if len(hit) else None

    c, o = one("one_holder")
    assert len(c.holders(c.named["p"])) == 1 and o["owner_slot"] == cs.T0 + 1 and o["status"] == cs.ST_DONE
    c, o = one("several_holders_shuffled")
    assert [k for k, _ in c.holders(c.named["p"])] == [cs.T0 + 1, cs.T0 + 3, cs.T0 + 5] and o["owner_slot"] == cs.T0 + 1
    assert not np.array_equal(c.slots, np.sort(c.slots))            # the list is shuffled
    c, o = one("twice_in_owners_row")
    h = c.holders(c.named["p"])
    assert [k for k, _ in h] == [cs.T0 + 1, cs.T0 + 1, cs.T0 + 2] and o["owner_idx"] == h[0][1] < h[1][1] and o["n_obs"] == 3
    c, o = one("no_vote_only")
    assert o["status"] == cs.ST_NO_OBSERVATION and o["n_obs"] == 0 and not np.array_equal(o["pos"], c.r.pos[c.named["p"]])      # moved all the same
    assert np.array_equal(o["normal"], c.r.normal[c.named["p"]]) and o["max_distance"] == c.r.max_d[c.named["p"]]
    for fam in ("bad_point", "skipped_point"):
        assert one(fam)[1] is None
    c, o = one("observers_outside_list")
    assert o["n_obs"] == 2 and o["status"] == cs.ST_DONE
    c, o = one("observers_of_other_ranks")
    assert o["owner_slot"] == cs.T0 + 1 and o["n_obs"] == 3 and o["status"] == cs.ST_DONE
    for fam, st in (("ref_lower_rank", cs.ST_NO_REF), ("ref_higher_rank", cs.ST_DONE), ("ref_outside_list", cs.ST_DONE), ("ref_minus_1", cs.ST_NO_REF),
                    ("ref_not_observing", cs.ST_NO_REF)):
        c, o = one(fam)
        assert o["status"] == st and o["owner_slot"] == cs.T0 + 2, fam
    c, o = one("octave_out_of_range")
    assert o["status"] == cs.ST_LEVEL_RANGE and one("octave_out_of_range", "q")[1]["status"] == cs.ST_DONE
    c = cs.family_scene("k_1", 1)
    kf, pts, _ = cs.ref_correct(c)
    assert len(kf) == 1 and same(kf["corrected"][0], c.Scw) and kf["n_points"][0] == len(pts) > 0
    c = cs.family_scene("scale_one", 1)
    assert c.Scw[7] == 1.0 and cs.family_scene("scale_other", 1).Scw[7] != 1.0
    c = cs.family_scene("empty_keyframe", 1)
    kf, _, _ = cs.ref_correct(c)
    assert kf["n_points"][c.slots == cs.T0 + 7][0] == 0
    for fam, at in (("anchor_first", 0), ("anchor_last", -1)):
        c = cs.family_scene(fam, 1)
        kf, _, _ = cs.ref_correct(c)
        assert c.slots[c.anchor] == np.sort(c.slots)[at] and same(kf["corrected"][c.anchor], c.Scw)      # Scw itself, bit for bit


def test_a_shuffled_list_gives_the_same_bytes():
    c = cs.family_scene("several_holders_shuffled", 2)
    kf, pts, after = cs.ref_correct(c)
    perm = np.random.default_rng(3).permutation(len(c.slots))
    kf2, pts2, after2 = cs.ref_correct(c, c.slots[perm], int(np.flatnonzero(perm == c.anchor)[0]))
    assert same(kf[perm], kf2) and same(pts, pts2) and same(after.centres, after2.centres) and same(after.pos, after2.pos)
    mkf, mpts = model(c, slots=c.slots[perm], anchor=int(np.flatnonzero(perm == c.anchor)[0]))
    assert same(mkf, kf2) and same(mpts, pts2)


def test_the_centres_read_are_the_present_ones_and_the_choice_matters():
    """the model with the rule's reading, with every centre old and with every listed centre new: the first two agree byte for
    byte in every scene (no listed observer stands below the owner), the third differs -- so the scenes can tell the readings apart"""
    for family in ("observers_of_other_ranks", "several_holders_shuffled", "random"):
        for seed in (1, 2, 3):
            c = cs.family_scene(family, seed)
            _, rule = model(c)
            _, old = model(c, "all_old")
            _, new = model(c, "all_new")
            assert same(rule, old), (family, seed)
            assert not same(rule["normal"], new["normal"]) and not same(rule["max_distance"], new["max_distance"]), (family, seed)
    c = cs.family_scene("observers_of_other_ranks", 1)
    _, rule = model(c)
    _, new = model(c, "all_new")
    i = int(np.flatnonzero(rule["id"] == c.named["p"])[0])
    assert not same(rule["normal"][i], new["normal"][i])            # the family's own point reads its higher-ranked observers' old centres


def test_what_the_loop_leaves_in_the_world():
    """positions of all moved points, normals and bounds of the DONE ones, centres of the listed keyframes; nothing else"""
    c = cs.family_scene("random", 4)
    kf, pts, after = cs.ref_correct(c)
    before = (c.r.centres.copy(), c.r.pos.copy(), c.r.normal.copy(), c.r.min_d.copy(), c.r.max_d.copy())
    c.apply(kf, pts)
    for x, y in zip((c.r.centres, c.r.pos, c.r.normal, c.r.min_d, c.r.max_d), (after.centres, after.pos, after.normal, after.min_d, after.max_d)):
        assert same(np.ascontiguousarray(x), np.ascontiguousarray(y))
    unlisted = np.setdiff1d(np.arange(c.kfcap), c.slots)
    assert same(c.r.centres[unlisted], before[0][unlisted]) and (pts["status"] != cs.ST_DONE).any() and (pts["status"] == cs.ST_DONE).sum() > 50


def test_record_layouts_agree_with_the_mirror():
    from orbslamm_amd import map_pool as mp
    fields = [("OrbeKeyFrame", n) for n in mp.CORRECT_KF_DTYPE.names] + [("OrbePoint", n) for n in mp.CORRECT_POINT_DTYPE.names]
    src = "#include \"orbslamm_correct.h\"\n#include <stddef.h>\nextern \"C\" int layout(int i) {\n    const int v[] = {(int)sizeof(OrbeKeyFrame), (int)sizeof(OrbePoint), " + \
          ", ".join("(int)offsetof(%s, %s)" % f for f in fields) + "};\n    return v[i];\n}\n"
    d = tempfile.mkdtemp(prefix="correct_layout_")
    with open(os.path.join(d, "layout.cpp"), "w") as f:
        f.write(src)
    so = os.path.join(d, "liblayout.so")
    subprocess.check_call(["g++", "-std=c++11", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.cpp"), "-o", so])
    L = C.CDLL(so)
    got = [L.layout(i) for i in range(2 + len(fields))]
    want = [mp.CORRECT_KF_DTYPE.itemsize, mp.CORRECT_POINT_DTYPE.itemsize] + [mp.CORRECT_KF_DTYPE.fields[n][1] for n in mp.CORRECT_KF_DTYPE.names] + \
           [mp.CORRECT_POINT_DTYPE.fields[n][1] for n in mp.CORRECT_POINT_DTYPE.names]
    assert got == want
    assert mp.CORRECT_KF_DTYPE == cs.KF_DTYPE and mp.CORRECT_POINT_DTYPE == cs.POINT_DTYPE
    assert cs.shim().cor_kf_size() == 192 and cs.shim().cor_point_size() == 52


def test_the_symbols_are_exported():
    import orbslamm_amd
    L = lib()
    for name in ("orbu_point_set_ref_kf", "orbe_correct_sim3"):
        assert _lib.declarations()[name].header == "orbslamm_correct.h" and hasattr(L, name)
    for name in ("set_ref_kf", "correct_sim3"):
        assert hasattr(orbslamm_amd.KeyFrameStore, name)
    assert orbslamm_amd.CORRECT_KF_DTYPE.itemsize == 192 and orbslamm_amd.CORRECT_POINT_DTYPE.itemsize == 52
    header = open(os.path.join(ROOT, "include", "orbslamm_hip.h")).read()
    assert '#include "orbslamm_correct.h"' in header


def test_the_restatement_shares_no_code_with_the_library():
    from ref_shim import assert_shares_no_code_with_the_library
    assert_shares_no_code_with_the_library(os.path.join(ROOT, "tools", "correct_ref.hpp"))


def test_refusals_that_need_no_gpu():
    """argument checks come before the handle's: with a NULL store the entries still name the bad argument, and the outputs keep
    their bytes"""
    from orbslamm_amd import map_pool as mp
    L = lib()
    K = 3
    slots = np.arange(K, dtype=np.int32)
    Tiw = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (K, 1))
    Scw = np.array([0, 0, 0, 1, 0.5, -0.5, 0.25, 1.5])
    skip, sf = np.zeros(2, np.int32), cs.SF.copy()
    kf, pts, n = np.zeros(K, mp.CORRECT_KF_DTYPE), np.zeros(8, mp.CORRECT_POINT_DTYPE), C.c_int(-77)
    kf.view(np.uint8)[:] = 0xAB
    pts.view(np.uint8)[:] = 0xCD
    good = dict(slots=ptr(slots), Tiw=ptr(Tiw), K=K, anchor=1, Scw=ptr(Scw), skip=ptr(skip), n_skip=2, sf=ptr(sf), nlevels=8, commit=1, kf=ptr(kf), pts=ptr(pts),
                cap=8, n=C.byref(n))

    def call(**kw):
        a = dict(good, **kw)
        return L.orbe_correct_sim3(None, a["slots"], a["Tiw"], a["K"], a["anchor"], a["Scw"], a["skip"], a["n_skip"], a["sf"], a["nlevels"], a["commit"], a["kf"],
                                   a["pts"], a["cap"], a["n"])

    for kw in (dict(slots=None), dict(Tiw=None), dict(Scw=None), dict(skip=None), dict(sf=None), dict(kf=None), dict(pts=None), dict(n=None), dict(K=-1), dict(K=0),
               dict(n_skip=-1), dict(cap=-1), dict(anchor=-1), dict(anchor=K), dict(nlevels=0), dict(nlevels=17)):
        assert call(**kw) == ORBX_E_INVALID, kw
        assert b"null store" not in L.orbx_last_error(), kw
    for bad in (np.nan, np.inf, -np.inf):
        T = Tiw.copy()
        T[2, 7] = bad
        assert call(Tiw=ptr(T)) == ORBX_E_INVALID and b"not finite" in L.orbx_last_error()
        S = Scw.copy()
        S[5] = bad
        assert call(Scw=ptr(S)) == ORBX_E_INVALID and b"not finite" in L.orbx_last_error()
    for s in (0.0, -1.0):
        S = Scw.copy()
        S[7] = s
        assert call(Scw=ptr(S)) == ORBX_E_INVALID and b"scale" in L.orbx_last_error()
    assert call() == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert call(skip=None, n_skip=0, pts=None, cap=0) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert (kf.view(np.uint8) == 0xAB).all() and (pts.view(np.uint8) == 0xCD).all() and n.value == -77
    f = L.orbu_point_set_ref_kf
    ids, ks = np.zeros(2, np.int32), np.zeros(2, np.int32)
    assert f(None, ptr(ids), ptr(ks), -1) == ORBX_E_INVALID and f(None, None, ptr(ks), 2) == ORBX_E_INVALID and f(None, ptr(ids), None, 2) == ORBX_E_INVALID
    assert b"null store" not in L.orbx_last_error()
    assert f(None, ptr(ids), ptr(ks), 2) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert f(None, None, None, 0) == ORBX_OK


@pytest.mark.parametrize("name", ["correct_dropin_gpu"])
def test_the_dropin_compiles_against_the_mocks(name):
    """include/LoopClosing_hip.hpp's CorrectLoopPosesT over tests/cpp/mock_correct.hpp, warnings as errors (syntax and types only:
    nothing is linked or run)"""
    dropin.syntax_only(name)
