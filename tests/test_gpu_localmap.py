"""The map-point pool on the device (orbw_*): k_view_project against the restatement (tools/frustum_ref.hpp) AS
BITS for both gate sets over every scene family, the query counts 0, 1, 63, 64, 65 and 3 000, unordered and repeated ids, the id
capacity - 1, th of 1, 3 and 5 and two level tables; the two searches against the host-array path fed with the restatement's
arrays; the pool's update semantics; the drop-in on mocks.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import numpy as np
import pytest

import dropin
import localmap_cases as lc

from localmap_cases import Rig, new_pool

pytestmark = pytest.mark.gpu
@pytest.fixture(scope="module")
def rig(gpu):
    return Rig()


def assert_local_bits(got, ref, tag):
    uvr, lvl, cos, st = got
    assert st.tobytes() == ref["status"].tobytes(), (tag, "status", np.flatnonzero(st != ref["status"])[:8])
    assert uvr.tobytes() == ref["uvr"].tobytes(), (tag, "uvr")
    assert lvl.tobytes() == ref["lvl"].tobytes(), (tag, "lvl")
    assert cos.tobytes() == ref["viewcos"].tobytes(), (tag, "viewcos")


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_view_project_equals_the_restatement_as_bits(rig, family):
    """every family at th = 1, 3 and 5: the pool's records sit at scattered slots (capacity - 1 among them), the id list is
    unordered and repeats"""
    view, pts = lc.family_scene(family)
    n = len(pts)
    rng = np.random.default_rng(77)
    cap = 4 * n
    slots = rng.permutation(cap - 1)[:n - 1].astype(np.int32)
    slots = np.concatenate([slots, [cap - 1]]).astype(np.int32)
    pool = new_pool(rig, cap)
    pool.set(slots, pts)
    order = np.concatenate([rng.permutation(n), rng.integers(0, n, n // 3), [n - 1, n - 1]]).astype(np.int32)
    for th in (1.0, 3.0, 5.0):
        ref = lc.ref_local(view, pts, order, th)
        assert_local_bits(pool.view_project(view, slots[order], th, rig.sf, rig.breaks), ref, (family, th))
        for code in lc.FAMILY_STATUS[family]:
            assert (ref["status"] == code).sum() > 0
    pool.close()


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 3000])
def test_view_project_query_counts(rig, nq):
    view, pts = lc.family_scene("pan", 3, n=800)
    pool = new_pool(rig, len(pts))
    pool.set(np.arange(len(pts)), pts)
    ids = np.random.default_rng(nq).integers(0, len(pts), nq).astype(np.int32)
    ref = lc.ref_local(view, pts, ids, 3.0)
    got = pool.view_project(view, ids, 3.0, rig.sf, rig.breaks)
    assert got[0].shape == (nq, 3)
    assert_local_bits(got, ref, nq)
    again = pool.view_project(view, ids, 3.0, rig.sf, rig.breaks)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))       # the same call twice: the same bytes
    pool.close()


def test_two_level_tables(rig):
    """the scale factors and the break table of another pyramid (1.3 per level): swapping the tables changes the answer, so a swap
    cannot pass"""
    view, pts = lc.family_scene("pan", 5, n=900)
    ids = np.arange(len(pts), dtype=np.int32)
    pool = new_pool(rig, len(pts))
    pool.set(ids, pts)
    ref_a = lc.ref_local(view, pts, ids, 3.0, lc.SF, lc.LOG_SF)
    ref_b = lc.ref_local(view, pts, ids, 3.0, lc.SF_B, lc.LOG_SF_B)
    assert ref_a["lvl"].tobytes() != ref_b["lvl"].tobytes() and ref_a["uvr"].tobytes() != ref_b["uvr"].tobytes()
    assert_local_bits(pool.view_project(view, ids, 3.0, lc.SF, rig.breaks), ref_a, "table a")
    assert_local_bits(pool.view_project(view, ids, 3.0, lc.SF_B, rig.breaks_b), ref_b, "table b")
    pool.close()


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, None])
def test_view_project_frame_equals_the_restatement_as_bits(rig, nq):
    """the frame/frame gate set: the octaves come from the resident LastFrame (slot 0); ids of -1, z == 0, points behind"""
    keys, _ = rig.host[0]
    n = len(keys) if nq is None else nq
    view, pts, ids, _ = lc.frame_scene(2, n=len(keys))
    ids = ids[:n]
    pool = new_pool(rig, len(pts))
    pool.set(np.arange(len(pts)), pts)
    for th in (7.0, 15.0):
        ref = lc.ref_frame(view, pts, ids, keys["octave"][:n], th)
        uvr, lvl, _, st = pool.view_project(view, ids, th, rig.sf, None, last=(rig.fs, 0))
        assert st.tobytes() == ref["status"].tobytes() and uvr.tobytes() == ref["uvr"].tobytes() and lvl.tobytes() == ref["lvl"].tobytes(), (n, th)
    if nq is None:
        for code in (lc.ST_NO_POINT, lc.ST_DEPTH, lc.ST_OUT_OF_IMAGE, lc.ST_IN_VIEW):
            assert (ref["status"] == code).sum() > 0
    pool.close()


def local_map_of(rig, seed=1):
    """a local map made of the features of frames 0 and 1 as a slightly moved camera sees them: (view, points)"""
    rng = np.random.default_rng(900 + seed)
    view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.01), [0.02, -0.01, 0.03])
    keys = np.concatenate([k for k, _ in rig.host[:2]])
    desc = np.concatenate([d for _, d in rig.host[:2]])
    return view, lc.points_from_keys(rng, view, keys, lc.SF, desc)


def host_way_local(fs, slot, view, pts, ids, th, occ=None):
    """the parent's way: the restatement's arrays through orbm_track_local_points"""
    ref = lc.ref_local(view, pts, ids, th)
    fs.track_local_points(slot, ref["uvr"], ref["lvl"], pts["desc"][ids], ref["valid"], ref["obs"], occ)
    assign, nm = fs.results()
    return assign.copy(), int(nm[0]), ref


@pytest.mark.parametrize("th,with_occ", [(1.0, False), (3.0, True), (5.0, False)])
def test_track_local_map_equals_the_host_array_path(rig, th, with_occ):
    view, pts = local_map_of(rig)
    n = len(pts)
    rng = np.random.default_rng(int(th))
    pool = new_pool(rig, n)
    pool.set(np.arange(n), pts)
    ids = rng.permutation(n).astype(np.int32)
    nt = len(rig.host[2][0])
    occ = (rng.random(nt) < 0.3).astype(np.uint8) if with_occ else None
    want, wn, ref = host_way_local(rig.fs, 2, view, pts, ids, th, occ)
    pool.track_local_map(rig.fs, 2, view, ids, th, rig.sf, rig.breaks, occ)
    assign, nm = rig.fs.results()
    assert nm[0] == wn and np.array_equal(assign, want), (th, nm[0], wn)
    assert wn > 100
    st = pool.track_status(rig.fs)
    assert st.tobytes() == ref["status"].tobytes()
    pool.close()


def test_track_local_map_with_no_queries(rig):
    view, pts = local_map_of(rig)
    pool = new_pool(rig, 8)
    pool.track_local_map(rig.fs, 2, view, np.zeros(0, np.int32), 1.0, rig.sf, rig.breaks)
    assign, nm = rig.fs.results()
    assert nm[0] == 0 and (assign[0, :len(rig.host[2][0])] == -1).all() and pool.track_status(rig.fs).shape[0] == 0
    pool.close()


@pytest.mark.parametrize("mode,th,thd", [(4, 15.0, 100), (5, 10.0, 64)])
def test_track_frame_pose_equals_the_host_array_path(rig, mode, th, thd):
    """LastFrame = slot 0, CurrentFrame = slot 1, the rotation check on: LastFrame's MapPoints as CurrentFrame's pose sees them"""
    rng = np.random.default_rng(mode)
    keys, desc = rig.host[0]
    n = len(keys)
    view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.004), [0.01, 0.0, -0.02])
    pts = lc.points_from_keys(rng, view, keys, lc.SF, desc, jitter=1.5)
    pts["pos"][::37, 2] = view[0]["Ow"][2] - 4.0          # a few behind the camera
    pool = new_pool(rig, n + 5)
    slots = rng.permutation(n + 5)[:n].astype(np.int32)
    pool.set(slots, pts)
    feat = np.where(rng.random(n) < 0.85, np.arange(n), -1).astype(np.int32)     # per LastFrame feature: its point or -1
    last_ids = np.where(feat >= 0, slots[np.maximum(feat, 0)], -1).astype(np.int32)
    nt = len(rig.host[1][0])
    occ = (rng.random(nt) < 0.2).astype(np.uint8)
    ref = lc.ref_frame(view, pts, feat, keys["octave"], th)
    rig.fs.track_projected(1, 0, ref["uvr"], ref["lvl"], ref["valid"], ref["obs"], occ, th_dist=thd, nnratio=0.9, check_ori=True, mode=mode)
    a, nm = rig.fs.results()
    want, wn = a.copy(), int(nm[0])
    pool.track_frame_pose(rig.fs, 1, 0, view, last_ids, th, rig.sf, occ, th_dist=thd, nnratio=0.9, check_ori=True, mode=mode)
    assign, nm = rig.fs.results()
    assert nm[0] == wn and np.array_equal(assign, want), (mode, nm[0], wn)
    assert wn > 100
    assert pool.track_status(rig.fs).tobytes() == ref["status"].tobytes()
    assert (ref["status"] == lc.ST_DEPTH).sum() > 0 and (ref["status"] == lc.ST_NO_POINT).sum() > 0
    pool.close()


def test_pool_semantics(rig):
    from orbslamm_amd import OrbError
    view, pts = local_map_of(rig, 2)
    n = len(pts)
    ids = np.arange(n, dtype=np.int32)
    pool = new_pool(rig, n)
    # ids never set, or outside the pool, are refused on the host
    for bad in ([0], [n], [-1]):
        with pytest.raises(OrbError) as e:
            pool.track_local_map(rig.fs, 2, view, np.array(bad, np.int32), 1.0, rig.sf, rig.breaks)
        assert e.value.code == -1
    with pytest.raises(OrbError):
        pool.set_flags([3], [0])
    # a repeated id within one call takes the last record
    pool.set(np.concatenate([ids, ids[:50]]), np.concatenate([pts[::-1], pts[:50]]))
    pool.set(ids[50:], pts[50:])
    first, n1, ref1 = host_way_local(rig.fs, 2, view, pts, ids, 3.0)
    pool.track_local_map(rig.fs, 2, view, ids, 3.0, rig.sf, rig.breaks)
    a, nm = rig.fs.results()
    assert nm[0] == n1 and np.array_equal(a, first) and n1 > 100
    # set other records, search again: the second answer
    rng = np.random.default_rng(5)
    pts2 = pts.copy()
    moved = ids[::3]
    pts2["pos"][moved] += rng.normal(0, 0.02, (len(moved), 3)).astype(np.float32)
    pts2["desc"][ids[1::3]] = rng.integers(0, 256, (len(ids[1::3]), 32), dtype=np.uint8)
    pool.set(np.concatenate([moved, ids[1::3]]), pts2[np.concatenate([moved, ids[1::3]])])
    second, n2, _ = host_way_local(rig.fs, 2, view, pts2, ids, 3.0)
    assert not np.array_equal(second, first)
    pool.track_local_map(rig.fs, 2, view, ids, 3.0, rig.sf, rig.breaks)
    a, nm = rig.fs.results()
    assert nm[0] == n2 and np.array_equal(a, second)
    again = a.copy()
    pool.track_local_map(rig.fs, 2, view, ids, 3.0, rig.sf, rig.breaks)            # the same call twice: identical bytes
    a, nm = rig.fs.results()
    assert a.tobytes() == again.tobytes() and nm[0] == n2
    # a flags-only change turns a match off
    nt = len(rig.host[2][0])                       # (the table has `cap` entries; those behind the frame's features are not results)
    taken = np.unique(second[0, :nt][second[0, :nt] >= 0])
    off = taken[:20]
    fl = pts2["flags"].copy()
    fl[off] |= lc.FLAG_BAD
    pool.set_flags(off, fl[off])
    pts3 = pts2.copy()
    pts3["flags"] = fl
    third, n3, ref3 = host_way_local(rig.fs, 2, view, pts3, ids, 3.0)
    assert not np.isin(off, third[0, :nt]).any() and np.isin(off, second[0, :nt]).all() and len(off) == 20
    pool.track_local_map(rig.fs, 2, view, ids, 3.0, rig.sf, rig.breaks)
    a, nm = rig.fs.results()
    assert nm[0] == n3 and np.array_equal(a, third)
    assert (pool.track_status(rig.fs)[off] == lc.ST_BAD).all()
    # two frame sets share one pool
    fs2 = rig.new_frame_set()
    fs2.build_from_extractor(0, rig.gex)
    pool.track_local_map(fs2, 2, view, ids, 3.0, rig.sf, rig.breaks)
    pool.track_local_map(rig.fs, 1, view, ids, 3.0, rig.sf, rig.breaks)
    a2, nm2 = fs2.results()
    assert nm2[0] == n3 and np.array_equal(a2, third)
    other, no, _ = host_way_local(fs2, 1, view, pts3, ids, 3.0)
    a1, nm1 = rig.fs.results()
    assert nm1[0] == no and np.array_equal(a1, other)
    fs2.close()
    # four searches in a row, each read back with back = 0 .. 3
    wants = []
    for k, th in enumerate((1.0, 3.0, 5.0, 2.0)):
        sub = ids[k::2]
        w_, n_, r_ = host_way_local(rig.fs, 2, view, pts3, sub, th)
        wants.append((w_, n_, r_["status"]))
    for k, th in enumerate((1.0, 3.0, 5.0, 2.0)):
        pool.track_local_map(rig.fs, 2, view, ids[k::2], th, rig.sf, rig.breaks)
    for back in range(4):
        w_, n_, s_ = wants[3 - back]
        a, nm = rig.fs.results(back)
        assert nm[0] == n_ and np.array_equal(a, w_), back
        assert pool.track_status(rig.fs, back).tobytes() == s_.tobytes(), back
    pool.close()


def last_of_each(keys):
    """the index of the last record of every key: the records that win a setter call"""
    keys = np.asarray(keys)
    return np.array([np.flatnonzero(keys == k)[-1] for k in np.unique(keys)])


def test_a_repeated_id_on_both_sides_of_a_staging_chunk(rig):
    """one orbw_pool_set and one orbw_pool_set_flags of 65 536 + 4 records (a setter launch stages 65 536) whose ids cycle over a
    pool of 8: ids 0 .. 3 repeat behind the chunk's end.  A fresh pool given the eight last records alone projects to the same bytes"""
    n = (1 << 16) + 4
    i = np.arange(n)
    ids = (i % 8).astype(np.int32)
    view = lc.make_view()
    K = lc.K_A.astype(np.float64)
    z = np.where(i % 3 == 0, -1.0, 2.0 + (i % 5) * 0.25)
    Xc = np.stack([(20 + i * 37 % 600 - K[2]) / K[0] * z, (20 + i * 53 % 440 - K[3]) / K[1] * z, z], axis=1)
    dist = np.linalg.norm(Xc, axis=1)
    desc = ((i[:, None] * (np.arange(32) + 1) >> 3) & 255).astype(np.uint8)
    pts = np.zeros(n, lc.POINT_DTYPE)
    pts["pos"], pts["normal"], pts["desc"], pts["flags"] = Xc, Xc / dist[:, None], desc, lc.FLAG_OBSERVED
    pts["max_distance"] = dist * 1.5
    pts["min_distance"] = pts["max_distance"] / lc.SF[-1]
    fl = np.where(i % 5 == 0, lc.FLAG_BAD, lc.FLAG_OBSERVED * (i % 2)).astype(np.uint8)
    win = last_of_each(ids)
    assert (win >= 1 << 16).sum() == 4 and (win < 1 << 16).sum() == 4            # winners in the second launch and in the first
    x, y = new_pool(rig, 8), new_pool(rig, 8)
    x.set(ids, pts)
    x.set_flags(ids, fl)
    y.set(ids[win], pts[win])
    y.set_flags(ids[win], fl[win])
    q = np.arange(8, dtype=np.int32)
    gx, gy = x.view_project(view, q, 3.0, rig.sf, rig.breaks), y.view_project(view, q, 3.0, rig.sf, rig.breaks)
    for a, b, name in zip(gx, gy, ("uvr", "lvl", "viewcos", "status")):
        assert a.tobytes() == b.tobytes(), name
    assert len(np.unique(gx[3])) >= 2, gx[3]
    x.close()
    y.close()


def test_localmap_dropin_on_mock_tracking(gpu):
    """include/Tracking_hip.hpp (SearchLocalPointsT::Run) on mock frames and MapPoints (tests/cpp/localmap_dropin_gpu.cpp) against the
    serial reference loop over the same mocks"""
    dropin.run(dropin.build("localmap_dropin_gpu"), timeout=300, marker="localmap dropin ok")
