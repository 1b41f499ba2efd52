"""The restatement of the map-point pool's projections (tools/frustum_ref.hpp) against an independent float64
numpy model of Frame::isInFrustum's geometry (localmap_cases.model64), the coverage of every status by the family built for it,
and every refusal of the orbw_* entries that needs no GPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import localmap_cases as lc
from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, ORBX_OK, lib, ptr

# measured over seeds 1 .. 10 of both scenes (3 000 points each, the points both models keep): max |u - u64| = 1.54e-4 px, max
# |v - v64| = 1.28e-4 px; the assertion stands at 10 x the larger
UV_BOUND = 10 * 1.54e-4


@pytest.mark.parametrize("scene", ["pan", "translation"])
@pytest.mark.parametrize("seed", list(lc.SEEDS))
def test_status_against_the_float64_model(scene, seed):
    view, pts = lc.family_scene(scene, seed, n=3000)
    ids = np.random.default_rng(seed).permutation(len(pts)).astype(np.int32)
    ref = lc.ref_local(view, pts, ids, 1.0)
    status, level, u, v, near = lc.model64(view, pts, ids, 1.0)
    share = near.mean()
    print("scene %s seed %d: %.2f %% within %g of a gate" % (scene, seed, 100 * share, lc.MARGIN))
    assert share <= 0.05
    keep = ~near
    assert np.array_equal(ref["status"][keep], status[keep])
    inview = keep & (status == lc.ST_IN_VIEW)
    assert inview.sum() > 300
    assert np.array_equal(ref["lvl"][inview, 1], level[inview]) and np.array_equal(ref["lvl"][inview, 0], level[inview] - 1)
    du = np.abs(ref["uvr"][inview, 0].astype(np.float64) - u[inview]).max()
    dv = np.abs(ref["uvr"][inview, 1].astype(np.float64) - v[inview]).max()
    print("max |u - u64| = %.3g px, max |v - v64| = %.3g px" % (du, dv))
    assert du <= UV_BOUND and dv <= UV_BOUND
    assert np.array_equal(ref["valid"], (ref["status"] == lc.ST_IN_VIEW).astype(np.uint8))
    assert np.array_equal(ref["obs"], (pts["flags"][ids] >> 1) & 1)


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_every_status_occurs_in_its_family(family):
    view, pts = lc.family_scene(family)
    ref = lc.ref_local(view, pts, np.arange(len(pts), dtype=np.int32), 3.0)
    for code in lc.FAMILY_STATUS[family]:
        assert (ref["status"] == code).sum() > 0, (family, code)
    if family == "level_edges":
        lr = ref["status"] == lc.ST_LEVEL_RANGE
        assert (ref["lvl"][lr, 1] == -1).sum() > 0 and (ref["lvl"][lr, 1] == lc.NLEVELS).sum() > 0
    if family == "pcz_zero":
        out = ref["status"] == lc.ST_OUT_OF_IMAGE
        assert np.isnan(ref["uvr"][out, 0]).sum() > 0 and np.isinf(ref["uvr"][out, 0]).sum() > 0
    if family == "on_bounds":
        iv = ref["status"] == lc.ST_IN_VIEW
        u, v = ref["uvr"][iv, 0], ref["uvr"][iv, 1]
        assert (u == 0).sum() > 0 and (u == lc.W).sum() > 0 and (v == 0).sum() > 0 and (v == lc.H).sum() > 0
    if family == "viewcos_edges":
        iv = ref["status"] == lc.ST_IN_VIEW
        assert (ref["uvr"][iv, 2] / lc.SF[ref["lvl"][iv, 1]] == np.float32(7.5)).sum() > 0     # 2.5 x th
        assert (ref["uvr"][iv, 2] / lc.SF[ref["lvl"][iv, 1]] == np.float32(12.0)).sum() > 0    # 4.0 x th


def test_frame_gate_set_statuses():
    view, pts, ids, octaves = lc.frame_scene(1)
    ref = lc.ref_frame(view, pts, ids, octaves, 15.0)
    for code in (lc.ST_NO_POINT, lc.ST_DEPTH, lc.ST_OUT_OF_IMAGE, lc.ST_IN_VIEW):
        assert (ref["status"] == code).sum() > 0, code
    assert np.array_equal(ref["status"] == lc.ST_NO_POINT, ids < 0)
    iv = ref["status"] == lc.ST_IN_VIEW
    assert np.array_equal(ref["uvr"][iv, 2], np.float32(15.0) * lc.SF[octaves[iv]])
    assert np.array_equal(ref["lvl"][iv, 0], octaves[iv] - 1) and np.array_equal(ref["lvl"][iv, 1], octaves[iv] + 1)


def test_refusals_that_need_no_gpu():
    """argument checks come before the handle's: with a NULL handle / pool / frame set the entries still name the bad argument, and
    zero counts return ORBX_OK"""
    from orbslamm_amd import map_pool as mp
    L = lib()
    out = C.c_void_p()
    assert L.orbw_pool_create(None, 16, None) == ORBX_E_INVALID
    assert L.orbw_pool_create(None, 0, C.byref(out)) == ORBX_E_INVALID
    assert L.orbw_pool_create(None, -5, C.byref(out)) == ORBX_E_INVALID
    assert L.orbw_pool_create(None, mp.MAX_CAPACITY + 1, C.byref(out)) == ORBX_E_UNSUPPORTED
    assert L.orbw_pool_create(None, mp.MAX_CAPACITY, C.byref(out)) == ORBX_E_INVALID and b"null handle" in L.orbx_last_error()
    assert L.orbw_pool_destroy(None) == ORBX_OK
    ids = np.zeros(4, np.int32)
    pts = np.zeros(4, mp.POINT_DTYPE)
    fl = np.zeros(4, np.uint8)
    assert L.orbw_pool_set(None, None, None, 0) == ORBX_OK
    assert L.orbw_pool_set_flags(None, None, None, 0) == ORBX_OK
    assert L.orbw_pool_set(None, ptr(ids), ptr(pts), -1) == ORBX_E_INVALID
    assert L.orbw_pool_set(None, None, ptr(pts), 4) == ORBX_E_INVALID
    assert L.orbw_pool_set(None, ptr(ids), None, 4) == ORBX_E_INVALID
    assert L.orbw_pool_set_flags(None, ptr(ids), None, 4) == ORBX_E_INVALID
    assert L.orbw_pool_set_flags(None, ptr(ids), ptr(fl), -2) == ORBX_E_INVALID
    assert L.orbw_pool_set(None, ptr(ids), ptr(pts), 4) == ORBX_E_INVALID and b"null pool" in L.orbx_last_error()
    view = lc.make_view()
    br = np.arange(lc.NLEVELS + 1, dtype=np.float32) + 1
    uvr, lvl, cos, st = np.zeros((4, 3), np.float32), np.zeros((4, 2), np.int8), np.zeros(4, np.float32), np.zeros(4, np.uint8)
    f = C.c_float(1.0)

    def project(view_=view, ids_=ids, nq=4, sf=lc.SF, br_=br, nl=lc.NLEVELS):
        return L.orbw_view_project(None, None, ptr(view_), ptr(ids_), nq, f, ptr(sf), ptr(br_), nl, ptr(uvr), ptr(lvl), ptr(cos), ptr(st))

    assert project(nq=0) == ORBX_OK
    assert L.orbw_view_project(None, None, None, None, 0, f, None, None, 0, None, None, None, None) == ORBX_OK
    assert project(nq=-1) == ORBX_E_INVALID
    assert project(view_=None) == ORBX_E_INVALID
    assert project(ids_=None) == ORBX_E_INVALID
    assert project(sf=None) == ORBX_E_INVALID
    assert project(br_=None) == ORBX_E_INVALID
    assert project(nl=0) == ORBX_E_INVALID and project(nl=17) == ORBX_E_INVALID
    assert project(br_=br[::-1].copy()) == ORBX_E_INVALID and b"ascend" in L.orbx_last_error()
    assert project() == ORBX_E_INVALID and b"null handle" in L.orbx_last_error()
    assert L.orbw_view_project_frame(None, 0, None, None, None, 0, f, None, None, None, None) == ORBX_OK
    assert L.orbw_view_project_frame(None, 0, None, ptr(view), ptr(ids), -1, f, ptr(lc.SF), ptr(uvr), ptr(lvl), ptr(st)) == ORBX_E_INVALID
    assert L.orbw_view_project_frame(None, 0, None, None, ptr(ids), 4, f, ptr(lc.SF), ptr(uvr), ptr(lvl), ptr(st)) == ORBX_E_INVALID
    assert L.orbw_view_project_frame(None, 0, None, ptr(view), ptr(ids), 4, f, ptr(lc.SF), ptr(uvr), ptr(lvl), ptr(st)) == ORBX_E_INVALID
    assert b"null frame set" in L.orbx_last_error()
    from orbslamm_amd._lib import OrbmProjParams
    pp = OrbmProjParams(3, 0.8, 0, 100)
    track = L.orbw_track_local_map
    assert track(None, 0, None, C.byref(pp), ptr(view), ptr(ids), -1, f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert track(None, 0, None, C.byref(pp), None, ptr(ids), 4, f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert track(None, 0, None, None, ptr(view), ptr(ids), 4, f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert track(None, 0, None, C.byref(pp), ptr(view), ptr(ids), 4, f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert b"null frame set" in L.orbx_last_error()
    pose = L.orbw_track_frame_pose
    assert pose(None, 0, -1, None, C.byref(pp), ptr(view), ptr(ids), 4, f, ptr(lc.SF), None) == ORBX_E_INVALID
    assert pose(None, 0, 1, None, C.byref(pp), ptr(view), None, 4, f, ptr(lc.SF), None) == ORBX_E_INVALID
    assert pose(None, 0, 1, None, C.byref(pp), ptr(view), ptr(ids), 4, f, ptr(lc.SF), None) == ORBX_E_INVALID and b"null frame set" in L.orbx_last_error()
    n = C.c_int(0)
    assert L.orbw_track_status(None, 0, None, C.byref(n)) == ORBX_E_INVALID
    assert L.orbw_track_status(None, 0, C.byref(out), C.byref(n)) == ORBX_E_INVALID
