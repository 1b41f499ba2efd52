"""The restatement of KeyFrame::UpdateConnections and KeyFrameCulling's counts (tools/covis_ref.hpp) against an
independent model written here with dicts, over seeds 1 .. 10 of every scene family; the occurrence of every named branch in the
family built for it; the layouts of the ABI's records against the mirror's; every refusal of the entries that needs no GPU; the
drop-ins against the mocks.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import covis_cases as cc
import dropin
from orbslamm_amd import _lib
from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, ORBX_OK, lib, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(1, 11)


def observations(s):
    """MapPoint::mObservations: point -> [(keyframe, feature), ...], one per voting entry of a set keyframe"""
    obs = {}
    for k in s.set_slots():
        for i, x in enumerate(s.entries[k]):
            if x >= 0 and not x & cc.NO_VOTE:
                obs.setdefault(int(x), []).append((int(k), i))
    return obs


def model_connections(s, obs, k, th):
    """UpdateConnections as the reference writes it, the two heap-address orders being slot order"""
    counter = {}
    for x in s.entries[k]:
        if x < 0 or s.pt_bad[int(x) & ~cc.NO_VOTE]:
            continue
        for kf, _ in obs.get(int(x) & ~cc.NO_VOTE, ()):
            if kf != k:
                counter[kf] = counter.get(kf, 0) + 1
    if not counter:
        return {"status": 1, "kf_max": -1, "n_max": 0, "cnt": [], "ord": []}
    n_max = max(counter.values())
    kf_max = min(kf for kf, w in counter.items() if w == n_max)
    members = [(kf, w) for kf, w in counter.items() if w >= th] or [(kf_max, n_max)]
    return {"status": 0, "kf_max": kf_max, "n_max": n_max, "cnt": sorted(counter.items()), "ord": sorted(members, key=lambda m: (-m[1], -m[0]))}


def model_culling(s, obs, k, th_obs):
    n_mps = n_red = 0
    for i, x in enumerate(s.entries[k]):
        if x < 0 or s.pt_bad[int(x) & ~cc.NO_VOTE]:
            continue
        n_mps += 1
        o = obs.get(int(x) & ~cc.NO_VOTE, ())
        if len(o) > th_obs:
            level = int(s.octaves[k, i])
            if sum(1 for kf, j in o if kf != k and int(s.octaves[kf, j]) <= level + 1) >= th_obs:
                n_red += 1
    return n_mps, n_red, int(n_red > 0.9 * n_mps)


def assert_ref_is_model(s, tag, th=cc.TH, th_obs=cc.TH_OBS):
    ref = cc.Ref(s)
    tg = s.set_slots()
    conn, cull = ref.connections(tg, th), ref.culling(tg, th_obs)
    obs = observations(s)
    for t, k in enumerate(tg):
        m = model_connections(s, obs, int(k), th)
        assert (conn["status"][t], conn["kf_max"][t], conn["n_max"][t]) == (m["status"], m["kf_max"], m["n_max"]), (tag, k)
        kf, w = cc.row(conn, t, "cnt")
        assert list(zip(kf.tolist(), w.tolist())) == m["cnt"], (tag, k, "counter")
        kf, w = cc.row(conn, t, "ord")
        assert list(zip(kf.tolist(), w.tolist())) == m["ord"], (tag, k, "ordered")
        assert (cull["n_mps"][t], cull["n_redundant"][t], cull["redundant"][t]) == model_culling(s, obs, int(k), th_obs), (tag, k, "culling")
    return ref, tg, conn, cull


@pytest.mark.parametrize("family", sorted(cc.FAMILIES))
def test_the_restatement_equals_the_model(family):
    seen = dict.fromkeys(cc.BRANCHES, 0)
    for seed in SEEDS:
        s = cc.family_scene(family, seed)
        ref, tg, conn, cull = assert_ref_is_model(s, (family, seed))
        for b, v in ref.seen().items():
            seen[b] += v
        # what the family is named after, seed by seed
        a = cc.T0
        if family == "random":
            assert conn["ord_start"][-1] > len(tg) and (conn["cnt_w"] >= cc.TH).any() and (conn["cnt_w"] < cc.TH).any()
            continue
        t = int(np.flatnonzero(tg == a)[0])
        cnt = dict(zip(*[x.tolist() for x in cc.row(conn, t, "cnt")]))
        okf, ow = [x.tolist() for x in cc.row(conn, t, "ord")]
        if family == "weights_14_and_15":
            assert cnt == {a + 1: 14, a + 2: 15, a + 3: 16} and okf == [a + 3, a + 2] and ow == [16, 15]
        if family == "two_at_the_maximum":
            assert conn["kf_max"][t] == a + 1 and conn["n_max"][t] == 20 and okf == [a + 2, a + 1, a + 3] and ow == [20, 20, 17]
        if family == "three_at_one_weight":
            assert okf == [a + 3, a + 2, a + 1, a + 4] and ow == [16, 16, 16, 15]
        if family == "none_at_th":
            assert max(cnt.values()) < cc.TH and okf == [a + 2] and ow == [9] and conn["kf_max"][t] == a + 2
        if family == "no_observed_point":
            for k in (a, a + 1, a + 2):
                tk = int(np.flatnonzero(tg == k)[0])
                assert conn["status"][tk] == 1 and conn["kf_max"][tk] == -1 and conn["cnt_start"][tk] == conn["cnt_start"][tk + 1]
                assert conn["ord_start"][tk] == conn["ord_start"][tk + 1]
            assert cull["n_mps"][t] == 10 and cull["n_redundant"][t] == 0
        if family == "duplicates_no_vote_bad":
            assert cnt == {a + 1: 3, a + 2: 4, a + 3: 16}      # the duplicate 2 and 4, the NO_VOTE slot 1 more, the bad point nothing
        if family == "observations_at_th":
            assert (cull["n_mps"][t], cull["n_redundant"][t]) == (6, 3)
        if family == "octave_edges":
            assert (cull["n_mps"][t], cull["n_redundant"][t]) == (4, 4)
        if family == "qualifying_edges":
            assert (cull["n_mps"][t], cull["n_redundant"][t]) == (6, 3)
        if family == "ratio_edges":
            assert [(cull["n_mps"][t + j], cull["n_redundant"][t + j], cull["redundant"][t + j]) for j in range(3)] == [(10, 9, 0), (10, 10, 1), (20, 19, 1)]
        if family == "own_slots_no_vote":
            assert (cull["n_mps"][t], cull["n_redundant"][t], cull["redundant"][t]) == (12, 12, 1) and conn["status"][t] == 0
    for b in cc.FAMILIES[family]:
        assert seen[b] > 0, (family, b, seen)


def test_every_named_branch_is_forced_by_some_family():
    assert sorted(set(b for v in cc.FAMILIES.values() for b in v)) == sorted(cc.BRANCHES)


@pytest.mark.parametrize("shape", [dict(nkf=1, crafted=0), dict(nkf=2, crafted=0), dict(nkf=65, crafted=0, npts=900),
                                   dict(nkf=12, stride=2048, npts=3000, crafted=0, spread=4.0), dict(nkf=30, stride=65, crafted=0)])
def test_the_restatement_equals_the_model_at_other_shapes(shape):
    s = cc.random_scene(np.random.default_rng(7), **shape)
    assert_ref_is_model(s, str(shape))
    assert_ref_is_model(s, str(shape), th=1, th_obs=0)


def test_record_layouts_agree_with_the_mirror():
    from orbslamm_amd import map_pool as mp
    src = """#include "orbslamm_covis.h"
#include <stddef.h>
extern "C" int layout(int i) {
    const int v[] = {(int)sizeof(OrbnConnections), (int)offsetof(OrbnConnections, status), (int)offsetof(OrbnConnections, kf_max), (int)offsetof(OrbnConnections, n_max),
                     (int)offsetof(OrbnConnections, cnt_start), (int)offsetof(OrbnConnections, cnt_kf), (int)offsetof(OrbnConnections, cnt_w),
                     (int)offsetof(OrbnConnections, ord_start), (int)offsetof(OrbnConnections, ord_kf), (int)offsetof(OrbnConnections, ord_w),
                     (int)sizeof(OrbnCulling), (int)offsetof(OrbnCulling, n_mps), (int)offsetof(OrbnCulling, n_redundant), (int)offsetof(OrbnCulling, redundant),
                     ORBN_OK, ORBN_EMPTY, ORBN_MAX_OCTAVE_VALUES};
    return v[i];
}
"""
    d = tempfile.mkdtemp(prefix="covis_layout_")
    with open(os.path.join(d, "layout.cpp"), "w") as f:
        f.write(src)
    so = os.path.join(d, "liblayout.so")
    subprocess.check_call(["g++", "-std=c++11", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.cpp"), "-o", so])
    got = [C.CDLL(so).layout(i) for i in range(17)]
    a, b = mp.OrbnConnections, mp.OrbnCulling
    want = [C.sizeof(a)] + [getattr(a, n).offset for n in mp.Connections.NAMES] + [C.sizeof(b)] + [getattr(b, n).offset for n in mp.Culling.NAMES]
    assert got == want + [mp.COVIS_OK, mp.COVIS_EMPTY, mp.MAX_OCTAVE_VALUES]
    assert a.K.offset == 0 and b.K.offset == 0 and a.K.size == 4


def test_the_symbols_are_exported():
    L = lib()
    for name in ("orbu_kf_set_octaves", "orbn_update_connections", "orbn_culling_counts"):
        assert _lib.declarations()[name].header == "orbslamm_covis.h" and hasattr(L, name)


def test_refusals_that_need_no_gpu():
    """argument checks come before the handle's: with a NULL store the entries still name the bad argument, and zero counts
    return ORBX_OK"""
    from orbslamm_amd import map_pool as mp
    L = lib()
    one = np.zeros(1, np.int32)
    octs = np.zeros(4, np.uint8)
    so = L.orbu_kf_set_octaves
    assert so(None, 0, ptr(octs), -1) == ORBX_E_INVALID
    assert so(None, -1, ptr(octs), 4) == ORBX_E_INVALID
    assert so(None, 0, None, 4) == ORBX_E_INVALID
    assert so(None, 0, ptr(octs), 4) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    for f, res in ((L.orbn_update_connections, mp.OrbnConnections()), (L.orbn_culling_counts, mp.OrbnCulling())):
        res.K = 77
        assert f(None, ptr(one), 1, 3, None) == ORBX_E_INVALID
        assert f(None, ptr(one), -1, 3, C.byref(res)) == ORBX_E_INVALID
        assert f(None, None, 1, 3, C.byref(res)) == ORBX_E_INVALID
        assert f(None, ptr(one), 1, -1, C.byref(res)) == ORBX_E_INVALID
        assert f(None, ptr(one), (1 << 17) + 1, 3, C.byref(res)) == ORBX_E_UNSUPPORTED
        assert f(None, ptr(one), 1, 3, C.byref(res)) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
        assert res.K == 77                                       # a refusal leaves the result as it was
        assert f(None, None, 0, 3, C.byref(res)) == ORBX_OK and res.K == 0


@pytest.mark.parametrize("name", ["covis_dropin_gpu"])
def test_the_dropins_compile_against_the_mocks(name):
    """include/KeyFrame_hip.hpp and KeyFrameCullingT of include/LocalMapping_hip.hpp over tests/cpp/mock_covis.hpp, warnings as errors
    (syntax and types only: nothing is linked or run)"""
    dropin.syntax_only(name)
