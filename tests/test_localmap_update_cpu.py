"""The restatement of Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (tools/localmap_update_ref.hpp) against
an independent model written here with dicts and sets, over seeds 1 .. 10 of every scene family; the occurrence of every named
branch in the family built for it; every refusal of the orbu_* entries that needs no GPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import localmap_update_cases as uc
from orbslamm_amd._lib import ORBX_E_INVALID, ORBX_E_UNSUPPORTED, ORBX_OK, lib, ptr

SEEDS = range(1, 11)


def model(s):
    """UpdateLocalKeyFrames + UpdateLocalPoints as the reference writes them: MapPoints with observation dicts, a counter dict, sets
    of included keyframes and points.  The two undefined orders are the defined ones: keyframes ascending by slot, children as
    given."""
    kfs = [k for k in range(s.kfcap) if s.kf_flags[k] & uc.KF_SET]
    observations = {}                                   # point -> {keyframe, ...} (MapPoint::mObservations)
    for k in kfs:
        for x in s.entries[k]:
            if x >= 0 and not x & uc.NO_VOTE:
                observations.setdefault(int(x), set()).add(k)
    counter = {}
    in_frame = set()
    for x in s.frame_ids:
        x = int(x)
        if x < 0 or s.pt_bad[x]:
            continue
        in_frame.add(x)
        for k in observations.get(x, ()):
            # a point twice in one keyframe is ONE observation of that keyframe per match slot in the store's terms: the store
            # votes per entry, so the model counts the entries
            counter[k] = counter.get(k, 0) + int(((s.entries[k] == x)).sum())
    votes = np.zeros(s.kfcap, np.int32)
    for k, v in counter.items():
        votes[k] = v
    out = {"votes": votes, "no_votes": not counter}
    if not counter:
        return out
    bad = lambda k: bool(s.kf_flags[k] & uc.KF_BAD)
    local, included, best, kf_max = [], set(), 0, -1
    for k in sorted(counter):
        if bad(k):
            continue
        if counter[k] > best:
            best, kf_max = counter[k], k
        local.append(k)
        included.add(k)

    def push(k):
        local.append(int(k))
        included.add(int(k))

    for k in list(local):
        if len(local) > s.max_keyframes:
            break
        for nb in s.neigh[k]:
            if nb >= 0 and not bad(nb) and int(nb) not in included:
                push(nb)
                break
        for ch in s.children[k, :s.nchildren[k]]:
            if not bad(ch) and int(ch) not in included:
                push(ch)
                break
        if s.parent[k] >= 0 and int(s.parent[k]) not in included:
            push(s.parent[k])
            break
    out.update(kf_max=kf_max, kf=np.array(local, np.int32))
    L, got = [], set()
    for k in local:
        for x in s.entries[k]:
            if x < 0:
                continue
            x = int(x) & ~uc.NO_VOTE
            if x in got or s.pt_bad[x]:
                continue
            got.add(x)
            L.append(x)
    L = np.array(L, np.int32)
    seen = np.array([1 if x in in_frame else 0 for x in L], np.uint8)
    out.update(L=L, seen=seen, S=L[seen == 0])
    return out


def assert_same(ref, want, tag):
    assert np.array_equal(ref["votes"], want["votes"]), (tag, "votes")
    assert ref["no_votes"] == want["no_votes"], (tag, "no_votes")
    if want["no_votes"]:
        return
    assert ref["kf_max"] == want["kf_max"], (tag, "kf_max")
    for key in ("kf", "L", "seen", "S"):
        assert np.array_equal(ref[key], want[key]), (tag, key)


@pytest.mark.parametrize("family", sorted(uc.FAMILIES))
def test_the_restatement_equals_the_model(family):
    seen_branches = dict.fromkeys(uc.BRANCHES, 0)
    for seed in SEEDS:
        s = uc.family_scene(family, seed)
        ref = uc.ref_update(s)
        assert_same(ref, model(s), (family, seed))
        obs = uc.ref_keyframes_from_observations(s, uc.observations(s))        # the votes cast per observation: the same lists
        assert np.array_equal(obs["votes"], ref["votes"]) and obs["kf_max"] == ref["kf_max"] and np.array_equal(obs["kf"], ref["kf"])
        for b, v in ref["branches"].items():
            seen_branches[b] += v
        # what the family is named after, seed by seed
        g = s.group()
        if family == "no_expansion":
            assert ref["branches"]["steps_run"] == 0 and np.array_equal(ref["kf"], g) and len(g) > s.max_keyframes
        if family == "group_at_limit":
            assert len(g) == s.max_keyframes and ref["branches"]["steps_run"] == 1 and len(ref["kf"]) > len(g)
        if family == "neighbours_all_included":
            assert ref["branches"]["neighbour_taken"] == 0
        if family == "children_full":
            assert (s.nchildren[g] == s.maxc).all()
        if family == "parent_bad_taken":
            assert s.kf_flags[ref["kf"][-1]] & uc.KF_BAD and ref["kf"][-1] == s.parent[g[0]] and ref["branches"]["steps_run"] == 1
        if family == "parent_break":
            assert ref["branches"]["steps_run"] == 3 < len(g) and ref["branches"]["size_break"] == 0 and ref["kf"][-1] == s.parent[g[2]]
        if family == "all_voted_bad":
            assert not ref["no_votes"] and ref["kf_max"] == -1 and len(ref["kf"]) == 0 and len(ref["L"]) == 0 and ref["votes"].max() > 0
        if family == "no_votes":
            assert ref["no_votes"] and (s.frame_ids >= 0).sum() > 20
        if family == "point_twice_in_frame":
            once = uc.ref_update(s, frame_ids=np.unique(s.frame_ids))
            assert (ref["votes"] > once["votes"]).any() and (ref["votes"] >= once["votes"]).all()
        if family == "point_in_many_keyframes":
            pt = s.pool_cap - 1
            first = ref["kf"][0]
            before = np.unique(s.entries[first][:np.flatnonzero((s.entries[first] & ~uc.NO_VOTE) == pt)[0]])
            assert (ref["L"] == pt).sum() == 1 and np.flatnonzero(ref["L"] == pt)[0] <= len(before)
        if family == "bad_points":
            assert not s.pt_bad[ref["L"]].any() and s.pt_bad[s.entries[ref["kf"]][s.entries[ref["kf"]] >= 0] & ~uc.NO_VOTE].any()
        if family in ("random", "random_wide") and not ref["no_votes"]:
            e = s.entries[ref["kf"]]
            assert ((e >= 0) & ((e & uc.NO_VOTE) != 0)).any()                     # NO_VOTE entries feed the list
            assert ref["seen"].any() and not ref["seen"].all()
    for b in uc.FAMILIES[family]:
        assert seen_branches[b] > 0, (family, b, seen_branches)


def test_a_point_twice_in_one_keyframe_is_listed_once_and_votes_per_entry():
    s = uc.Scene(2, 8, 0, 4)
    s.kf_flags[:] = uc.KF_SET
    s.entries[0, [1, 5]] = 2
    s.entries[1, 0] = 3
    s.frame_ids = np.array([2], np.int32)
    ref = uc.ref_update(s)
    assert list(ref["votes"]) == [2, 0] and list(ref["kf"]) == [0] and list(ref["L"]) == [2] and list(ref["seen"]) == [1] and len(ref["S"]) == 0
    assert_same(ref, model(s), "twice")


def test_local_points_alone_over_a_given_list():
    """the unit orbu_local_points is held to: repeats in the list, the empty list"""
    s = uc.family_scene("random", 3)
    lst = np.concatenate([s.set_slots()[::-1], s.set_slots()[:3]])
    r = uc.ref_points(s, lst)
    assert len(r["L"]) == len(np.unique(r["L"])) > 50 and np.array_equal(r["S"], r["L"][r["seen"] == 0])
    assert len(uc.ref_points(s, np.zeros(0, np.int32))["L"]) == 0


def test_refusals_that_need_no_gpu():
    """argument checks come before the handle's: with a NULL pool / store the entries still name the bad argument, and zero counts
    return ORBX_OK"""
    from orbslamm_amd import map_pool as mp
    L = lib()
    out = C.c_void_p()
    create = L.orbu_store_create
    assert create(None, 16, 64, 4, 100, None) == ORBX_E_INVALID
    for bad in ((0, 64, 4, 100), (16, 0, 4, 100), (16, 64, -1, 100), (16, 64, 4, 0)):
        assert create(None, *bad, C.byref(out)) == ORBX_E_INVALID
    for big in (((1 << 17) + 1, 64, 4, 100), (16, (1 << 13) + 1, 4, 100), (16, 64, 1025, 100), (16, 64, 4, mp.MAX_CAPACITY + 1), (1 << 17, 1 << 13, 4, 100)):
        assert create(None, *big, C.byref(out)) == ORBX_E_UNSUPPORTED
    assert create(None, 16, 64, 4, 100, C.byref(out)) == ORBX_E_INVALID and b"null pool" in L.orbx_last_error()
    assert L.orbu_store_destroy(None) == ORBX_OK
    one = np.zeros(1, np.int32)
    neigh = np.full(10, -1, np.int32)
    fl = np.zeros(1, np.uint8)

    def rec(nkf=1, slot=one, flags=fl, n=one, neigh_=neigh, parent=one, nch=one):
        return mp.OrbuKeyFrames(nkf, ptr(slot), ptr(flags), ptr(n), None, ptr(neigh_), ptr(parent), ptr(nch), None)

    for f in (L.orbu_kf_set, L.orbu_kf_set_graph):
        assert f(None, None) == ORBX_E_INVALID
        assert f(None, C.byref(rec(nkf=0))) == ORBX_OK
        assert f(None, C.byref(rec(nkf=-1))) == ORBX_E_INVALID
        assert f(None, C.byref(rec(slot=None))) == ORBX_E_INVALID
        assert f(None, C.byref(rec(neigh_=None))) == ORBX_E_INVALID
        assert f(None, C.byref(rec(nch=np.array([-1], np.int32)))) == ORBX_E_INVALID
        assert f(None, C.byref(rec(nch=np.array([2], np.int32)))) == ORBX_E_INVALID          # children counted, none given
        assert f(None, C.byref(rec())) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert L.orbu_kf_set(None, C.byref(rec(flags=None))) == ORBX_E_INVALID
    assert L.orbu_kf_set(None, C.byref(rec(n=np.array([3], np.int32)))) == ORBX_E_INVALID    # entries counted, none given
    assert L.orbu_kf_set_flags(None, None, None, 0) == ORBX_OK and L.orbu_kf_set_entries(None, 0, None, None, 0) == ORBX_OK
    assert L.orbu_kf_set_flags(None, ptr(one), ptr(fl), -1) == ORBX_E_INVALID
    assert L.orbu_kf_set_flags(None, None, ptr(fl), 1) == ORBX_E_INVALID and L.orbu_kf_set_flags(None, ptr(one), None, 1) == ORBX_E_INVALID
    assert L.orbu_kf_set_flags(None, ptr(one), ptr(fl), 1) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert L.orbu_kf_set_entries(None, -1, ptr(one), ptr(one), 1) == ORBX_E_INVALID
    assert L.orbu_kf_set_entries(None, 0, None, ptr(one), 1) == ORBX_E_INVALID and L.orbu_kf_set_entries(None, 0, ptr(one), None, 1) == ORBX_E_INVALID
    assert L.orbu_kf_set_entries(None, 0, ptr(one), ptr(one), 1) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    res = mp.OrbuResult()
    upd, pts = L.orbu_update_local_map, L.orbu_local_points
    assert upd(None, ptr(one), 1, 80, None) == ORBX_E_INVALID
    assert upd(None, None, 1, 80, C.byref(res)) == ORBX_E_INVALID and upd(None, ptr(one), -1, 80, C.byref(res)) == ORBX_E_INVALID
    assert upd(None, ptr(one), 1, -1, C.byref(res)) == ORBX_E_INVALID
    assert upd(None, ptr(one), (1 << 20) + 1, 80, C.byref(res)) == ORBX_E_UNSUPPORTED
    assert upd(None, ptr(one), 1, 80, C.byref(res)) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert pts(None, None, 1, ptr(one), 1, C.byref(res)) == ORBX_E_INVALID and pts(None, ptr(one), -1, ptr(one), 1, C.byref(res)) == ORBX_E_INVALID
    assert pts(None, ptr(one), 1, ptr(one), 1, None) == ORBX_E_INVALID
    assert pts(None, ptr(one), 1, ptr(one), 1, C.byref(res)) == ORBX_E_INVALID and b"null store" in L.orbx_last_error()
    assert L.orbu_debug_set_generation(None, 5) == ORBX_E_INVALID
    from orbslamm_amd._lib import OrbmProjParams
    import localmap_cases as lc
    pp = OrbmProjParams(3, 0.8, 0, 100)
    view = lc.make_view()
    br = np.arange(lc.NLEVELS + 1, dtype=np.float32) + 1
    f = C.c_float(1.0)
    res_track = L.orbw_track_local_map_resident
    assert res_track(None, 0, None, None, C.byref(pp), None, f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert res_track(None, 0, None, None, None, ptr(view), f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert res_track(None, 0, None, None, C.byref(pp), ptr(view), f, ptr(lc.SF), ptr(br[::-1].copy()), lc.NLEVELS, None) == ORBX_E_INVALID
    assert b"ascend" in L.orbx_last_error()
    assert res_track(None, 0, None, None, C.byref(pp), ptr(view), f, ptr(lc.SF), ptr(br), lc.NLEVELS, None) == ORBX_E_INVALID
    assert b"null store" in L.orbx_last_error()


def test_last_wins_staging_on_the_host_under_the_sanitizers(tmp_path):
    """stage_last_wins (orbslamm_amd/csrc/orbx_lastwins.hpp, under the three setters) with in-memory emit and flush, built with
    -fsanitize=address,undefined (tests/cpp/lastwins_host.cpp): window == launch and one window with more survivors than a launch
    (the flush inside a window), held to the last record of every key; a failing flush leaves the scratch zero"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lastwins_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(root, "tests", "cpp", "lastwins_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lastwins ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
