"""The call table of the one-handle tests (tests/one_handle_cases.py) cannot go stale: every host file that reserves the shared
S_BLOCK of a matcher handle, and every export that takes a matcher handle, is run by a table entry or named below with its reason; the
seeded schedules have the two properties tests/test_gpu_one_handle.py relies on; and the table's cases reach distinct verdicts in
the restatements, so that bytes equal everywhere cannot come from an early return everywhere."""
import glob
import os
import re

import pytest

import one_handle_cases as oh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbslamm_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

# exports that take an orbm_t* and are in no table entry: one line of reason each
NOT_IN_THE_TABLE = {
    "orbm_create": "every rig makes its matcher with it",
    "orbm_destroy": "every rig closes its matcher with it",
    "orbm_thread_handle": "hands out a handle; runs nothing on it",
    "orbm_alloc_stats": "reads two counters; the steady-state test reads them through it",
    "orbm_last_search_stats": "reads two members; the test of a legacy search behind an orbq chain reads them through it",
    "orbq_debug_reloc_arena": "sets and reads relocArena; the arena test of test_gpu_one_handle.py drives it",
    "orbq_debug_motion_arena": "sets and reads motionArena; the arena test of test_gpu_one_handle.py drives it",
    "orbi_create_frame": "orbi_create with a resident reference frame: the same solver, its blocks its own",
    "orbp_create_frame": "orbp_create with a resident frame: the same solver, its blocks its own",
    "orbl_fuse_batch_frames": "fuse_batch with resident targets: the same orbl_fuse_core behind it",
    "orbc_search_and_fuse_frames": "search_and_fuse with resident targets: the same orbc_core behind it",
    # the older entries: blocks under names of their own (none packs into S_BLOCK but the two orbl ones), interleaved on one handle by
    # test_one_handle_runs_every_entry_in_any_order in test_gpu_matcher.py
    "orbm_distance_matrix": "S_DM_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_search_by_projection_stereo": "proj_core with two more arrays; in test_gpu_matcher.py's table as window_best chi2 stereo's neighbour",
    "orbm_window_best": "S_WIN_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_window_best_frame": "S_WIN_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_search_for_initialization": "S_INI_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_search_for_initialization_frames": "S_INI_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_search_for_triangulation": "S_TRI_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_search_for_triangulation_frames": "S_TRI_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_search_by_projection_frame": "proj_core on a resident train side; in test_gpu_matcher.py's table",
    "orbm_search_by_bow_frames": "bow_core on resident frames; in test_gpu_matcher.py's table",
    "orbm_undistort_keypoints": "S_UND_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_compute_stereo_from_rgbd": "S_RGBD_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_distinctive_descriptors": "S_DIS_* blocks of its own; in test_gpu_matcher.py's table",
    "orbm_features_in_area": "S_FA_* and G_* blocks of its own; in test_gpu_matcher.py's table",
    "orbl_create_new_map_points": "orbl_core, S_BLOCK: in test_gpu_matcher.py's table; orbl_host.inc is covered here through fuse_batch",
    "orbl_create_new_map_points_frames": "the same orbl_core with resident frames",
}


def _code(path):
    s = open(path).read()
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", s), flags=re.S)


def _headers():
    """include/orbslamm_hip.h and the headers it includes"""
    top = os.path.join(INCLUDE, "orbslamm_hip.h")
    return [top] + [os.path.join(INCLUDE, n) for n in re.findall(r'#include "(orbslamm_\w+\.h)"', open(top).read())]


def _exports():
    """name -> parameter text of every function the headers declare"""
    return {m.group(1): m.group(2) for h in _headers() for m in re.finditer(r"\b(orb[a-z]_\w+)\s*\(([^;{]*?)\)\s*;", _code(h))}


def _covered():
    return {n for c in oh.TABLE for n in c.covers}


def test_every_host_file_that_reserves_the_shared_block_is_in_the_table():
    reserving = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*_host.inc")))
                 if re.search(r"orbm_reserve\(\s*h\s*,\s*S_BLOCK\b|\{\s*S_BLOCK\s*,", _code(p))]
    assert len(reserving) >= 10 and "orbz_host.inc" in reserving and "orbo_host.inc" in reserving, reserving
    missing = [f for f in reserving if f not in _covered()]
    assert not missing, "host files that pack a call into S_BLOCK and are run by no entry of one_handle_cases.TABLE: %s" % missing


def test_the_shared_blocks_comment_lists_its_users():
    """the comment at S_BLOCK in orbm_host.inc names a core of every host file that reserves it"""
    line = [l for l in open(os.path.join(CSRC, "orbm_host.inc")).read().splitlines() if re.match(r"\s*S_BLOCK,", l)]
    assert len(line) == 1
    for core in ("orbl_core", "orbl_fuse_core", "orbc_core", "orbo_core", "orbw_project_sync", "orby_compute_sim3", "orbq_track_pose", "orbq_track_reference",
                 "orbq_relocalize", "orbq_track_motion_model", "orbb_core", "orbz_optimize_sim3"):
        assert core in line[0], core


def test_every_export_that_takes_a_matcher_handle_is_in_the_table_or_has_its_reason():
    exports = _exports()
    takes = sorted(n for n, params in exports.items() if re.search(r"\borbm_t\s*\*", params))
    assert len(takes) >= 45, takes
    covered = _covered()
    unknown = sorted(n for n in covered if not n.endswith(".inc") and n not in exports)
    assert not unknown, "covers= names that no header declares: %s" % unknown
    missing = [n for n in takes if n not in covered and n not in NOT_IN_THE_TABLE]
    assert not missing, "exports that take an orbm_t*, are run by no table entry and have no reason here: %s" % missing
    stale = [n for n in NOT_IN_THE_TABLE if n not in takes or n in covered]
    assert not stale, "reasons for names that are covered, or are no export that takes an orbm_t*: %s" % stale


def test_every_entry_comes_small_and_large():
    for name in oh.NAMES:
        sizes = {c.size for c in oh.of(name)}
        assert {"small", "large"} <= sizes, (name, sizes)
    assert len({oh.key(c) for c in oh.TABLE}) == len(oh.TABLE)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_schedule_holds_every_entry_once_behind_a_larger_call_of_another_family(seed):
    sched = oh.schedule(seed)
    assert 55 <= len(sched) <= 70, len(sched)
    assert [oh.key(c) for c in sched] == [oh.key(c) for c in oh.schedule(seed)], "the same seed, the same schedule"
    for name in oh.NAMES:
        at = [i for i, c in enumerate(sched) if c.name == name]
        assert at, (seed, name, "never runs")
        behind = [i for i in at if i and sched[i - 1].family != sched[i].family and oh.RANK[sched[i - 1].size] > oh.RANK[sched[i].size]]
        assert behind, (seed, name, "never directly follows a larger call of another family")
    assert len({oh.key(c) for c in sched}) > len(oh.TABLE) // 2, "the sizes are drawn, not fixed"


def test_the_schedules_differ():
    assert len({tuple(oh.key(c) for c in oh.schedule(s)) for s in (1, 2, 3)}) == 3


@pytest.mark.parametrize("name", oh.TRACKING)
def test_the_tracking_cases_reach_distinct_verdicts(oracle, name):
    """from the restatements alone: at least one case of each tracking entry per exit the entry has"""
    reached = {c.verdict(oracle) for c in oh.of(name)}
    assert reached == set(oh.VERDICTS[name]), (name, reached)


def test_the_restatements_of_small_and_large_differ(oracle):
    """a case that ends at its early return has little to say: the sizes of an entry give different bytes in the restatement"""
    for name in oh.NAMES:
        refs = [oh.joined(c.ref(oracle)) for c in oh.of(name) if c.ref]
        assert len(set(refs)) == len(refs), name
