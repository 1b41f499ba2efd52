"""The keyframe store's optional columns, mark words and family blocks (orbx_poolutil.inc, DESIGN.md §8q "host side"): what a
store allocates and when, pinned as it is.  One tiny store with every column set; a "round" is every family entry once
(orbu_update_local_map, orbn_update_connections, orbn_culling_counts, orbr_refresh_points, orbe_correct_sim3, nothing
committed).  A second round gives the same bytes and allocates nothing; a round across the generation wrap gives the same bytes
(every family's mark words are cleared there); a second store on the same pool repeats the first one's bytes and its allocation
counts; a store whose families were never called, or only its setters, closes.
A fault, hang or abort met on the GPU is a finding to explain from the code, not to retry."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)
SCW = np.array([0.0, 0.0, 0.0, 1.0, 0.25, -0.5, 0.125, 1.5])   # q (x y z w), t, s
EYE = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (2, 1))
IDS = np.arange(32, dtype=np.int32)
ENTRIES = [np.arange(4, dtype=np.int32), np.arange(2, 6, dtype=np.int32)]   # two keyframes of 4 entries, ids 2 and 3 in both


@pytest.fixture(scope="module")
def matcher(gpu):
    from orbslamm_amd import ORBmatcher
    return ORBmatcher(0.8, True, device=0)


@pytest.fixture(scope="module")
def scene():
    from orbslamm_amd.map_pool import map_points
    rng = np.random.default_rng(5)
    pos = rng.uniform(-2, 2, (32, 3)).astype(np.float32) + np.float32([0, 0, 6])
    nrm = rng.normal(size=(32, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = map_points(pos, nrm, 1.0, 20.0, rng.integers(0, 256, (32, 32), dtype=np.uint8), 0)
    return {"points": pts, "octaves": rng.integers(0, 8, (2, 8), dtype=np.uint8), "desc": rng.integers(0, 256, (2, 8, 32), dtype=np.uint8),
            "centres": rng.uniform(-1, 1, (2, 3)).astype(np.float32), "ref_kf": (IDS % 2).astype(np.int32)}


def alloc_stats(matcher):
    """(device, host) allocations of the matcher's handle so far"""
    from orbslamm_amd._lib import lib
    dev, host = C.c_int64(0), C.c_int64(0)
    assert lib().orbm_alloc_stats(matcher._h, C.byref(dev), C.byref(host), None) == 0
    return np.array([dev.value, host.value])


def make_store(pool, scene, columns=True):
    from orbslamm_amd import KeyFrameStore
    store = KeyFrameStore(pool, 4, 8, 4, 32)
    none = [np.zeros(0, np.int32)] * 2
    store.set([0, 1], [0, 0], ENTRIES, none, [-1, -1], none)
    if columns:
        for k in (0, 1):
            store.set_octaves(k, scene["octaves"][k])
            store.set_descriptors(k, scene["desc"][k])
        store.set_centres([0, 1], scene["centres"])
        store.set_ref_kf(IDS, scene["ref_kf"])
    return store


def a_round(store, scene):
    """every family entry once, nothing committed -> every output's bytes"""
    from orbslamm_amd.map_pool import LOCAL_OK
    out = []
    m = store.update([0, 2, 5])
    assert m.status == LOCAL_OK
    out += [np.array([m.status, m.kf_max, m.nkf, m.nL, m.nS]), m.kf, m.L, m.seen, m.votes]
    conn = store.update_connections([0, 1], th=1)
    out += [getattr(conn, n) for n in conn.NAMES]
    cull = store.culling_counts([0, 1])
    out += [getattr(cull, n) for n in cull.NAMES]
    out.append(store.refresh_points(IDS[:6], scene["ref_kf"][:6], SF, commit=False))
    kf, pts = store.correct_sim3([0, 1], EYE, 0, SCW, SF, commit=False)
    assert len(pts) == 6
    out += [kf, pts]
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_rounds_allocations_the_wrap_and_a_second_store(matcher, scene):
    from orbslamm_amd import MapPool
    pool = MapPool(matcher, 64)
    pool.set(IDS, scene["points"])
    a0 = alloc_stats(matcher)
    store = make_store(pool, scene)
    first = a_round(store, scene)
    a1 = alloc_stats(matcher)
    assert a_round(store, scene) == first                               # (a)
    assert (alloc_stats(matcher) == a1).all(), (a1, alloc_stats(matcher))
    store.debug_set_generation(0xffffffff)                              # (b): the next tag wraps, in orbu_update_local_map
    assert a_round(store, scene) == first
    store.close()
    b0 = alloc_stats(matcher)                                           # (c)
    store = make_store(pool, scene)
    assert a_round(store, scene) == first
    assert (alloc_stats(matcher) - b0 == a1 - a0).all(), (a0, a1, b0, alloc_stats(matcher))
    store.close()
    pool.close()


def test_a_store_closes_before_any_family_entry(matcher, scene):
    from orbslamm_amd import MapPool
    pool = MapPool(matcher, 64)
    pool.set(IDS, scene["points"])
    make_store(pool, scene, columns=False).close()                      # (d): no column, no family block
    make_store(pool, scene).close()                                     # every column, no family block
    store = make_store(pool, scene)                                     # the pool still serves a store after both
    assert len(a_round(store, scene)) > 0
    store.close()
    pool.close()
