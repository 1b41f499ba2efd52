"""orbn_update_connections and orbn_culling_counts through the Python mirror against the restatement on one host core (DESIGN.md
§8u): a store of 1 000 keyframes by 2 000 features, 1 600 points a keyframe, about 8 observations a point, octaves 0 .. 7, with
  one target       LocalMapping's call
  30 targets       the keyframes a loop correction touches
  1 000 targets    every keyframe of a map, a merge
  device           KeyFrameStore.update_connections / culling_counts: the call, the wait and the copies of every output array
  host             tools/covis_ref.hpp at g++ -O2 through tests/cpp/covis_ref_capi.cpp into buffers made once: flat arrays and an
                   observation index that is built ONCE outside the clock (the reference keeps its observations up to date as it goes)
After 1 s of warm-up the two ways are ALTERNATED repeat by repeat, host clock around each; every output array of both ways is compared
byte for byte before anything is timed.  The median and the 10th .. 90th percentile go to profiles/covis_bench.json.

    python tools/covis_bench.py [--repeats 30] [--out profiles/covis_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NKF, STRIDE, NEW_PER_KF, PER_KF, WINDOW_KFS = 1000, 2000, 200, 1600, 9


def make_scene(cc, rng):
    """keyframe k holds PER_KF points of a window of WINDOW_KFS keyframes' worth of points around it"""
    npts = (NKF + WINDOW_KFS) * NEW_PER_KF
    s = cc.Scene(NKF, STRIDE, npts, rng)
    s.pt_bad[:] = rng.random(npts) < 0.02
    s.kf_flags[:] = cc.KF_SET
    win = WINDOW_KFS * NEW_PER_KF
    for k in range(NKF):
        pts = (k * NEW_PER_KF + rng.permutation(win)[:PER_KF]).astype(np.int32)
        pts[rng.random(PER_KF) < 0.01] |= cc.NO_VOTE
        pos = np.sort(rng.permutation(STRIDE)[:PER_KF])
        s.entries[k, pos] = pts
        s.octaves[k, pos] = rng.integers(0, 8, PER_KF)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import covis_cases as cc
    from ref_shim import p
    from orbslamm_amd import KeyFrameStore, MapPool, ORBmatcher
    from orbslamm_amd.map_pool import POINT_DTYPE, Connections, Culling
    rng = np.random.default_rng(1)
    s = make_scene(cc, rng)
    m = ORBmatcher(0.8, True, device=0)
    pool = MapPool(m, s.pool_cap)
    pts = np.zeros(s.pool_cap, POINT_DTYPE)
    pts["flags"] = s.pt_bad
    pool.set(np.arange(s.pool_cap), pts)
    store = KeyFrameStore(pool, NKF, STRIDE, 4, 1 << 15)
    recs = s.records()
    for c0 in range(0, NKF, 250):
        store.set(*[r[c0:c0 + 250] for r in recs])
    for k in range(NKF):
        store.set_octaves(k, s.octaves[k])
    ref = cc.Ref(s, count_branches=False)
    shim = cc.shim()
    e = s.entries
    voting = (e >= 0) & ((e & cc.NO_VOTE) == 0)
    obs_per_point = float(np.bincount(e[voting], minlength=s.pool_cap)[np.unique(e[voting])].mean())

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def run(ways):
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            for fn in ways.values():
                fn()
        times = {k: [] for k in ways}
        for _ in range(a.repeats):
            for k, fn in ways.items():
                times[k].append(timed(fn))
        q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
        return {k: q(v) for k, v in times.items()}

    rows = []
    for name, K in (("one_target", 1), ("30_targets", 30), ("1000_targets", NKF)):
        tg = np.arange(NKF, dtype=np.int32) if K == NKF else np.sort(rng.permutation(NKF)[:K]).astype(np.int32)
        cap = K * NKF
        ob = {n: np.zeros(K + 1 if n.endswith("start") else (K if n in ("status", "kf_max", "n_max") else cap), np.int32) for n in Connections.NAMES}
        cb = {"n_mps": np.zeros(K, np.int32), "n_redundant": np.zeros(K, np.int32), "redundant": np.zeros(K, np.uint8)}

        def host_conn():
            assert shim.cov_connections(ref._h, p(tg), K, cc.TH, *[p(ob[n]) for n in Connections.NAMES], cap, None) == 0

        def host_cull():
            shim.cov_culling(ref._h, p(tg), K, cc.TH_OBS, p(cb["n_mps"]), p(cb["n_redundant"]), p(cb["redundant"]), None)

        dev_conn = lambda: store.update_connections(tg, cc.TH)
        dev_cull = lambda: store.culling_counts(tg, cc.TH_OBS)
        # both ways' outputs, byte for byte, before anything is timed
        host_conn()
        host_cull()
        gc, gu = dev_conn(), dev_cull()
        for n in Connections.NAMES:
            want = ob[n] if n in ("status", "kf_max", "n_max") or n.endswith("start") else ob[n][:ob[n[:3] + "_start"][-1]]
            assert getattr(gc, n).tobytes() == want.tobytes(), n
        for n in Culling.NAMES:
            assert getattr(gu, n).tobytes() == cb[n].tobytes(), n
        r1 = run({"host": host_conn, "device": dev_conn})
        r2 = run({"host": host_cull, "device": dev_cull})
        for what, r, extra in (("update_connections", r1, dict(connections=int(gc.cnt_start[-1]), ordered=int(gc.ord_start[-1]))),
                               ("culling_counts", r2, dict(redundant=int(gu.redundant.sum()), n_mps_mean=float(gu.n_mps.mean()), n_redundant_mean=float(gu.n_redundant.mean())))):
            row = dict(what=what, shape=name, targets=K, keyframes=NKF, stride=STRIDE, pool_points=int(s.pool_cap), observations_per_point=obs_per_point,
                       repeats=a.repeats, **extra, **r)
            print(json.dumps(row), flush=True)
            rows.append(row)
    store.close()
    pool.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/covis_bench.py",
                       note="host clock around each way, ways alternated repeat by repeat after 1 s of warm-up; host is tools/covis_ref.hpp at g++ -O2 on "
                            "one core through ctypes into buffers made once, over flat arrays and an observation index built outside the clock; the "
                            "reference's own walk goes through heap objects, std::map nodes and mutexes and is expected to cost more than that (an "
                            "expectation, not a measurement); device is the Python mirror's call with the copies of every output array; the kernels' own "
                            "times are not measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("covis bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
