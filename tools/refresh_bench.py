"""orbr_refresh_points through the Python mirror against the restatement on one host core: §8u's store of 1 000
keyframes by 2 000 features, 1 600 points a keyframe, about 8 observations a point, with
  one keyframe's points    about 1 600: ProcessNewKeyFrame / CreateNewMapPoints / SearchInNeighbors
  a local map's            about 10 000: the points a local bundle adjustment moved
  every point of the pool  a loop correction or a merge
each for both halves, and for normal and depth alone with new positions (what follows a bundle adjustment); and one synthetic store at
up to 72 observations a point, 64 in its interior (256 keyframes by 512 features, 2 624 points).
  device   KeyFrameStore.refresh_points with the commit and the copy down of `out`
  host     tools/refresh_ref.hpp at g++ -O2 on one core through ONE ctypes call into a buffer made once, its observation index built
           ONCE outside the clock, followed by the orbw_pool_set of the same records (assembled outside the clock) that the host way needs
After 1 s of warm-up the two ways are ALTERNATED repeat by repeat, host clock around each; every output record of both ways is compared
byte for byte before anything is timed.  The median and the 10th .. 90th percentile go to profiles/refresh_bench.json.

    python tools/refresh_bench.py [--repeats 30] [--out profiles/refresh_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_store_scene(cc, rc, rng, nkf, stride, new_per_kf, per_kf, window_kfs):
    """tools/covis_bench.py's scene (keyframe k holds per_kf points of a window of window_kfs keyframes' worth of points around it)
    with descriptors, centres, pool records and the first observer as mpRefKF"""
    npts = (nkf + window_kfs) * new_per_kf
    s = cc.Scene(nkf, stride, npts, rng)
    s.pt_bad[:] = rng.random(npts) < 0.02
    s.kf_flags[:] = cc.KF_SET
    win = window_kfs * new_per_kf
    for k in range(nkf):
        pts = (k * new_per_kf + rng.permutation(win)[:per_kf]).astype(np.int32)
        pts[rng.random(per_kf) < 0.01] |= cc.NO_VOTE
        pos = np.sort(rng.permutation(stride)[:per_kf])
        s.entries[k, pos] = pts
        s.octaves[k, pos] = rng.integers(0, 8, per_kf)
    r = rc.RScene(s, rng)
    for k in range(nkf - 1, -1, -1):                              # mpRefKF: the first keyframe that observes the point
        e = s.entries[k]
        r.ref_kf[e[(e >= 0) & ((e & cc.NO_VOTE) == 0)]] = k
    return r


def load(r, matcher):
    from orbslamm_amd import KeyFrameStore, MapPool
    s = r.s
    pool = MapPool(matcher, s.pool_cap)
    pool.set(np.arange(s.pool_cap), r.pool_records())
    store = KeyFrameStore(pool, s.kfcap, s.stride, 4, 1 << 15)
    recs = s.records()
    for c0 in range(0, s.kfcap, 250):
        store.set(*[x[c0:c0 + 250] for x in recs])
    for k in range(s.kfcap):
        store.set_octaves(k, s.octaves[k])
        store.set_descriptors(k, r.desc[k])
    store.set_centres(np.arange(s.kfcap), r.centres)
    return pool, store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import covis_cases as cc
    import refresh_cases as rc
    from ref_shim import p
    from orbslamm_amd import ORBmatcher
    from orbslamm_amd.map_pool import POINT_DTYPE
    m = ORBmatcher(0.8, True, device=0)

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

    def bench_store(store_name, r, shapes):
        s = r.s
        pool, store = load(r, m)
        shim = rc.shim()
        e = s.entries
        voting = (e >= 0) & ((e & cc.NO_VOTE) == 0)
        obs_per_point = float(np.bincount(e[voting], minlength=s.pool_cap)[np.unique(e[voting])].mean())
        rng = np.random.default_rng(2)
        for shape, ids in shapes(s):
            ids = np.ascontiguousarray(ids, np.int32)
            refkf = np.ascontiguousarray(r.ref_kf[ids])
            moved = np.ascontiguousarray((r.pos[ids] + rng.uniform(-0.05, 0.05, (len(ids), 3))).astype(np.float32))
            for what, pos, label in ((rc.BOTH, None, "both_halves"), (rc.NORMAL_DEPTH, moved, "normal_depth_new_pos")):
                out = np.zeros(len(ids), rc.POINT_DTYPE)
                ref = rc.Ref(r, count_branches=False)             # the scene as the pool holds it now: the commits so far are in it

                def host_ref():
                    shim.rfr_refresh(ref._h, p(ids), p(refkf), p(pos), len(ids), what, p(rc.SF), rc.NLEVELS, p(out), None)

                # both ways' records, byte for byte (NaNs aside: there are none here), before anything is timed or committed
                host_ref()
                got = store.refresh_points(ids, refkf, rc.SF, what, pos, commit=False)
                assert rc.same_records(got, out), (store_name, shape, label)
                assert not np.isnan(out["normal"]).any()
                recs = np.zeros(len(ids), POINT_DTYPE)
                for n in ("pos", "normal", "min_distance", "max_distance", "desc"):
                    recs[n] = out[n]
                recs["flags"] = r.pt_flags()[ids]

                def host():
                    host_ref()
                    pool.set(ids, recs)

                device = lambda: store.refresh_points(ids, refkf, rc.SF, what, pos, commit=True)
                t = run({"host": host, "device": device})
                row = dict(store=store_name, shape=shape, what=label, points=int(len(ids)), keyframes=int(s.kfcap), stride=int(s.stride), pool_points=int(s.pool_cap),
                           observations_per_point=obs_per_point, done_descriptor=int((out["st_descriptor"] == rc.ST_DONE).sum()),
                           done_normal_depth=int((out["st_normal_depth"] == rc.ST_DONE).sum()), repeats=a.repeats, **t)
                print(json.dumps(row), flush=True)
                rows.append(row)
                r.apply(ids, out, pos is not None)                # what both ways have left in the pool
        store.close()
        pool.close()

    def shapes_8u(s):
        one = s.entries[500]
        yield "one_keyframe", np.unique(one[one >= 0] & ~cc.NO_VOTE)
        loc = s.entries[480:521]
        yield "local_map", np.unique(loc[loc >= 0] & ~cc.NO_VOTE)
        yield "whole_pool", np.arange(s.pool_cap, dtype=np.int32)

    bench_store("1000x2000", make_store_scene(cc, rc, np.random.default_rng(1), 1000, 2000, 200, 1600, 9), shapes_8u)
    # 64 observations a point: 256 keyframes by 512 features, each holding 512 of a window of 72 keyframes' worth of 8 points
    bench_store("256x512_64obs", make_store_scene(cc, rc, np.random.default_rng(3), 256, 512, 8, 512, 72),
                lambda s: [("whole_pool", np.arange(s.pool_cap, dtype=np.int32))])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/refresh_bench.py",
                       note="host clock around each way, ways alternated repeat by repeat after 1 s of warm-up; host is tools/refresh_ref.hpp at g++ -O2 on "
                            "one core through one ctypes call into a buffer made once, over flat arrays and an observation index built outside the clock, "
                            "followed by orbw_pool_set of the same records (assembled outside the clock); device is the Python mirror's call with the commit "
                            "and the copy down of out; the kernels' own times are not measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("refresh bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
