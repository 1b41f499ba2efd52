"""Tracking's two projection searches from the map-point pool against the parent's way, 3 000 local points at
1241 x 376 with 2 000 features, th = 1 and 3:
  host_loop_plus_upload   the parent's way: Frame::isInFrustum + the head of SearchByProjection over the list on one host core
                          (tools/frustum_ref.hpp at g++ -O2 -ffp-contract=off), the descriptor gather, then
                          orbm_track_local_points (one pinned upload, two launches) and orbm_track_results
  pool_device             orbw_track_local_map (ids + one view record up, k_view_project, the same two launches) and
                          orbm_track_results
and the same pair for the frame/frame search (ORBmatcher.cc:1353-1392 on the host + orbm_track_frame_projected against
orbw_track_frame_pose).  host_loop_only is the first way's host part alone: what of a gain is the loop and what the upload.
pool_set is orbw_pool_set of the 3 000 records: the price of residency, paid when LocalMapping touches the points, not per
frame.  After 1 s of warm-up the ways are ALTERNATED repeat by repeat, host clock around the call and its results; the median
and the 10th .. 90th percentile go to profiles/localmap_bench.json with the bytes either way sends up.  Both ways' tables are
compared before anything is timed.

    python tools/localmap_bench.py [--repeats 30] [--out profiles/localmap_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KITTI_K = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localmap_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import localmap_cases as lc
    from orbslamm_amd import MapPool, ORBextractor, ORBmatcher, level_breaks, make_grid, synth
    w, h, nf = 1241, 376, 2000
    bounds = (0.0, float(w), 0.0, float(h))
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=3, device=0)
    sf = np.array(gex.GetScaleFactors(), np.float32)
    m = ORBmatcher(0.8, True, device=0)
    fs = m.frame_set(4, gex.max_keypoints, KITTI_K, [0, 0, 0, 0, 0], make_grid(0.0, 0.0, float(w), float(h)), list(bounds), sf)
    gex.extract_batch_device(*gex.upload_frames(synth.make_frames(w, h, 3, stream=31)))
    fs.build_from_extractor(0, gex)
    host = [gex.download(f) for f in range(3)]
    breaks = level_breaks(lc.LOG_SF, lc.NLEVELS)
    rng = np.random.default_rng(11)
    view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.01), [0.02, -0.01, 0.03], K=KITTI_K, bounds=bounds)
    keys = np.concatenate([k for k, _ in host[:2]])
    desc = np.concatenate([d for _, d in host[:2]])
    pick = rng.permutation(len(keys))[:a.points]
    pts = lc.points_from_keys(rng, view, keys[pick], sf, desc[pick])
    n = len(pts)
    ids = rng.permutation(n).astype(np.int32)
    pool = MapPool(m, 1 << 16)
    slots = rng.permutation(1 << 16)[:n].astype(np.int32)
    pool.set(slots, pts)
    pool_ids = slots[ids]
    # the frame/frame pair: LastFrame = slot 0, CurrentFrame = slot 1
    kl, dl = host[0]
    fpts = lc.points_from_keys(rng, view, kl, sf, dl, jitter=1.5)
    fpool_slots = rng.permutation(1 << 16)[:len(kl)].astype(np.int32)
    fpool = MapPool(m, 1 << 16)
    fpool.set(fpool_slots, fpts)
    feat = np.where(rng.random(len(kl)) < 0.85, np.arange(len(kl)), -1).astype(np.int32)
    last_ids = np.where(feat >= 0, fpool_slots[np.maximum(feat, 0)], -1).astype(np.int32)
    octs = kl["octave"].astype(np.int32)
    rows = []

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def run(name, ways, check):
        got = {k: fn() for k, fn in ways.items()}
        check(got)
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            for fn in ways.values():
                fn()
        times = {k: [] for k in ways}
        for _ in range(a.repeats):
            for k, fn in ways.items():
                times[k].append(timed(fn)[0])
        q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
        return {k: q(v) for k, v in times.items()}

    for th in (1.0, 3.0):
        def host_loop():
            ref = lc.ref_local(view, pts, ids, th, sf)
            return ref, np.ascontiguousarray(pts["desc"][ids])

        def host_way():
            ref, qd = host_loop()
            fs.track_local_points(2, ref["uvr"], ref["lvl"], qd, ref["valid"], ref["obs"])
            a_, nm = fs.results()
            return a_.copy(), int(nm[0])

        def pool_way():
            pool.track_local_map(fs, 2, view, pool_ids, th, sf, breaks)
            a_, nm = fs.results()
            return a_.copy(), int(nm[0])

        def same(got):
            assert got["host_loop_plus_upload"][1] == got["pool_device"][1] and np.array_equal(got["host_loop_plus_upload"][0], got["pool_device"][0])

        ways = {"host_loop_plus_upload": host_way, "pool_device": pool_way, "host_loop_only": host_loop}
        r = run("local_map", ways, same)
        row = dict(search="local_map", th=th, points=n, features=int(len(host[2][0])), nmatches=host_way()[1], repeats=a.repeats,
                   upload_bytes=dict(host_loop_plus_upload=n * (12 + 2 + 32 + 1 + 1), pool_device=n * 4 + 96), **r)
        print(json.dumps(row), flush=True)
        rows.append(row)
    for th in (15.0, 7.0):
        def fhost_loop():
            return lc.ref_frame(view, fpts, feat, octs, th, sf)

        def fhost_way():
            ref = fhost_loop()
            fs.track_projected(1, 0, ref["uvr"], ref["lvl"], ref["valid"], ref["obs"], nnratio=0.9, check_ori=True, mode=4)
            a_, nm = fs.results()
            return a_.copy(), int(nm[0])

        def fpool_way():
            fpool.track_frame_pose(fs, 1, 0, view, last_ids, th, sf, nnratio=0.9, check_ori=True, mode=4)
            a_, nm = fs.results()
            return a_.copy(), int(nm[0])

        def fsame(got):
            assert got["host_loop_plus_upload"][1] == got["pool_device"][1] and np.array_equal(got["host_loop_plus_upload"][0], got["pool_device"][0])

        r = run("frame_frame", {"host_loop_plus_upload": fhost_way, "pool_device": fpool_way, "host_loop_only": fhost_loop}, fsame)
        nl = len(kl)
        row = dict(search="frame_frame", th=th, points=nl, features=int(len(host[1][0])), nmatches=fhost_way()[1], repeats=a.repeats,
                   upload_bytes=dict(host_loop_plus_upload=nl * (12 + 2 + 1 + 1), pool_device=nl * 4 + 96), **r)
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the price of residency
    ts = []
    for _ in range(a.repeats + 5):
        ts.append(timed(lambda: pool.set(slots, pts))[0])
    ts = ts[5:]
    set_row = dict(search="pool_set", points=n, repeats=a.repeats, upload_bytes=n * 80, median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)),
                   p90_ms=float(np.percentile(ts, 90)))
    print(json.dumps(set_row), flush=True)
    rows.append(set_row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/localmap_bench.py",
                       note="host clock around each call and its results (orbm_track_results), ways alternated repeat by repeat after 1 s of "
                            "warm-up; host_loop_* is tools/frustum_ref.hpp at g++ -O2 -ffp-contract=off on one core, called through ctypes with the "
                            "descriptor gather in numpy; all ways pay the Python mirror's argument handling; the kernels' own times are not "
                            "measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("localmap bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
