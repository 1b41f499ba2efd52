"""Tracking::UpdateLocalMap + SearchLocalPoints' search from the keyframe store against the parent's way: stores
of 200, 2 000 and 8 000 keyframes of stride 2 048 (about 1 100 points each, every point in about ten keyframes), a frame of 1 500
features holding about 1 200 MapPoints, 640 x 480 with 1 000 features to search:
  host_loop_plus_upload   the parent's way: UpdateLocalKeyFrames with the votes cast from per-point observation lists and
                          UpdateLocalPoints over the keyframes' arrays on one host core (tools/localmap_update_ref.hpp at g++ -O2
                          -ffp-contract=off), the points the frame holds taken out of the list, then orbw_track_local_map with that
                          id list (one pinned upload) and orbm_track_results
  store_device            orbu_update_local_map, then orbw_track_local_map_resident and orbm_track_results
  host_loop_only / update_only   the first part of either way alone
kf_set is orbu_kf_set of 20 keyframes: the price of residency, paid when LocalMapping touches a keyframe, not per frame.  After 1 s
of warm-up the ways are ALTERNATED repeat by repeat, host clock around the calls and their results; the median and the 10th .. 90th
percentile go to profiles/localmap_update_bench.json.  Both ways' lists and tables are compared before anything is timed.

    python tools/localmap_update_bench.py [--repeats 30] [--keyframes 200 2000 8000] [--out profiles/localmap_update_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STRIDE, NEW_PER_KF, PER_KF, FILLED = 2048, 110, 1100, 1400


def make_scene(uc, rng, nkf):
    """keyframe k holds PER_KF points of a window of ten keyframes' worth around it, in the first FILLED slots with holes; the ten
    nearest keyframes are its neighbours, k - 1 its parent, k + 1 its child; the frame looks at the middle of the map"""
    npts = nkf * NEW_PER_KF + 10 * NEW_PER_KF
    s = uc.Scene(nkf, STRIDE, 4, npts)
    s.pt_bad[:] = rng.random(npts) < 0.02
    s.kf_flags[:] = uc.KF_SET
    s.kf_flags[rng.random(nkf) < 0.02] |= uc.KF_BAD
    win = 10 * NEW_PER_KF
    for k in range(nkf):
        lo = k * NEW_PER_KF
        pts = (lo + rng.permutation(win)[:PER_KF]).astype(np.int32)
        pts[rng.random(PER_KF) < 0.01] |= uc.NO_VOTE
        s.entries[k, np.sort(rng.permutation(FILLED)[:PER_KF])] = pts
        near = [k + d for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5) if 0 <= k + d < nkf]
        s.neigh[k, :len(near)] = near
        s.parent[k] = k - 1
        if k + 1 < nkf:
            s.set_children(k, [k + 1])
    c = (nkf // 2) * NEW_PER_KF
    ids = (c + rng.integers(0, win + NEW_PER_KF, 1500)).astype(np.int32)
    ids[rng.random(1500) < 0.2] = -1
    s.frame_ids = ids
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[200, 2000, 8000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localmap_update_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import localmap_cases as lc
    import localmap_update_cases as uc
    from ref_shim import p
    from orbslamm_amd import KeyFrameStore, MapPool, ORBextractor, ORBmatcher, level_breaks, make_grid, synth
    w, h, nf = lc.W, lc.H, 1000
    gex = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=3, device=0)
    sf = np.array(gex.GetScaleFactors(), np.float32)
    m = ORBmatcher(0.8, True, device=0)
    gex.extract_batch_device(*gex.upload_frames(synth.make_frames(w, h, 3, stream=31)))
    host = [gex.download(f) for f in range(3)]
    breaks = level_breaks(lc.LOG_SF, lc.NLEVELS)
    view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.01), [0.02, -0.01, 0.03])
    keys = np.concatenate([k for k, _ in host[:2]])
    desc = np.concatenate([d for _, d in host[:2]])
    shim = uc.shim()
    rows = []

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

    for nkf in a.keyframes:
        rng = np.random.default_rng(nkf)
        s = make_scene(uc, rng, nkf)
        max_local = 1 << 15
        # every pool point projects near a feature of the frames: the search behind the update does a search's work
        pick = rng.integers(0, len(keys), s.pool_cap)
        pts = lc.points_from_keys(rng, view, keys[pick], sf, desc[pick])
        pts["flags"] = (pts["flags"] & ~np.uint8(1)) | s.pt_bad
        pool = MapPool(m, s.pool_cap)
        pool.set(np.arange(s.pool_cap), pts)
        fs = m.frame_set(16, gex.max_keypoints, lc.K_A, [0, 0, 0, 0, 0], make_grid(0.0, 0.0, float(w), float(h)), list(lc.BOUNDS), sf)
        fs.build_from_extractor(0, gex)
        store = KeyFrameStore(pool, nkf, STRIDE, 4, max_local)
        recs = s.records()
        for c0 in range(0, nkf, 500):
            store.set(*[r[c0:c0 + 500] for r in recs])
        obs = uc.observations(s)
        st, keep = uc._ref_store(s)
        ids = np.ascontiguousarray(s.frame_ids)
        hdr, votes, lst = np.zeros(16, np.int32), np.zeros(nkf, np.int32), np.zeros(nkf, np.int32)
        cnt, L, seen, S = np.zeros(2, np.int32), np.zeros(max_local, np.int32), np.zeros(max_local, np.uint8), np.zeros(max_local, np.int32)

        def host_loop():
            shim.lmu_keyframes_obs(C.byref(st), p(obs[0]), p(obs[1]), p(ids), len(ids), 80, p(hdr), p(votes), p(lst))
            shim.lmu_points(C.byref(st), p(lst), int(hdr[2]), p(ids), len(ids), max_local, p(cnt), p(L), p(seen), p(S))
            return lst[:hdr[2]], L[:cnt[0]], seen[:cnt[0]], S[:cnt[1]]

        def host_way():
            _, _, _, S_ = host_loop()
            pool.track_local_map(fs, 2, view, S_, 1.0, sf, breaks)
            a_, nm = fs.results()
            return a_, int(nm[0])

        def update_only():
            return store.update(ids, 80)

        def store_way():
            store.update(ids, 80)
            store.track_local_map(fs, 2, view, 1.0, sf, breaks)
            a_, nm = fs.results()
            return a_, int(nm[0])

        # both ways' results, compared before anything is timed
        kf_h, L_h, seen_h, S_h = [x.copy() for x in host_loop()]
        got = update_only()
        assert np.array_equal(got.kf, kf_h) and np.array_equal(got.L, L_h) and np.array_equal(got.seen, seen_h) and got.nS == len(S_h)
        ah, nh = host_way()
        ah = ah.copy()
        ad, nd = store_way()
        assert nh == nd and np.array_equal(ah, ad)
        r = run({"host_loop_plus_upload": host_way, "store_device": store_way, "host_loop_only": host_loop, "update_only": update_only})
        row = dict(what="update_and_search", keyframes=nkf, stride=STRIDE, pool_points=int(s.pool_cap), frame_points=int((ids >= 0).sum()),
                   observers_per_frame_point=float(np.diff(obs[0])[ids[ids >= 0]].mean()), local_keyframes=int(len(kf_h)), nL=int(len(L_h)), nS=int(len(S_h)),
                   nmatches=nh, repeats=a.repeats, upload_bytes=dict(host_loop_plus_upload=int(len(S_h)) * 4 + 96, store_device=len(ids) * 4 + 96), **r)
        print(json.dumps(row), flush=True)
        rows.append(row)
        if nkf == a.keyframes[0]:
            # the price of residency: 20 whole keyframe records
            sub = [r[:20] for r in recs]
            ts = [timed(lambda: store.set(*sub)) for _ in range(a.repeats + 5)][5:]
            row = dict(what="kf_set", keyframes_set=20, stride=STRIDE, repeats=a.repeats, upload_bytes=20 * (16 + 4 + STRIDE) * 4,
                       median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)))
            print(json.dumps(row), flush=True)
            rows.append(row)
        store.close()
        fs.close()
        pool.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/localmap_update_bench.py",
                       note="host clock around each way's calls and results, ways alternated repeat by repeat after 1 s of warm-up; host_loop_* is "
                            "tools/localmap_update_ref.hpp at g++ -O2 -ffp-contract=off on one core through ctypes: flat arrays, the votes cast from "
                            "per-point observation lists, which is cheaper than the reference's walk over heap objects and std::map nodes, but "
                            "it zeroes two pool-sized vectors per call where the reference stamps frame ids; all ways pay the Python mirror's "
                            "argument handling; the kernels' own times are not measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("localmap update bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
