#!/usr/bin/env python3
"""CreateNewMapPoints for one keyframe, host call to result, two ways of doing the same work on device-resident frames
(2000 features per keyframe, 20 neighbours), in one process on one GPU, both through the ctypes mirror:

  (a) the parent's way: per neighbour ComputeF12 on the host, one orbm_search_for_triangulation_frames (its own uploads,
      two launches, a copy down and a synchronise), then the triangulation and the gates of the returned pairs on one host
      core (the restatement tools/newpoints_ref.hpp at g++ -O2), the successes folded into skip1 before the next search;
  (b) the new call: one orbl_create_new_map_points_frames.

Both are warmed, then ALTERNATED keyframe by keyframe over --keyframes keyframes (cycling through --scenes different
scenes); the clock is the host's around calls that return with the device synchronised.  Results are checked equal.  The
medians with their spread (10th / 90th percentile), (a)'s search-only share and the counts go to profiles/newpoints_bench.json
(DESIGN.md §8k).  Per-kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python
tools/newpoints_bench.py --keyframes 40`.

    python tools/newpoints_bench.py [--keyframes 300] [--scenes 4] [--out profiles/newpoints_bench.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=300)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newpoints_bench.json"))
    a = ap.parse_args()
    import newpoints_cases as nc
    from oracle import binding as ob
    from orbslamm_amd import ORBextractor, ORBmatcher, ORBVocabulary, local_mapping as lm, make_grid
    from ref_shim import p as _p
    from vocab_cases import make_vocab
    ob.build()
    m = ORBmatcher(0.6, False, device=0)
    voc = make_vocab(np.random.default_rng(3), 10, 4)
    G = ORBVocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1, device=0)
    g = make_grid(0.0, 0.0, nc.W, nc.H)
    L = nc.ref_lib()
    scenes = []
    for s in range(a.scenes):
        rng = np.random.default_rng(100 + s)
        nb = []
        for _ in range(a.neighbours):
            d = rng.normal(size=3) * np.array([1.0, 0.4, 0.2])
            nb.append((tuple(d / np.linalg.norm(d) * rng.uniform(0.06, 0.3)), float(rng.uniform(0.01, 0.06)), nc.K_A, "true"))
        case = nc.make_case(5000 + s, n=int(a.features * 0.8), nb=nb, depth=(4, 9), noise=0.25, vis=0.35, skip1=0.3, skip2=0.3)
        frames = []
        for side in [case["cur"]] + case["nbs"]:
            dk = gex.upload_frames(np.ascontiguousarray(side["keys"]).view(np.uint8).reshape(1, 1, -1))[0]
            dd = gex.upload_frames(np.ascontiguousarray(side["desc"]).reshape(1, 1, -1))[0]
            F = m.frame_from_device(dk, dd, len(side["keys"]), side["kf"]["K"], [0, 0, 0, 0, 0], g)
            m.frame_compute_bow(F, G, 4)
            frames.append(F)
        scenes.append((case, frames))

    def parents_way(case, frames):
        cur = case["cur"]
        n1 = len(cur["keys"])
        kf1 = np.ascontiguousarray(cur["kf"], dtype=lm.KF_DTYPE)
        skip1 = cur["skip"].copy()
        pts, t_search = [], 0.0
        t0 = time.perf_counter()
        for k, nbs in enumerate(case["nbs"]):
            kf2 = np.ascontiguousarray(nbs["kf"], dtype=lm.KF_DTYPE)
            m12 = None
            if not L.npref_baseline_too_short(_p(kf1), _p(kf2)):
                F, e = lm.compute_f12(kf1, kf2)
                ts = time.perf_counter()
                m12, _ = m.SearchForTriangulationFrames(frames[0], skip1, frames[1 + k], nbs["skip"], F, float(e[0]), float(e[1]), case["sf"], case["sigma2"])
                t_search += time.perf_counter() - ts
            out = np.zeros(n1, dtype=lm.NEWPOINT_DTYPE)
            st = np.zeros(n1, np.uint8)
            n = L.npref_neighbour(k, _p(kf1), _p(kf2), _p(cur["keys"]), n1, _p(nbs["keys"]), _p(m12), _p(skip1), _p(case["sf"]), _p(case["sigma2"]),
                                  len(case["sf"]), C.c_float(case["scale_factor"]), _p(out), _p(st))
            pts.append(out[:n])
        return (time.perf_counter() - t0) * 1e3, t_search * 1e3, np.concatenate(pts)

    def new_call(case, frames):
        cur = dict(frame=frames[0], skip=case["cur"]["skip"], kf=case["cur"]["kf"])
        nbs = [dict(frame=F, skip=nb["skip"], kf=nb["kf"]) for F, nb in zip(frames[1:], case["nbs"])]
        t0 = time.perf_counter()
        pts, _, _ = lm.create_new_map_points(m, cur, nbs, case["sf"], case["sigma2"], case["scale_factor"], want_status=False, want_f12=False)
        return (time.perf_counter() - t0) * 1e3, pts

    counts = []
    for case, frames in scenes:                      # equal results, and the warm-up of both
        _, _, want = parents_way(case, frames)
        _, got = new_call(case, frames)
        assert got.tobytes() == want.tobytes(), "the new call and the parent's way disagree"
        counts.append(len(got))
        for _ in range(3):
            parents_way(case, frames); new_call(case, frames)
    ta, ts, tb = [], [], []
    for i in range(a.keyframes):
        case, frames = scenes[i % len(scenes)]
        t, s, _ = parents_way(case, frames)
        ta.append(t); ts.append(s)
        tb.append(new_call(case, frames)[0])
    q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
    row = dict(features=a.features, neighbours=a.neighbours, keyframes=a.keyframes, scenes=a.scenes, new_points_per_keyframe=counts,
               parents_way=q(ta), parents_way_search_only=q(ts), new_call=q(tb))
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/newpoints_bench.py", note="host clock around synchronising calls, alternated keyframe by keyframe; host = "
                       "tools/newpoints_ref.hpp at g++ -O2 on one core", rows=[row]), f, indent=1)
        f.write("\n")
    print("newpoints bench: equal results, written to %s" % a.out)


if __name__ == "__main__":
    main()
