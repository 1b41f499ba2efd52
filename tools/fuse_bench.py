#!/usr/bin/env python3
"""SearchInNeighbors' searches for one keyframe, host call to result, three ways of doing the same work (25 targets x 2000
points x 2000 features per target, then a second phase of 50 000 candidates into one keyframe), in one process on one GPU,
all through the ctypes mirror:

  (a) the parent's way, still in the tree: per target the projection of every point on one host core (the restatement
      tools/fuse_ref.hpp at g++ -O2, standing in for ORBmatcherT::Fuse's cv::Mat loop) and one orbm_window_best call with
      that target's host arrays (its own uploads, the grid build, a launch, two copies down and a synchronise);
  (b) one orbl_fuse_batch over host arrays;
  (c) one orbl_fuse_batch_frames over device-resident frames.

All are warmed, then ALTERNATED repeat by repeat; the clock is the host's around calls that return with the device
synchronised.  Results are checked equal.  The medians with their spread (10th / 90th percentile) go to
profiles/fuse_bench.json.  The kernel's own time comes from a run of its own under `rocprofv3 --kernel-trace
--stats -- python tools/fuse_bench.py --repeats 40 --batch-only`; build variants (-DORBL_FUSE_LPP, -DORBL_FUSE_STAGE_CELLS)
are compared by loading another build through ORBSLAMM_HIP_LIB (docs/experiments.md).

    python tools/fuse_bench.py [--repeats 60] [--batch-only] [--out profiles/fuse_bench.json]"""
import argparse
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
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--targets", type=int, default=25)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--candidates", type=int, default=50000)
    ap.add_argument("--batch-only", action="store_true", help="time only the two batch entries (kernel A/B, profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import fuse_cases as fc
    from orbslamm_amd import ORBextractor, ORBmatcher, local_mapping as lm, make_grid
    from orbslamm_amd._lib import OrbmGrid
    m = ORBmatcher(0.6, False, device=0)
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1, device=0)
    g = make_grid(0.0, 0.0, fc.W, fc.H)
    breaks = lm.level_breaks(fc.LOG_SF, fc.NLEVELS)
    phases = {
        "phase1": fc.make_case(7001, targets=(a.targets, a.targets), points=(a.points, a.points), feats=a.features, all_points=True),
        "phase2": fc.make_case(7002, targets=(1, 1), points=(a.candidates, a.candidates), feats=a.features, pix_noise=0.4, all_points=True),
    }
    frames = {}
    for name, case in phases.items():
        tg = []
        for t in case["targets"]:
            dk = gex.upload_frames(np.ascontiguousarray(t["keys"]).view(np.uint8).reshape(1, 1, -1))[0]
            dd = gex.upload_frames(np.ascontiguousarray(t["desc"]).reshape(1, 1, -1))[0]
            tg.append(dict(rec=t["rec"], frame=m.frame_from_device(dk, dd, len(t["keys"]), t["rec"]["K"], [0, 0, 0, 0, 0], g)))
        frames[name] = tg

    def parents_way(case):
        js, jp = case["jobs"]
        out = np.zeros(int(js[-1]), dtype=lm.FUSE_RESULT_DTYPE)
        t0 = time.perf_counter()
        for k, t in enumerate(case["targets"]):
            idx = jp[js[k]:js[k + 1]]
            res, _ = fc.ref_project(case, k, idx)
            rows, uvr, pred, qd = fc.window_queries(case, res, idx)
            if len(rows):
                bi, bd = m.window_best(uvr, pred, qd, None, g, t["keys"], t["desc"], case["inv_sigma2"], chi2=True)
                res["best_idx"][rows], res["best_dist"][rows] = bi, bd
                res["status"][rows] = np.where(bi >= 0, lm.FUSE_ST_FOUND, lm.FUSE_ST_NO_CANDIDATE)
            out[js[k]:js[k + 1]] = res
        return (time.perf_counter() - t0) * 1e3, out

    def batch(case, targets):
        t0 = time.perf_counter()
        out = lm.fuse_batch(m, targets, case["points"], case["jobs"], case["sf"], case["inv_sigma2"], breaks, th=case["th"])
        return (time.perf_counter() - t0) * 1e3, out

    rows = []
    for name, case in phases.items():
        ways = {"batch_host_arrays": lambda c=case: batch(c, c["targets"]), "batch_frames": lambda c=case, n=name: batch(c, frames[n])}
        if not a.batch_only:
            ways = dict({"parents_way": lambda c=case: parents_way(c)}, **ways)
        outs = {w: fn()[1] for w, fn in ways.items()}            # equal results
        first = next(iter(outs.values()))
        assert all(o.tobytes() == first.tobytes() for o in outs.values()), "the ways disagree"
        t_end = time.perf_counter() + 2.0                         # warm-up: every way, until the clocks have ramped
        while time.perf_counter() < t_end:
            for fn in ways.values():
                fn()
        times = {w: [] for w in ways}
        for _ in range(a.repeats):
            for w, fn in ways.items():
                times[w].append(fn()[0])
        q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
        row = dict(phase=name, targets=len(case["targets"]), pairs=int(case["jobs"][0][-1]), features=a.features, repeats=a.repeats,
                   found=int((first["status"] == lm.FUSE_ST_FOUND).sum()), **{w: q(v) for w, v in times.items()})
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/fuse_bench.py", library=os.environ.get("ORBSLAMM_HIP_LIB") or "orbslamm_amd/liborbslamm_hip.so",
                       note="host clock around synchronising calls, alternated repeat by repeat; the parent's way projects with "
                            "tools/fuse_ref.hpp at g++ -O2 on one core", rows=rows), f, indent=1)
        f.write("\n")
    print("fuse bench: equal results, written to %s" % a.out)


if __name__ == "__main__":
    main()
