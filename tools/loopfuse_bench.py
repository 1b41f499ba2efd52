#!/usr/bin/env python3
"""SearchAndFuse's searches, host call to hit list, three ways of doing the same work, at two shapes (device-resident frames of
2000 features, 8000 loop points: a loop closure of 60 corrected keyframes, a map merge of 600 of which nine in ten look away
from the loop points), in one process on one GPU, all through the ctypes mirror:

  (a) the parent's per-keyframe way, still in the tree: per target the projection of every point on one host core (the
      restatement tools/loopfuse_ref.hpp at g++ -O2, standing in for ORBmatcherT::Fuse(KF, Scw)'s cv::Mat loop) and one
      orbm_window_best_frame call with that target's resident frame;
  (b) the parent's best batched way: orbl_fuse_batch_frames on the dense job list with inv_level_sigma2 all zero (its
      chi-square gate disabled), in chunks inside its 128-target / 4 194 304-job limits, its 20-byte result per pair
      filtered on the host;
  (c) one orbc_search_and_fuse_frames (and, beside it, the same C entry called with records and result buffers that were
      packed once, which leaves out what the ctypes mirror itself costs per call).

All are warmed, then ALTERNATED repeat by repeat; the clock is the host's around calls that return with the device
synchronised.  The hit lists are checked equal.  The medians with their spread (10th / 90th percentile) go to
profiles/loopfuse_bench.json.  The kernels' own time comes from a run of its own under `rocprofv3
--kernel-trace --stats -- python tools/loopfuse_bench.py --repeats 20 --only-c`; build variants (-DORBC_TILE, -DORBC_LPP) are
compared by loading another build through ORBSLAMM_HIP_LIB (docs/experiments.md).

    python tools/loopfuse_bench.py [--repeats 30] [--only-c] [--shapes loop,merge] [--out profiles/loopfuse_bench.json]"""
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
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--loop-targets", type=int, default=60)
    ap.add_argument("--merge-targets", type=int, default=600)
    ap.add_argument("--shapes", default="loop,merge")
    ap.add_argument("--only-c", action="store_true", help="time only the new entry (kernel A/B, profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loopfuse_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import fuse_cases as fc
    import loopfuse_cases as lc
    from orbslamm_amd import ORBextractor, ORBmatcher, local_mapping as lm, loop_closing as lo, make_grid
    m = ORBmatcher(0.8, False, device=0)
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1, device=0)
    g = make_grid(0.0, 0.0, fc.W, fc.H)
    breaks = lm.level_breaks(fc.LOG_SF, fc.NLEVELS)
    zero_sigma = np.zeros(fc.NLEVELS, np.float32)

    def scene(seed, T, away_share):
        case = lc.make_dense(seed, targets=(T, T), points=(a.points, a.points), feats=a.features)
        rng = np.random.default_rng(seed + 1)
        tg = []
        for t in case["targets"]:
            if rng.uniform() < away_share:      # a keyframe of the merged map that looks elsewhere
                turn = lc.rot_axis_angle([0.1 * rng.normal(), 1.0, 0.1 * rng.normal()], rng.uniform(1.3, np.pi))
                R = turn @ t["rec"]["Rcw"].astype(np.float64)
                O = t["rec"]["Ow"].astype(np.float64)
                t = lc.with_pose(t, R, -R @ O, O)
            tg.append(t)
        case["targets"] = tg
        fr = []
        for t in tg:
            dk = gex.upload_frames(np.ascontiguousarray(t["keys"]).view(np.uint8).reshape(1, 1, -1))[0]
            dd = gex.upload_frames(np.ascontiguousarray(t["desc"]).reshape(1, 1, -1))[0]
            fr.append(dict(rec=t["rec"], frame=m.frame_from_device(dk, dd, len(t["keys"]), t["rec"]["K"], [0, 0, 0, 0, 0], g)))
        return case, fr

    def as_hits(parts):
        """(target, point, best_idx, best_dist) arrays of the pairs with best_idx >= 0 and best_dist <= TH_LOW"""
        out = np.zeros(sum(len(p[1]) for p in parts), dtype=lo.HIT_DTYPE)
        at = 0
        for k, rows, bi, bd in parts:
            out["target"][at:at + len(rows)], out["point"][at:at + len(rows)] = k, rows
            out["best_idx"][at:at + len(rows)], out["best_dist"][at:at + len(rows)] = bi, bd
            at += len(rows)
        return out

    def per_keyframe(case, frames):
        P = len(case["points"])
        t0 = time.perf_counter()
        parts = []
        for k, f in enumerate(frames):
            res, _ = lc.ref_project(case, k)
            rows = np.flatnonzero(res["status"] == lm.FUSE_ST_NO_CANDIDATE)
            if not len(rows):
                continue
            uvr = np.stack([res["u"][rows], res["v"][rows], (np.float32(case["th"]) * case["sf"][res["level"][rows]]).astype(np.float32)], axis=1)
            bi, bd = m.window_best_frame(uvr, res["level"][rows], case["points"]["desc"][rows], None, f["frame"], None, chi2=False)
            keep = (bi >= 0) & (bd <= lo.TH_LOW)
            parts.append((k, rows[keep], bi[keep], bd[keep]))
        hits = as_hits(parts)
        return (time.perf_counter() - t0) * 1e3, hits, P

    def fuse_batch_chunks(case, frames):
        P = len(case["points"])
        per = max(1, min(lm.FUSE_MAX_TARGETS, lm.FUSE_MAX_JOBS // P))
        t0 = time.perf_counter()
        parts = []
        for c0 in range(0, len(frames), per):
            tg = frames[c0:c0 + per]
            js = (np.arange(len(tg) + 1) * P).astype(np.int32)
            jp = np.tile(np.arange(P, dtype=np.int32), len(tg))
            res = lm.fuse_batch(m, tg, case["points"], (js, jp), case["sf"], zero_sigma, breaks, th=case["th"]).reshape(len(tg), P)
            tk, pk = np.nonzero((res["best_idx"] >= 0) & (res["best_dist"] <= lo.TH_LOW))
            parts.append((tk + c0, pk, res["best_idx"][tk, pk], res["best_dist"][tk, pk]))
        hits = as_hits(parts)
        return (time.perf_counter() - t0) * 1e3, hits, P

    def one_call(case, frames):
        t0 = time.perf_counter()
        hits, start, _ = lo.search_and_fuse(m, frames, case["points"], case["sf"], breaks, th=case["th"], capacity=1 << 18)
        return (time.perf_counter() - t0) * 1e3, hits, len(case["points"])

    def raw_entry(case, frames):
        """the same C entry with the records packed and the result buffers made once, as a C++ caller holds them: what the
        ctypes mirror adds per call (packing T records, fresh result arrays) is left out"""
        import ctypes as C
        from orbslamm_amd._lib import check, lib, ptr
        L = lib()
        T, P = len(frames), len(case["points"])
        recs = np.array([t["rec"] for t in frames], dtype=lm.FUSE_TARGET_DTYPE)
        fr = (C.c_void_p * T)(*[t["frame"].value for t in frames])
        hits, start, nh = np.zeros(1 << 18, lo.HIT_DTYPE), np.zeros(T + 1, np.int32), C.c_int(0)
        pts, sf = case["points"], np.ascontiguousarray(case["sf"], np.float32)

        def run():
            t0 = time.perf_counter()
            check(L.orbc_search_and_fuse_frames(m._h, ptr(recs), fr, T, ptr(pts), P, C.c_float(case["th"]), lo.TH_LOW, ptr(sf), len(sf), ptr(breaks),
                                                ptr(hits), len(hits), C.byref(nh), ptr(start), None))
            return (time.perf_counter() - t0) * 1e3, hits[:nh.value], P
        return run

    shapes = {"loop": (7101, a.loop_targets, 0.0), "merge": (7102, a.merge_targets, 0.9)}
    rows = []
    for name in a.shapes.split(","):
        seed, T, away = shapes[name]
        case, frames = scene(seed, T, away)
        ways = {"c_search_and_fuse": lambda: one_call(case, frames), "c_raw_c_entry": raw_entry(case, frames)}
        if not a.only_c:
            ways = dict({"a_per_keyframe": lambda: per_keyframe(case, frames), "b_fuse_batch_chunks": lambda: fuse_batch_chunks(case, frames)}, **ways)
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
        row = dict(shape=name, targets=T, points=a.points, pairs=T * a.points, features=a.features, repeats=a.repeats, hits=int(len(first)),
                   **{w: q(v) for w, v in times.items()})
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/loopfuse_bench.py", library=os.environ.get("ORBSLAMM_HIP_LIB") or "orbslamm_amd/liborbslamm_hip.so",
                       note="host clock around synchronising calls, alternated repeat by repeat; way (a) projects with "
                            "tools/loopfuse_ref.hpp at g++ -O2 on one core; the hit lists of the ways are equal", rows=rows), f, indent=1)
        f.write("\n")
    print("loopfuse bench: equal results, written to %s" % a.out)


if __name__ == "__main__":
    main()
