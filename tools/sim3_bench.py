#!/usr/bin/env python3
"""One query's whole Sim3 solve, host call to result: C candidate solvers (1, 4, 16) of N correspondences (20, 100, 500)
each, SetRansacParameters(0.99, 10, 300) (35 iterations at N = 20, 300 from N = 100), 30 % wrong matches.  Device: one
orbs_run over all candidates, then find on each (orbslamm_amd.sim3).  Host: the restatement (tools/sim3_ref.hpp at
g++ -O2, through tests/sim3_cases.py) on one core, find on each candidate -- which stops at its first success -- and,
as a second column, every hypothesis of every candidate (what the device evaluates).  Results are checked equal;
medians go to profiles/sim3_bench.json.  The solvers exist before the clock starts on both sides (the
constructor is not timed); the sets are drawn before it too.

    python tools/sim3_bench.py [--reps 9] [--out profiles/sim3_bench.json]"""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_bench.json"))
    a = ap.parse_args()
    import sim3_cases as sc
    from orbslamm_amd import ORBmatcher
    from orbslamm_amd.sim3 import run_all
    m = ORBmatcher(0.9, True, device=0)
    med = lambda v: float(np.median(v))
    rows = []
    for C in (1, 4, 16):
        for N in (20, 100, 500):
            cases = [sc.family_case("outliers_30", 100 + c, n=N, ransac=(0.99, 10, 300)) for c in range(C)]
            devs = [sc.device_solver(m, case) for case in cases]
            its = devs[0].max_iterations
            sets = [sc.case_sets(case, its, seed=c) for c, case in enumerate(cases)]

            def device_once():
                for d, case in zip(devs, cases):
                    d.set_ransac(*case["ransac"])       # (rewinds mnIterations; mnBestInliers persists as in the reference)
                t0 = time.perf_counter()
                run_all(devs, sets)
                t1 = time.perf_counter()
                out = [d.find() for d in devs]
                return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, out

            def host_once(exhaust):
                refs = [sc.ref_solve(case, sets=s) for case, s in zip(cases, sets)]
                t0 = time.perf_counter()
                out = []
                for r in refs:
                    o = r.find()
                    out.append(o)
                    while exhaust and not o["no_more"]:
                        o = r.find()
                return (time.perf_counter() - t0) * 1e3, out

            # fresh device solvers for the equality check (the timed ones carry mnBestInliers across repetitions)
            fresh = [sc.device_solver(m, case) for case in cases]
            run_all(fresh, sets)
            got = [d.find() for d in fresh]
            _, want = host_once(False)
            for g, w in zip(got, want):
                sc.assert_same_result(g, w, "C %d N %d" % (C, N))
            for d in fresh:
                d.close()
            device_once(); device_once()               # warm-up (allocations, first launches)
            dev, run, legs = [], [], []
            for _ in range(a.reps):
                t, r, _ = device_once()
                dev.append(t); run.append(r); legs.append(devs[0].last_run_ms())
            host_once(False)
            cpu_find = [host_once(False)[0] for _ in range(a.reps)]
            cpu_all = [host_once(True)[0] for _ in range(a.reps)]
            legs = np.median(np.array(legs), axis=0)
            row = dict(candidates=C, n=N, iterations=its, device_ms=med(dev), device_run_ms=med(run), device_min_ms=float(min(dev)),
                       device_max_ms=float(max(dev)), leg_fit_ms=float(legs[0]), leg_host_libm_ms=float(legs[1]), leg_score_ms=float(legs[2]),
                       host_find_ms=med(cpu_find), host_all_hypotheses_ms=med(cpu_all), returned=int(sum(w["returned"] for w in want)),
                       first_return_hypothesis=[int(w["hypothesis"]) for w in want][:4], reps=a.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
            for d in devs:
                d.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/sim3_bench.py", note="medians of --reps runs after warm-up; host = tools/sim3_ref.hpp at g++ -O2 on one core",
                       rows=rows), f, indent=1)
        f.write("\n")
    print("sim3 bench: %d rows equal, written to %s" % (len(rows), a.out))


if __name__ == "__main__":
    main()
