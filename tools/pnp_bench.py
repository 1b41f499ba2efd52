#!/usr/bin/env python3
"""One frame's relocalisation solve, host call to result: C candidate solvers (1, 4, 16) of N correspondences (20, 100, 500)
each, with Tracking's SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) (35 iterations) and with the constructor's
defaults, at 30 % wrong matches (the first success comes early) and at 60 % (every hypothesis runs: the lost-robot case).
Device: one orbp_run over all candidates, then find on each (orbslamm_amd.pnp).  Host: the restatement
(tools/pnp_ref.hpp at g++ -O2, through tests/pnp_cases.py) on one core, find on each candidate -- which stops at its
first success -- and, as a second column, every hypothesis of every candidate (what the device evaluates).  Results are
checked equal; medians of --reps runs after warm-up, with the spread, go to profiles/pnp_bench.json.  The
solvers exist before the clock starts on both sides (the constructor is not timed); the sets are drawn before it too.

    python tools/pnp_bench.py [--reps 11] [--out profiles/pnp_bench.json]"""
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
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_bench.json"))
    a = ap.parse_args()
    import pnp_cases as pc
    from orbslamm_amd import ORBmatcher
    from orbslamm_amd.pnp import EXTRA_SETS, run_all
    m = ORBmatcher(0.9, True, device=0)
    med = lambda v: float(np.median(v))
    rows = []
    for pname, params in (("tracking", pc.TRACKING), ("defaults", pc.DEFAULTS)):
        for wrong in (0.3, 0.6):
            for C in (1, 4, 16):
                for N in (20, 100, 500):
                    cases = [pc.family_case("wrong_20", 100 + c, n=N, wrong=wrong, ransac=params) for c in range(C)]
                    probe = pc.device_solver(m, cases[0])
                    its = probe.max_iterations
                    probe.close()
                    sets = [pc.case_sets(case, its + EXTRA_SETS, seed=c) for c, case in enumerate(cases)]

                    def device_once():
                        devs = [pc.device_solver(m, case) for case in cases]   # (a table starts at hypothesis 0: fresh solvers)
                        t0 = time.perf_counter()
                        run_all(devs, sets)
                        t1 = time.perf_counter()
                        out = [d.find() for d in devs]
                        t2 = time.perf_counter()
                        legs = devs[0].last_run_ms()
                        for d in devs:
                            d.close()
                        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, legs, out

                    def host_once(exhaust):
                        refs = [pc.ref_solve(case, sets=s) for case, s in zip(cases, sets)]
                        t0 = time.perf_counter()
                        out = []
                        for r in refs:
                            out.append(r.iterate(len(r.sets), stop_on_refine=False) if exhaust else r.find())
                        return (time.perf_counter() - t0) * 1e3, out

                    _, _, _, got = device_once()
                    _, want = host_once(False)
                    for g, w in zip(got, want):
                        pc.assert_same_result(g, w, "%s wrong %.1f C %d N %d" % (pname, wrong, C, N))
                    device_once()                              # warm-up (allocations, first launches)
                    dev, run, legs = [], [], []
                    for _ in range(a.reps):
                        t, r, lg, _ = device_once()
                        dev.append(t); run.append(r); legs.append(lg)
                    host_once(False)
                    cpu_find = [host_once(False)[0] for _ in range(a.reps)]
                    cpu_all = [host_once(True)[0] for _ in range(a.reps)]
                    legs = np.median(np.array(legs), axis=0)
                    row = dict(parameters=pname, wrong=wrong, candidates=C, n=N, iterations=its, device_ms=med(dev), device_min_ms=float(min(dev)),
                               device_max_ms=float(max(dev)), device_run_ms=med(run), leg_chain_host_clock_ms=float(legs[0]), leg_fit_ms=float(legs[1]),
                               leg_score_records_ms=float(legs[2]), leg_refine_ms=float(legs[3]), host_find_ms=med(cpu_find),
                               host_find_min_ms=float(min(cpu_find)), host_find_max_ms=float(max(cpu_find)), host_all_hypotheses_ms=med(cpu_all),
                               returned=int(sum(w["returned"] for w in want)), first_return_hypothesis=[int(w["hypothesis"]) for w in want][:4],
                               reps=a.reps)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/pnp_bench.py", note="medians of --reps runs after warm-up; host = tools/pnp_ref.hpp at g++ -O2 on one core",
                       rows=rows), f, indent=1)
        f.write("\n")
    print("pnp bench: %d rows equal, written to %s" % (len(rows), a.out))


if __name__ == "__main__":
    main()
