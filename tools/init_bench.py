#!/usr/bin/env python3
"""One Initialize call, host to result, on the device (orbi_initialize) and in the restatement on one host core
(tools/init_ref.hpp at g++ -O2, through tests/init_cases.py), for both models, over 1 000 / 2 000 / 4 000 keys per frame
and 100 / 500 / 2 000 matches (30 % outliers, noise 0.5 px, 200 iterations).  Results are checked equal; medians go
to profiles/init_bench.json.

    python tools/init_bench.py [--reps 9] [--out profiles/init_bench.json]"""
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
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_bench.json"))
    a = ap.parse_args()
    import init_cases as ic
    from orbslamm_amd import ORBmatcher, _lib
    from orbslamm_amd.initializer import Initializer, make_sets
    m = ORBmatcher(0.9, True, device=0)
    rows = []
    for nkeys in (1000, 2000, 4000):
        for nmatch in (100, 500, 2000):
            if nmatch > nkeys:
                continue
            rng = np.random.default_rng(nkeys + nmatch)
            keys1, keys2, m12, _, _ = ic.make_scene(rng, n_match=nmatch, n1=nkeys, n2=nkeys, noise=0.5, outliers=0.3)
            sets = make_sets(int((m12 >= 0).sum()), 200)
            for model in ("HF", "F"):
                ini = Initializer(m, keys1, ic.K_TUM, iterations=200, model=model)
                ini.initialize(keys2, m12, sets)   # warm-up (allocations, first launches)
                dev = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    got = ini.initialize(keys2, m12, sets)
                    dev.append((time.perf_counter() - t0) * 1e3)
                cpu = []
                for _ in range(a.cpu_reps):
                    t0 = time.perf_counter()
                    want = ic.ref_initialize(keys1, keys2, m12, sets, model=model)
                    cpu.append((time.perf_counter() - t0) * 1e3)
                ic.assert_equal_results(got, want)
                ini.close()
                row = dict(keys=nkeys, matches=nmatch, model=model, device_ms=round(float(np.median(dev)), 3),
                           cpu_ms=round(float(np.median(cpu)), 3), ok=bool(want["ok"]), reconstructed_h=int(want["res"]["reconstructed_h"]))
                row["speedup"] = round(row["cpu_ms"] / row["device_ms"], 2)
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = dict(what="one Initialize call, host to result: device (orbi_initialize) vs the restatement on one host core (g++ -O2)",
               iterations=200, outliers=0.3, noise_px=0.5, reps=a.reps, cpu_reps=a.cpu_reps,
               device=_lib.device_pci_bus_id(0), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
