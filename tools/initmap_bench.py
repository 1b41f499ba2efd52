#!/usr/bin/env python3
"""The initial map, host call to results: the device entry through the ctypes mirror (orbb_initial_map on host arrays: one
upload, ONE launch, one copy down, one synchronise) against the Serial restatement (tools/initmap_ref.hpp at g++ -O2
-ffp-contract=off) on one host core over the same inputs, for 1 problem and batches of 8 and 64 at 100 / 300 / 1 000 / 2 000
points a problem (`noisy` scenes of tests/initmap_cases.py: the first pose fixed, 20 iterations allowed, the Huber kernel on).

Both are warmed, then ALTERNATED repeat by repeat; the clock is the host's around calls that return with the device
synchronised.  The verdict and the point count of the two sides are checked equal, and the device's bytes against the Defined
restatement.  The medians with their spread (10th / 90th percentile) and who wins go to profiles/initmap_bench.json (DESIGN.md
§8aa): one problem is one wave, so a single map is expected to LOSE to a host core, as a single frame does in §8o -- the
losses are recorded, not hidden.  The kernel's own time comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/initmap_bench.py --repeats 20 --device-only`.

    python tools/initmap_bench.py [--repeats 20] [--device-only] [--out profiles/initmap_bench.json]"""
import argparse
import importlib
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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--problems", default="1,8,64")
    ap.add_argument("--points", default="100,300,1000,2000")
    ap.add_argument("--family", default="noisy")
    ap.add_argument("--device-only", action="store_true", help="time only the device entry (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initmap_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import initmap_cases as ic
    from orbslamm_amd import ORBmatcher
    im = importlib.import_module("orbslamm_amd.initial_map")
    m = ORBmatcher(0.9, True, device=0)
    sig, sf = ic.inv_level_sigma2(a.family), ic.scale_factors()
    rows = []
    for B in [int(v) for v in a.problems.split(",")]:
        for N in [int(v) for v in a.points.split(",")]:
            cases = [ic.make_case(a.family, N, 5000 + i) for i in range(B)]
            problems = np.zeros(B, dtype=im.PROBLEM_DTYPE)
            for i, c in enumerate(cases):
                problems[i] = im.pack_problem(c)
            k1, k2 = [c["keys_un1"] for c in cases], [c["keys_un2"] for c in cases]
            m12, p3d = [c["matches12"] for c in cases], [c["P3D"] for c in cases]

            def device():
                t0 = time.perf_counter()
                rc, out, pts = im.initial_map_raw(m._h, problems, k1, k2, None, None, m12, p3d, sig, sf)
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0
                return dt, out, pts

            def host():
                t0 = time.perf_counter()
                res = [ic.ref_run(c, ic.SERIAL, sig, sf) for c in cases]
                return (time.perf_counter() - t0) * 1e3, res

            ways = {"device_mirror": device}
            if not a.device_only:
                ways["host_serial_one_core"] = host
            _, out, pts = device()
            defined = [ic.ref_run(c, ic.DEFINED, sig, sf) for c in cases]
            for i in range(B):
                assert out[i:i + 1].tobytes() == defined[i][0].tobytes() and pts[i].tobytes() == defined[i][1].tobytes(), "the device disagrees with the Defined restatement"
            if not a.device_only:
                serial = host()[1]
                assert [int(r[0]["verdict"]) for r in serial] == out["verdict"].tolist() and [int(r[0]["n_points"]) for r in serial] == out["n_points"].tolist()
            t_end = time.perf_counter() + 1.0                      # warm-up: every way, until the clocks have ramped
            while time.perf_counter() < t_end:
                for fn in ways.values():
                    fn()
            times = {w: [] for w in ways}
            for _ in range(a.repeats):
                for w, fn in ways.items():
                    times[w].append(fn()[0])
            q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
            row = dict(problems=B, points=N, family=a.family, repeats=a.repeats, verdicts=out["verdict"].tolist()[:4],
                       iterations=out["iterations"].tolist()[:4], trials=out["trials"].tolist()[:4], **{w: q(v) for w, v in times.items()})
            if not a.device_only:
                row["device_over_host"] = row["device_mirror"]["median_ms"] / row["host_serial_one_core"]["median_ms"]
                row["device_loses"] = bool(row["device_over_host"] > 1.0)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/initmap_bench.py", library=os.environ.get("ORBSLAMM_HIP_LIB") or "orbslamm_amd/liborbslamm_hip.so",
                       note="host clock around synchronising calls, alternated repeat by repeat; host_serial_one_core is "
                            "tools/initmap_ref.hpp (Serial) at g++ -O2 on one core, called once per problem through ctypes; "
                            "device_over_host above 1 is a loss of the device", rows=rows), f, indent=1)
        f.write("\n")
    print("initmap bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
