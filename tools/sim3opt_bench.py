"""OptimizeSim3 on the device against one host core: the device call (orbz_optimize_sim3: the checks, one packed
upload, ONE launch, one copy down, one synchronise) against the Serial restatement (tools/sim3opt_ref.hpp at g++ -O2
-ffp-contract=off, one core) on the same problems, for 1, 8 and 64 problems a call at 50, 150 and 500 correspondences a problem
(`gross_30` scenes of tests/sim3opt_cases.py: two passes, 10 more iterations after the first check).  Three ways are timed:
  device_mirror   orbslamm_amd.optimize_sim3_batch, packing included (what a Python caller pays)
  device_c_entry  the C entry on arrays packed once (what the C++ drop-in pays after its walk)
  host_serial_one_core  the restatement's Serial mode
after a 1 s warm-up a shape, alternated repeat by repeat, host clock around the synchronising call.  n_in is checked against the
Defined restatement before anything is timed.  The medians with their spread (10th / 90th percentile) go to
profiles/sim3opt_bench.json.  The kernel's own time is NOT measured here: it is what is left of device_c_entry after the copies
and the launch, an inference, unless a run of its own is made under a profiler.

    python tools/sim3opt_bench.py [--repeats 30] [--device-only] [--out profiles/sim3opt_bench.json]"""
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
    ap.add_argument("--problems", default="1,8,64")
    ap.add_argument("--corrs", default="50,150,500")
    ap.add_argument("--family", default="gross_30")
    ap.add_argument("--device-only", action="store_true", help="time only the device entry (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import sim3opt_cases as sc
    from orbslamm_amd import ORBmatcher, optimizer as opt
    from orbslamm_amd._lib import check, lib, ptr
    m = ORBmatcher(0.9, True, device=0)
    L = lib()
    sig = sc.inv_level_sigma2()
    rows = []
    for B in [int(v) for v in a.problems.split(",")]:
        for E in [int(v) for v in a.corrs.split(",")]:
            cases = [sc.make_case(a.family, E, 5000 + i, 0) for i in range(B)]
            items = [dict(c, S12=(c["q"], c["t"], c["s"])) for c in cases]

            def device():
                t0 = time.perf_counter()
                r = opt.optimize_sim3_batch(m, items, sig, sig)
                return (time.perf_counter() - t0) * 1e3, [x["n_in"] for x in r]

            probs = np.concatenate([opt.pack_sim3_problem(it) for it in items])
            corrs = np.concatenate([opt.pack_sim3_corrs(it) for it in items])
            start = (np.arange(B + 1) * E).astype(np.int32)
            out, flags = np.zeros(B, opt.SIM3_RESULT_DTYPE), np.zeros(B * E, np.uint8)
            opt.optimize_sim3_raw(None, None, None, None, None, None)   # (sets the argument types; zero problems return at once)

            def raw():
                t0 = time.perf_counter()
                check(L.orbz_optimize_sim3(m._h, ptr(probs), B, ptr(start), ptr(corrs), ptr(sig), ptr(sig), sig.shape[0], ptr(out), ptr(flags)))
                return (time.perf_counter() - t0) * 1e3, out["n_in"].tolist()

            RL = sc.ref_lib()
            rprobs = np.concatenate([sc.ref_problem(c) for c in cases])
            rcorrs = np.concatenate([sc.ref_corrs(c, sig, sig) for c in cases])
            rout, rflags = np.zeros(B, sc.REF_RESULT), np.zeros(B * E, np.uint8)

            def host():
                t0 = time.perf_counter()
                RL.sim3optref_run(sc.SERIAL, ptr(rprobs), B, ptr(start), ptr(rcorrs), ptr(rout), ptr(rflags), None, None)
                return (time.perf_counter() - t0) * 1e3, rout["n_in"].tolist()

            ways = {"device_mirror": device, "device_c_entry": raw}
            if not a.device_only:
                ways["host_serial_one_core"] = host
            got = {w: fn()[1] for w, fn in ways.items()}
            assert got["device_mirror"] == got["device_c_entry"], "the two device calls disagree"
            defined, _, _, _ = sc.ref_run(sc.DEFINED, cases)
            assert got["device_mirror"] == defined["n_in"].tolist(), "the device disagrees with the Defined restatement"
            t_end = time.perf_counter() + 1.0                      # warm-up: every way, until the clocks have ramped
            while time.perf_counter() < t_end:
                for fn in ways.values():
                    fn()
            times = {w: [] for w in ways}
            for _ in range(a.repeats):
                for w, fn in ways.items():
                    times[w].append(fn()[0])
            q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
            row = dict(problems=B, corrs=E, family=a.family, repeats=a.repeats, n_in=got["device_mirror"][:4],
                       iterations=defined["iterations"][0].tolist(), trials=defined["trials"][0].tolist(), **{w: q(v) for w, v in times.items()})
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/sim3opt_bench.py", library=os.environ.get("ORBSLAMM_HIP_LIB") or "orbslamm_amd/liborbslamm_hip.so",
                       note="host clock around synchronising calls, alternated repeat by repeat; host_serial_one_core is "
                            "tools/sim3opt_ref.hpp (Serial) at g++ -O2 -ffp-contract=off on one core; the kernel's own time is not "
                            "measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("sim3opt bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
