#!/usr/bin/env python3
"""PoseOptimization, host call to results: the device entry through the ctypes mirror (orbo_pose_optimize on host arrays: one
upload, ONE launch, one copy down, one synchronise) against the Serial restatement (tools/poseopt_ref.hpp at g++ -O2
-ffp-contract=off) on one host core over the same inputs, for 1 frame and batches of 8 and 64 frames at 100 / 300 / 2000
edges a frame (`gross_30` scenes of tests/poseopt_cases.py: four full rounds, a third of the edges dropped after the first).

Both are warmed, then ALTERNATED repeat by repeat; the clock is the host's around calls that return with the device
synchronised.  Beside the mirror's call the same C entry is timed with its arguments packed once, as a C++ caller holds
them (what the mirror itself costs per call is left out).  The integer outputs of the two sides are checked equal where the
restatement's two modes agree (tests/poseopt_cases.py says why they need not).  The medians with their spread (10th / 90th
percentile) go to profiles/poseopt_bench.json.  The kernel's own time comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/poseopt_bench.py --repeats 20 --device-only`.

    python tools/poseopt_bench.py [--repeats 30] [--device-only] [--out profiles/poseopt_bench.json]"""
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
    ap.add_argument("--frames", default="1,8,64")
    ap.add_argument("--edges", default="100,300,2000")
    ap.add_argument("--family", default="gross_30")
    ap.add_argument("--device-only", action="store_true", help="time only the device entry (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseopt_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import poseopt_cases as pc
    from orbslamm_amd import ORBmatcher, optimizer as opt
    from orbslamm_amd._lib import check, lib, ptr
    m = ORBmatcher(0.9, True, device=0)
    L = lib()
    sig = pc.inv_level_sigma2()
    rows = []
    for B in [int(v) for v in a.frames.split(",")]:
        for E in [int(v) for v in a.edges.split(",")]:
            cases = [pc.make_case(a.family, E, 5000 + i) for i in range(B)]
            items = [dict(Tcw=c["Tcw"], K=c["K"], keys_un=c["keys_un"], feature=c["feature"], Xw=c["Xw"]) for c in cases]

            def device():
                t0 = time.perf_counter()
                r = opt.pose_optimization_batch(m, items, sig)
                return (time.perf_counter() - t0) * 1e3, [x["n_good"] for x in r]

            import ctypes as C
            frames = np.zeros(B, dtype=opt.FRAME_DTYPE)
            for i, c in enumerate(cases):
                frames["Tcw"][i], frames["K"][i] = c["Tcw"].reshape(16), c["K"]
            start = (np.arange(B + 1) * E).astype(np.int32)
            edges = np.concatenate([opt.pack_edges(c["feature"], c["Xw"]) for c in cases])
            keys = [np.ascontiguousarray(c["keys_un"]) for c in cases]
            kp = (C.c_void_p * B)(*[ptr(k) for k in keys])
            nk = np.array([k.shape[0] for k in keys], dtype=np.int32)
            out, flags = np.zeros(B, opt.RESULT_DTYPE), np.zeros(B * E, np.uint8)

            def raw():
                t0 = time.perf_counter()
                check(L.orbo_pose_optimize(m._h, ptr(frames), kp, ptr(nk), B, ptr(start), ptr(edges), ptr(sig), sig.shape[0], ptr(out), ptr(flags)))
                return (time.perf_counter() - t0) * 1e3, out["n_good"].tolist()

            RL = pc.ref_lib()
            rframes = np.zeros(B, dtype=pc.REF_FRAME)
            rframes["Tcw"], rframes["K"] = frames["Tcw"], frames["K"]
            redges = np.concatenate([pc.ref_edges(c, sig) for c in cases])
            rout, rflags = np.zeros(B, pc.REF_RESULT), np.zeros(B * E, np.uint8)

            def host():
                t0 = time.perf_counter()
                RL.poseoptref_run(pc.SERIAL, ptr(rframes), B, ptr(start), ptr(redges), ptr(rout), ptr(rflags), None, None)
                return (time.perf_counter() - t0) * 1e3, rout["n_good"].tolist()

            ways = {"device_mirror": device, "device_c_entry": raw}
            if not a.device_only:
                ways["host_serial_one_core"] = host
            good = {w: fn()[1] for w, fn in ways.items()}
            assert good["device_mirror"] == good["device_c_entry"], "the two device calls disagree"
            defined, _, _, _ = pc.ref_run(pc.DEFINED, cases)
            assert good["device_mirror"] == defined["n_good"].tolist(), "the device disagrees with the Defined restatement"
            t_end = time.perf_counter() + 1.0                      # warm-up: every way, until the clocks have ramped
            while time.perf_counter() < t_end:
                for fn in ways.values():
                    fn()
            times = {w: [] for w in ways}
            for _ in range(a.repeats):
                for w, fn in ways.items():
                    times[w].append(fn()[0])
            q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
            row = dict(frames=B, edges=E, family=a.family, repeats=a.repeats, n_good=good["device_mirror"][:4],
                       iterations=defined["iterations"][0].tolist(), trials=defined["trials"][0].tolist(), **{w: q(v) for w, v in times.items()})
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/poseopt_bench.py", library=os.environ.get("ORBSLAMM_HIP_LIB") or "orbslamm_amd/liborbslamm_hip.so",
                       note="host clock around synchronising calls, alternated repeat by repeat; host_serial_one_core is "
                            "tools/poseopt_ref.hpp (Serial) at g++ -O2 on one core", rows=rows), f, indent=1)
        f.write("\n")
    print("poseopt bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
