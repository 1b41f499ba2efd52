"""Tracking::TrackWithMotionModel from the predicted pose to the counts in one call (orbq_track_motion_model) against the
parent's way: 1, 8 and 64 jobs a call, frame pairs of 2 000 features on a 1241 x 376 image, each with and without the retry.
  chain_host      the parent's way as ONE C entry (tests/cpp/motionmodel_bench_capi.cpp, g++ -O2): per job the host pose product and view
                  record, orbw_track_frame_pose + orbm_track_results (the wait that lets the host compare nmatches with 20), both again
                  with 2 * th below 20, then ONE orbq_track_pose over the jobs that passed the gate
  motion_device   ONE orbq_track_motion_model
The jobs are scenes of tests/motionmodel_cases.py at that size (four seeds in turn), each pair in a frame set of its own; the pool holds
every scene's points.  Without the retry a scene has 1 000 points where they are seen; with it 10, and 990 that only 2 * th finds.  Both
ways' outputs -- records, ids, outlier bytes, tables, counts -- are compared byte for byte with each other, and job 0 with the restatement
(tools/motionmodel_ref.hpp), before anything is timed.  After 1 s of warm-up the ways are ALTERNATED repeat by repeat, host clock around
one ctypes call either way (every array and pointer made once, outside the timed functions); the median and the 10th .. 90th percentile
go to profiles/motionmodel_bench.json.

    python tools/motionmodel_bench.py [--repeats 30] [--jobs 1 8 64] [--out profiles/motionmodel_bench.json]"""
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

SCENES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motionmodel_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import localmap_cases as lc
    import motionmodel_cases as mc
    from ref_shim import build_ref_shim
    from orbslamm_amd import make_grid
    from orbslamm_amd._lib import lib, table
    from orbslamm_amd.track_pose import MOTION_RESULT_DTYPE, TRACK_RESULT_DTYPE, pack_motion_jobs
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    raw = lambda h: h.value if isinstance(h, vp) else int(h)

    class ParentWay(C.Structure):   # tests/cpp/motionmodel_bench_capi.cpp
        _fields_ = ([(k, vp) for k in ("trackFramePose", "trackResults", "trackPose", "h", "pool")] + [(k, i32) for k in ("J", "n", "nq", "nlevels", "minMatches")] +
                    [("th", C.c_float)] + [(k, vp) for k in ("fs", "lastIds", "velocity", "lastTcw", "K", "bounds", "sig", "sf", "tjobs", "tout", "idsPtr", "outlPtr",
                                                              "which", "TcwPred", "nSearch", "wide", "status", "out", "idsOut", "outlierOut", "assignOut")])
    bshim = build_ref_shim("motionmodel_bench")
    assert bshim.motionbench_sizeof() == C.sizeof(ParentWay) and bshim.motionbench_sizeof_res() == TRACK_RESULT_DTYPE.itemsize
    bshim.motionbench_parent_way.argtypes = [vp]
    rig = mc.Rig()
    N = mc.BIG_N
    nmax = max(a.jobs)
    grid = make_grid(0.0, 0.0, float(mc.BIG_W), float(mc.BIG_H))
    bounds = np.array([0.0, mc.BIG_W, 0.0, mc.BIG_H], np.float32)
    sig, sf, K = mc.sigma2(), np.ascontiguousarray(lc.SF, np.float32), np.ascontiguousarray(mc.BIG_K, np.float32)
    fn = lambda name: C.cast(getattr(L, name), vp).value
    sets = [rig.m.frame_set(2, N, mc.BIG_K, mc.rc.D0, grid, list(bounds), lc.SF) for _ in range(nmax)]
    rows = []
    for retry in (False, True):
        scenes, base = [], 0
        for k in range(SCENES):
            c = mc.big_case(seed=11 + k, true=10 if retry else 1000, far=990 if retry else 0)
            c["own_ids"] = c["last_ids"].copy()
            c["last_ids"] = np.where(c["last_ids"] >= 0, c["last_ids"] + base, -1).astype(np.int32)
            base += len(c["pool"])
            scenes.append(c)
        records = np.concatenate([c["pool"] for c in scenes])
        pool = mc.new_pool(rig, records)
        for j in range(nmax):
            rig.put_case(sets[j], 0, 1, scenes[j % SCENES])
        ref = mc.ref_run(dict(scenes[0], last_ids=scenes[0]["own_ids"]))
        for nj in a.jobs:
            jobs = [mc.job(sets[j], 0, 1, scenes[j % SCENES]) for j in range(nj)]
            got = mc.call(rig, pool, jobs)
            assert got[0] == 0
            mc.assert_job_equals_ref(got, 0, ref, ("bench", retry, nj))   # (scene 0's ids carry no shift)
            assert all(int(w) == int(retry) for w in got[1]["wide"]) and (got[1]["status"] == mc.TRACKED).all()
            # ---- the device way's arrays
            rec, keep = pack_motion_jobs(jobs)
            out = np.zeros(nj, MOTION_RESULT_DTYPE)
            ids = [np.zeros(N, np.int32) for _ in range(nj)]
            outl = [np.zeros(N, np.uint8) for _ in range(nj)]
            asg = [np.zeros(N, np.int32) for _ in range(nj)]
            pi, po, pa = table(ids), table(outl), table(asg)
            args = (rig.m._h, pool._h, rec.ctypes.data, nj, C.c_float(mc.TH), mc.MIN_MATCHES, 1, sig.ctypes.data, sf.ctypes.data, len(sig), out.ctypes.data, pi, po, pa, None)
            # ---- the parent's way's arrays
            lids = [np.ascontiguousarray(scenes[j % SCENES]["last_ids"], np.int32) for j in range(nj)]
            vel = np.ascontiguousarray([scenes[j % SCENES]["velocity"].reshape(16) for j in range(nj)], np.float32)
            ltc = np.ascontiguousarray([scenes[j % SCENES]["last_Tcw"].reshape(16) for j in range(nj)], np.float32)
            k = dict(fs=(vp * nj)(*[raw(sets[j]._h) for j in range(nj)]), lastIds=table(lids), tjobs=np.zeros(nj * 112, np.uint8), tout=np.zeros(nj, TRACK_RESULT_DTYPE),
                     idsPtr=(vp * nj)(), outlPtr=(vp * nj)(), which=np.zeros(nj, np.int32), TcwPred=np.zeros((nj, 16), np.float32), nSearch=np.zeros((nj, 2), np.int32),
                     wide=np.zeros(nj, np.int32), status=np.zeros(nj, np.int32), out=np.zeros(nj, TRACK_RESULT_DTYPE), idsOut=np.zeros((nj, N), np.int32),
                     outlierOut=np.zeros((nj, N), np.uint8), assignOut=np.zeros((nj, N), np.int32))
            addr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else C.cast(x, vp).value
            pw = ParentWay(fn("orbw_track_frame_pose"), fn("orbm_track_results"), fn("orbq_track_pose"), raw(rig.m._h), raw(pool._h), nj, N, N, len(sig), mc.MIN_MATCHES,
                           mc.TH, addr(k["fs"]), addr(k["lastIds"]), addr(vel), addr(ltc), addr(K), addr(bounds), addr(sig), addr(sf),
                           *[addr(k[x]) for x in ("tjobs", "tout", "idsPtr", "outlPtr", "which", "TcwPred", "nSearch", "wide", "status", "out", "idsOut", "outlierOut",
                                                  "assignOut")])

            def device():
                t0 = time.perf_counter()
                rcode = L.orbq_track_motion_model(*args)
                dt = time.perf_counter() - t0
                assert rcode == 0
                return dt

            def host():
                t0 = time.perf_counter()
                rcode = bshim.motionbench_parent_way(C.byref(pw))
                dt = time.perf_counter() - t0
                assert rcode == 0, rcode
                return dt
            device(); host()
            assert out.tobytes() == got[1].tobytes(), "the same call twice"
            assert out["track"].tobytes() == k["out"].tobytes() and out["Tcw_pred"].tobytes() == k["TcwPred"].tobytes(), "both ways' records, byte for byte"
            assert out["n_search"].tobytes() == k["nSearch"].tobytes() and out["wide"].tobytes() == k["wide"].tobytes() and out["status"].tobytes() == k["status"].tobytes()
            for j in range(nj):
                assert ids[j].tobytes() == k["idsOut"][j].tobytes() and outl[j].tobytes() == k["outlierOut"][j].tobytes() and asg[j].tobytes() == k["assignOut"][j].tobytes(), j
            t_end = time.perf_counter() + 1.0
            while time.perf_counter() < t_end:
                device(); host()
            td, th = [], []
            for _ in range(a.repeats):
                td.append(device()); th.append(host())
            td, th = np.array(td) * 1e3, np.array(th) * 1e3
            assert out["track"].tobytes() == k["out"].tobytes()
            summ = lambda t: dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))
            rows.append(dict(what="track_motion_model", jobs=nj, features_per_frame=N, image=[mc.BIG_W, mc.BIG_H], retry=retry, repeats=a.repeats,
                             n_search=[int(x) for x in out["n_search"][0]], n_matches=int(out["track"]["n_matches"][0]), chain_host=summ(th), motion_device=summ(td),
                             ratio_host_over_device=float(np.median(th) / np.median(td))))
            print(json.dumps(rows[-1]), flush=True)
        pool.close()
    doc = dict(tool="tools/motionmodel_bench.py",
               note="host clock around ONE ctypes call either way, ways alternated repeat by repeat after 1 s of warm-up; chain_host is one C entry at g++ -O2 that "
                    "makes the library calls of the parent commit (one frame/frame search and one wait a job, a second pair below 20 matches, one batched "
                    "orbq_track_pose); every array and pointer of either way is made once, outside the timed functions; both ways' outputs were compared byte for "
                    "byte with each other and job 0 with tools/motionmodel_ref.hpp first; the kernels' own times are not measured (no profiler run)", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
