"""The body of Tracking::Relocalization behind PnPsolver::iterate in one call (orbq_relocalize) against the parent's way:
1, 8 and 32 candidate keyframes a call, lost frames of 2 000 features, rows of 1 700 entries, with the mixture of exits stated per row.
  stages_host     the parent's way as ONE C entry (tests/cpp/reloc_bench_capi.cpp, g++ -O2): per stage ONE orbo_pose_optimize_frames over
                  the jobs still running (edge records gathered from a flat host copy of the pool), the host discard and gates, the host
                  projection of the candidate's row over flat arrays (no pointer chasing: the kindest host form), one
                  orbm_track_frame_projected + orbm_track_results a job at each of the two searches
  reloc_device    ONE orbq_relocalize
The candidates are scenes of tests/reloc_cases.py at that size -- third_succeeds, second_low, narrow_short, wide_short, first and
rejected in turn -- each with its lost frame and its keyframe in a slot pair of a frame set (two candidates a set) and a row of the
store; the pool holds every scene's points.  The keyframe's slot holds the row's points' descriptors, which is where
orbm_track_frame_projected takes its query descriptors from (orbq_relocalize reads the pool's).  Both ways' outputs -- records, ids,
outlier bytes, status bytes -- are compared byte for byte with each other and with the restatement (tools/reloc_ref.hpp) before
anything is timed.  After 1 s of warm-up the ways are ALTERNATED repeat by repeat, host clock around one ctypes call either way (every
array and pointer made once, outside the timed functions); the median and the 10th .. 90th percentile go to profiles/reloc_bench.json.

    python tools/reloc_bench.py [--repeats 30] [--jobs 1 8 32] [--out profiles/reloc_bench.json]"""
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

N_FEAT, N_ROW, CAP = 2000, 1700, 2048
MIX = ("third_succeeds", "second_low", "narrow_short", "wide_short", "first", "rejected")
EXIT_NAMES = ("REJECTED", "FIRST", "WIDE_SHORT", "SECOND", "NARROW_SHORT", "THIRD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import localmap_cases as lc
    import reloc_cases as rc
    from ref_shim import build_ref_shim
    from orbslamm_amd._lib import lib, table
    from orbslamm_amd.optimizer import EDGE_DTYPE, FRAME_DTYPE, RESULT_DTYPE
    from orbslamm_amd.track_pose import RELOC_RESULT_DTYPE, pack_reloc_jobs
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    raw = lambda h: h.value if isinstance(h, vp) else int(h)

    class ParentWay(C.Structure):   # tests/cpp/reloc_bench_capi.cpp
        _fields_ = ([(k, vp) for k in ("poseOpt", "trackProjected", "trackResults", "h")] + [(k, i32) for k in ("J", "n", "stride", "cap", "nlevels", "checkOri")] +
                    [(k, vp) for k in ("fs", "slot", "kfSlot", "resident", "entries", "idsIn", "TcwIn", "K", "pos", "minD", "maxD", "flags")] + [("poolCap", i32)] +
                    [(k, vp) for k in ("sig", "sf", "breaks", "bounds", "frames", "residentLive", "edges", "start", "optOut", "eflags", "live", "uvr", "lvl", "qv",
                                       "occ", "mark", "out", "idsOut", "outlierOut", "status")])
    bshim = build_ref_shim("reloc_bench")
    assert bshim.relocbench_sizeof() == C.sizeof(ParentWay) and bshim.relocbench_sizeof_res() == RELOC_RESULT_DTYPE.itemsize
    bshim.relocbench_parent_way.argtypes = [vp]
    rig = rc.Rig()
    nmax = max(a.jobs)
    cases, base = [], 0
    for j in range(nmax):
        fam = MIX[j % len(MIX)]
        c = rc.make_case(fam, 11 + j, n=N_FEAT, nk=N_ROW, counts=rc.EXIT_FAMILIES[fam])
        c["entries"] = np.where(c["entries"] >= 0, c["entries"] + base, -1).astype(np.int32)
        c["ids"] = np.where(c["ids"] >= 0, c["ids"] + base, -1).astype(np.int32)
        base += len(c["pool"])
        cases.append(c)
    records = np.concatenate([c["pool"] for c in cases])
    sets = [rig.new_set(CAP) for _ in range((nmax + 1) // 2)]
    resident = []
    for j, c in enumerate(cases):
        c["pool"] = records
        row = c["entries"].astype(np.int64)
        kfdesc = np.where((row >= 0)[:, None], records["desc"][np.maximum(row & ~rc.NO_VOTE, 0)], 0).astype(np.uint8)
        rig.put(sets[j // 2], 2 * (j % 2), rc.kf_keys(c), kfdesc)
        resident.append(rig.put(sets[j // 2], 2 * (j % 2) + 1, c["keys"], c["desc"], resident=True))
    pool, store = rc.new_world(rig, records, [c["entries"] for c in cases], N_ROW, kfcap=nmax)
    refs = [rc.ref_run(c) for c in cases]
    sig, sf, brk = rc.sigma2(), np.ascontiguousarray(lc.SF, np.float32), rc.breaks()
    pos, mind, maxd = (np.ascontiguousarray(records[k], np.float32) for k in ("pos", "min_distance", "max_distance"))
    flags, bounds, K = np.ascontiguousarray(records["flags"], np.uint8), np.array(lc.BOUNDS, np.float32), np.ascontiguousarray(lc.K_A, np.float32)
    fn = lambda name: C.cast(getattr(L, name), vp).value
    rows = []
    for nj in a.jobs:
        jobs = [rc.job(sets[j // 2], 2 * (j % 2), 2 * (j % 2) + 1, j, cases[j]) for j in range(nj)]
        got = rc.call(rig, pool, store, jobs)
        for j in range(nj):
            rc.assert_job_equals_ref(got, j, refs[j], ("bench", nj, j))
        # ---- the device way's arrays
        rec, keep = pack_reloc_jobs(jobs)
        out = np.zeros(nj, RELOC_RESULT_DTYPE)
        ids = [np.zeros(N_FEAT, np.int32) for _ in range(nj)]
        outl = [np.zeros(N_FEAT, np.uint8) for _ in range(nj)]
        status = [np.zeros((2, N_ROW), np.uint8) for _ in range(nj)]
        pi, po, ps = table(ids), table(outl), table(status)
        args = (rig.m._h, pool._h, store._h, rec.ctypes.data, nj, 1, sig.ctypes.data, sf.ctypes.data, brk.ctypes.data, len(sig), out.ctypes.data, pi, po, ps)
        # ---- the parent's way's arrays
        ents = [np.ascontiguousarray(cases[j]["entries"], np.int32) for j in range(nj)]
        idin = [np.ascontiguousarray(cases[j]["ids"], np.int32) for j in range(nj)]
        tcw = np.ascontiguousarray([np.asarray(cases[j]["Tcw"], np.float32).reshape(16) for j in range(nj)], np.float32)
        k = dict(fs=(vp * nj)(*[raw(sets[j // 2]._h) for j in range(nj)]), slot=np.array([2 * (j % 2) + 1 for j in range(nj)], np.int32),
                 kfSlot=np.array([2 * (j % 2) for j in range(nj)], np.int32), resident=(vp * nj)(*[raw(f) for f in resident[:nj]]), entries=table(ents), idsIn=table(idin),
                 frames=np.zeros(nj, FRAME_DTYPE), residentLive=(vp * nj)(), edges=np.zeros(nj * N_FEAT, EDGE_DTYPE), start=np.zeros(nj + 1, np.int32),
                 optOut=np.zeros(nj, RESULT_DTYPE), eflags=np.zeros(nj * N_FEAT, np.uint8), live=np.zeros(nj, np.int32), uvr=np.zeros(3 * N_ROW, np.float32),
                 lvl=np.zeros(2 * N_ROW, np.int8), qv=np.zeros(N_ROW, np.uint8), occ=np.zeros(CAP, np.uint8), mark=np.zeros(len(records), np.uint8),
                 out=np.zeros(nj, RELOC_RESULT_DTYPE), idsOut=np.zeros((nj, N_FEAT), np.int32), outlierOut=np.zeros((nj, N_FEAT), np.uint8),
                 status=np.zeros((nj, 2, N_ROW), np.uint8))
        addr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else C.cast(x, vp).value
        pw = ParentWay(fn("orbo_pose_optimize_frames"), fn("orbm_track_frame_projected"), fn("orbm_track_results"), raw(rig.m._h),
                       nj, N_FEAT, N_ROW, CAP, len(sig), 1, addr(k["fs"]), addr(k["slot"]), addr(k["kfSlot"]), addr(k["resident"]), addr(k["entries"]), addr(k["idsIn"]),
                       addr(tcw), addr(K), addr(pos), addr(mind), addr(maxd), addr(flags), len(records), addr(sig), addr(sf), addr(brk), addr(bounds),
                       *[addr(k[x]) for x in ("frames", "residentLive", "edges", "start", "optOut", "eflags", "live", "uvr", "lvl", "qv", "occ", "mark", "out", "idsOut",
                                              "outlierOut", "status")])

        def device():
            t0 = time.perf_counter()
            rcode = L.orbq_relocalize(*args)
            dt = time.perf_counter() - t0
            assert rcode == 0
            return dt

        def host():
            t0 = time.perf_counter()
            rcode = bshim.relocbench_parent_way(C.byref(pw))
            dt = time.perf_counter() - t0
            assert rcode == 0, rcode
            return dt
        device(); host()
        assert out.tobytes() == got[1].tobytes() == k["out"].tobytes(), "both ways' records, byte for byte"
        for j in range(nj):
            assert ids[j].tobytes() == k["idsOut"][j].tobytes() and outl[j].tobytes() == k["outlierOut"][j].tobytes() and status[j].tobytes() == k["status"][j].tobytes(), j
        assert not k["mark"].any()
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            device(); host()
        td, th = [], []
        for _ in range(a.repeats):
            td.append(device()); th.append(host())
        td, th = np.array(td) * 1e3, np.array(th) * 1e3
        assert out.tobytes() == k["out"].tobytes()
        exits = [int(e) for e in out["exit"]]
        summ = lambda t: dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))
        rows.append(dict(what="relocalize", jobs=nj, features_per_frame=N_FEAT, row_entries=N_ROW, repeats=a.repeats,
                         exits={EXIT_NAMES[e]: exits.count(e) for e in sorted(set(exits))}, stages_host=summ(th), reloc_device=summ(td),
                         ratio_host_over_device=float(np.median(th) / np.median(td))))
        print(json.dumps(rows[-1]))
    doc = dict(tool="tools/reloc_bench.py",
               note="host clock around ONE ctypes call either way, ways alternated repeat by repeat after 1 s of warm-up; stages_host is one C entry at g++ -O2 that "
                    "makes the library calls and runs the discard, the gates and the projection over flat arrays (the reference chases MapPoint pointers instead); "
                    "every array and pointer of either way is made once, outside the timed functions; both ways' outputs were compared byte for byte with each "
                    "other and with tools/reloc_ref.hpp first; the kernels' own times are not measured (no profiler run)", rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    store.close(); pool.close()


if __name__ == "__main__":
    main()
