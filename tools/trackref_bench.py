"""Tracking::TrackReferenceKeyFrame from the BoW search to the pose verdict in one call (orbq_track_reference) against the
parent's way: 1, 8 and 64 (keyframe, frame) pairs a call, frames of 2 000 features, keyframes whose features all hold good points (so
that both ways compute the same thing: orbm_bow_frames counts every keyframe feature as valid), a 10 x 10 x 10 vocabulary with the
FeatureVector at its 100 level-2 nodes:
  bow_host_edges  the parent's way as ONE C entry (tests/cpp/trackref_bench_capi.cpp, g++ -O2): orbm_bow_frames + orbm_bow_results per
                  frame set, the merge through a flat host copy of the keyframe's match list and the gather of Xw from a flat host copy of
                  the pool into edge records (no pointer chasing: the kindest host form), ONE orbo_pose_optimize_frames for all frames,
                  the walk over the outlier bytes with the discard and the two counts; the tables are read where orbm_bow_results left them
  reference_device  ONE orbq_track_reference, the match tables asked for
The pairs lie in 16 frame sets of four slots (two pairs a set; a call of 64 names each pair twice).  After 1 s of warm-up the ways are
ALTERNATED repeat by repeat, host clock around one ctypes call either way (every array and pointer made once, outside the timed functions); the median and the 10th .. 90th percentile go to
profiles/trackref_bench.json.  Both ways' outputs are compared byte for byte before anything is timed.

    python tools/trackref_bench.py [--repeats 30] [--jobs 1 8 64] [--out profiles/trackref_bench.json]"""
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

N_FEAT, SETS, SLOTS = 2000, 16, 4
VOC_K, VOC_L, LEVELSUP = 10, 3, 1
FRAME_IN_BYTES, REF_JOB_DEV_BYTES = 104, 152   # sizeof(orbo::FrameIn), sizeof(orbq::RefJobDev): orbq_host.inc holds both with a static_assert


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackref_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    if max(a.jobs) > SETS * SLOTS:
        ap.error("at most %d jobs: a frame set's orbm_bow_frames takes as many pairs as it has slots" % (SETS * SLOTS))
    import localmap_cases as lc
    import poseopt_cases as pc
    import trackref_cases as rc
    from ref_shim import build_ref_shim
    from orbslamm_amd import KeyFrameStore, MapPool, ORBextractor, ORBmatcher, ORBVocabulary, make_grid
    from orbslamm_amd._lib import check, lib, ptr
    from orbslamm_amd.optimizer import EDGE_DTYPE, FRAME_DTYPE, RESULT_DTYPE
    from orbslamm_amd.track_pose import REF_RESULT_DTYPE, pack_ref_jobs
    L = lib()
    vp = C.c_void_p

    class ParentWay(C.Structure):   # tests/cpp/trackref_bench_capi.cpp
        _fields_ = ([(k, vp) for k in ("bowFrames", "bowResults", "poseOpt", "h")] + [("ncalls", C.c_int32)] +
                    [(k, vp) for k in ("call_fs", "call_start", "kf_slots", "frame_slots", "job_of")] + [("nnratio", C.c_float), ("check_ori", C.c_int32),
                    ("J", C.c_int32), ("n", C.c_int32)] + [(k, vp) for k in ("entries", "pos", "flags", "frames", "resident", "sig")] + [("nlevels", C.c_int32)] +
                    [(k, vp) for k in ("tables", "merged", "edges", "start", "out", "eflags", "nbow", "ids_out", "outlier_out", "counts", "match_copy")])
    bshim = build_ref_shim("trackref_bench")
    assert bshim.trackrefbench_sizeof() == C.sizeof(ParentWay)
    bshim.trackrefbench_parent_way.argtypes = [vp]
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=lc.W, max_height=lc.H, max_batch=1, device=0)   # (device memory for the frames' keys)
    m = ORBmatcher(0.7, True, device=0)
    grid = make_grid(0.0, 0.0, float(lc.W), float(lc.H))
    sig = pc.inv_level_sigma2(lc.NLEVELS)
    v = rc.vocabulary(VOC_K, VOC_L)
    G = ORBVocabulary(VOC_K, VOC_L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)
    sets = [m.frame_set(SLOTS, N_FEAT, lc.K_A, [0, 0, 0, 0, 0], grid, list(lc.BOUNDS), lc.SF) for _ in range(SETS)]

    def up(arr):
        arr = np.ascontiguousarray(arr)
        d = C.c_void_p()
        check(L.orbx_device_alloc(gex._h, C.c_size_t(arr.nbytes), C.byref(d)))
        check(L.orbx_upload(gex._h, d, ptr(arr), C.c_size_t(arr.nbytes)))
        return d.value

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def run(ways):
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            for fn in ways.values():
                fn()
        times = {k: [] for k in ways}
        for _ in range(a.repeats):
            for k, fn in ways.items():
                times[k].append(timed(fn))
        q = lambda t: dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))
        return {k: q(t) for k, t in times.items()}

    # 32 pairs: pair k in set k // 2, keyframe in slot 2 (k % 2), frame in slot 2 (k % 2) + 1, store slot k
    npairs = SETS * SLOTS // 2
    src, records, rows_e = [], [], []
    off = 0
    for k in range(npairs):
        c = rc.make_case("all_valid", 100 + k, n=N_FEAT)
        fs, ks = sets[k // 2], 2 * (k % 2)
        for slot, keys, desc in ((ks, c["kkeys"], c["kdesc"]), (ks + 1, c["keys"], c["desc"])):
            dk, dd, dn = up(keys), up(desc), up(np.array([N_FEAT], np.int32))
            fs.build(slot, 1, dk, dd, dn, N_FEAT)
        frame = m.frame_from_device(dk, dd, N_FEAT, lc.K_A, [0, 0, 0, 0, 0], grid)
        ent = (c["entries"] + off).astype(np.int32)
        src.append(dict(fs=fs, set=k // 2, kf_slot=ks, slot=ks + 1, kf=k, Tcw=c["Tcw"], frame=frame, entries=ent))
        records.append(c["pool"])
        rows_e.append(ent)
        off += len(c["pool"])
    records = np.concatenate(records)
    pool = MapPool(m, len(records))
    pool.set(np.arange(len(records)), records)
    store = KeyFrameStore(pool, npairs, N_FEAT, 0, 16)
    store.set(np.arange(npairs), np.zeros(npairs, np.uint8), rows_e, [[] for _ in range(npairs)], [-1] * npairs, [[] for _ in range(npairs)])
    pos = np.ascontiguousarray(records["pos"], np.float32)
    flags = np.ascontiguousarray(records["flags"], np.uint8)
    for fs in sets:
        fs.sync()
        fs.compute_bow(G, 0, SLOTS, LEVELSUP)

    rows = []
    for J in a.jobs:
        jobs = [src[j % npairs] for j in range(J)]
        # ---- the parent's way, every buffer made once: the jobs of one frame set go into one orbm_bow_frames
        by_set = {}
        for j, s in enumerate(jobs):
            by_set.setdefault(s["set"], []).append(j)
        calls = [(sets[k], np.array([jobs[j]["kf_slot"] for j in js], np.int32), np.array([jobs[j]["slot"] for j in js], np.int32), js) for k, js in by_set.items()]
        assert all(len(c[3]) <= SLOTS for c in calls)
        frames = np.zeros(J, FRAME_DTYPE)
        for j, s in enumerate(jobs):
            frames["Tcw"][j], frames["K"][j] = np.asarray(s["Tcw"], np.float32).reshape(16), lc.K_A
        resident = (C.c_void_p * J)(*[s["frame"] for s in jobs])
        edges = np.zeros(J * N_FEAT, EDGE_DTYPE)
        start = np.zeros(J + 1, np.int32)
        merged = np.zeros((J, N_FEAT), np.int32)
        out_h = np.zeros(J, RESULT_DTYPE)
        eflags = np.zeros(J * N_FEAT, np.uint8)
        ids_h, outl_h, counts_h = np.zeros((J, N_FEAT), np.int32), np.zeros((J, N_FEAT), np.uint8), np.zeros((J, 2), np.int32)
        match_h, nbow_h = np.zeros((J, N_FEAT), np.int32), np.zeros(J, np.int32)
        # every pointer made ONCE, as for the new way: the timed function is one C call (tests/cpp/trackref_bench_capi.cpp)
        call_fs = (C.c_void_p * len(calls))(*[c[0]._h.value for c in calls])
        call_start = np.concatenate([[0], np.cumsum([len(c[3]) for c in calls])]).astype(np.int32)
        kslots, fslots = np.concatenate([c[1] for c in calls]).astype(np.int32), np.concatenate([c[2] for c in calls]).astype(np.int32)
        job_of = np.concatenate([c[3] for c in calls]).astype(np.int32)
        ent_ptrs = (C.c_void_p * J)(*[s["entries"].ctypes.data for s in jobs])
        tables = (C.c_void_p * J)()
        fn = lambda f: C.cast(f, C.c_void_p).value
        w = ParentWay(fn(L.orbm_bow_frames), fn(L.orbm_bow_results), fn(L.orbo_pose_optimize_frames), m._h.value,
                      len(calls), C.cast(call_fs, vp).value, call_start.ctypes.data, kslots.ctypes.data, fslots.ctypes.data, job_of.ctypes.data, 0.7, 1,
                      J, N_FEAT, C.cast(ent_ptrs, vp).value, pos.ctypes.data, flags.ctypes.data, frames.ctypes.data, C.cast(resident, vp).value, sig.ctypes.data, len(sig),
                      C.cast(tables, vp).value, merged.ctypes.data, edges.ctypes.data, start.ctypes.data, out_h.ctypes.data, eflags.ctypes.data,
                      nbow_h.ctypes.data, ids_h.ctypes.data, outl_h.ctypes.data, counts_h.ctypes.data, match_h.ctypes.data)
        pw = C.byref(w)

        def bow_host_edges():
            check(bshim.trackrefbench_parent_way(pw))

        # ---- the new way
        rec = pack_ref_jobs([dict(fs=s["fs"], kf_slot=s["kf_slot"], slot=s["slot"], kf=s["kf"], n=N_FEAT, solve=1, Tcw=s["Tcw"], K=lc.K_A) for s in jobs])
        out_d = np.zeros(J, REF_RESULT_DTYPE)
        ids_d, outl_d, match_d = np.zeros((J, N_FEAT), np.int32), np.zeros((J, N_FEAT), np.uint8), np.zeros((J, N_FEAT), np.int32)
        pi = (C.c_void_p * J)(*[ids_d[j].ctypes.data for j in range(J)])
        po = (C.c_void_p * J)(*[outl_d[j].ctypes.data for j in range(J)])
        pt = (C.c_void_p * J)(*[match_d[j].ctypes.data for j in range(J)])

        def reference_device():
            check(L.orbq_track_reference(m._h, pool._h, store._h, ptr(rec), J, 0.7, 1, 15, ptr(sig), len(sig), ptr(out_d), pi, po, pt))

        # both ways' results, compared byte for byte before anything is timed; the parent's tables are copied out for that alone
        bow_host_edges()
        reference_device()
        w.match_copy = None
        assert match_d.tobytes() == match_h.tobytes() and np.array_equal(out_d["n_bow"], nbow_h)
        assert out_d["track"]["opt"].tobytes() == out_h.tobytes() and ids_d.tobytes() == ids_h.tobytes() and outl_d.tobytes() == outl_h.tobytes()
        assert np.array_equal(out_d["track"]["n_matches"], counts_h[:, 0]) and np.array_equal(out_d["track"]["n_matches_map"], counts_h[:, 1])
        assert (out_d["status"] == 0).all() and (nbow_h > 1000).all() and (out_h["rounds"] == 4).all() and (counts_h[:, 1] > 900).all()
        r = run({"bow_host_edges": bow_host_edges, "reference_device": reference_device})
        ne = int(start[J]) // J
        row = dict(what="track_reference", jobs=J, features_per_frame=N_FEAT, edges_per_frame=ne, repeats=a.repeats,
                   upload_bytes_per_frame=dict(bow_host_edges=ne * EDGE_DTYPE.itemsize + FRAME_IN_BYTES + 8, reference_device=REF_JOB_DEV_BYTES), **r)
        row["ratio_host_over_device"] = row["bow_host_edges"]["median_ms"] / row["reference_device"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/trackref_bench.py",
                       note="host clock around ONE ctypes call either way, ways alternated repeat by repeat after 1 s of warm-up; bow_host_edges is one C "
                            "entry at g++ -O2 that makes the library calls and runs the merge, gather and epilogue over flat arrays (the reference chases "
                            "MapPoint pointers instead); every array and pointer of either way is made once, outside the timed functions; the kernels' own "
                            "times are not measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("trackref bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
