"""PoseOptimization behind the local-map search, fed from the pool (orbq_track_pose) against the parent's way: 1, 8 and
64 frames a call, about 100, 300 and 1 000 edges a frame out of frames of 2 000 features, a third of the edges held by the frame
before the search and the rest matched by it:
  host_edges    the parent's way: orbm_track_results per frame, the merge and the gather of Xw from a flat host copy of the pool into
                edge records (g++ -O2, no pointer chasing: the kindest host form), ONE orbo_pose_optimize_frames for all frames, the walk
                over the outlier bytes with the discard and the two counts
  pool_device   orbm_track_results per frame, ONE orbq_track_pose
The frames lie in 32 slots of eight frame sets (a call of 64 names each twice).  After 1 s of warm-up the ways are ALTERNATED repeat by
repeat, host clock around the calls and their results; the median and the 10th .. 90th percentile go to profiles/trackpose_bench.json
with the bytes either way sends up per frame (computed from the record sizes).  Both ways' outputs are compared before anything is timed.

    python tools/trackpose_bench.py [--repeats 30] [--jobs 1 8 64] [--edges 100 300 1000] [--out profiles/trackpose_bench.json]"""
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

N_FEAT, SETS, SLOTS = 2000, 8, 4
# what a frame adds to a call's packed upload, COMPUTED from the record sizes (sizeof(orbo::FrameIn), sizeof(orbq::JobDev); an edge record is
# EDGE_DTYPE, a base id 4 bytes), not read back from the library; a call's blocks are padded to 16 bytes, at most 15 more a call
FRAME_IN_BYTES, JOB_DEV_BYTES = 104, 136   # (orbq_host.inc holds both with a static_assert)


def lattice_keys(rng, n, KP_DTYPE):
    """n keypoints on an 11-pixel lattice, moved by up to a pixel, octaves 0 and 1: no search window holds two"""
    cols, rows = 56, 40
    cell = rng.permutation(cols * rows)[:n]
    keys = np.zeros(n, KP_DTYPE)
    keys["x"] = 12.0 + 11.0 * (cell % cols) + rng.uniform(-1, 1, n)
    keys["y"] = 12.0 + 11.0 * (cell // cols) + rng.uniform(-1, 1, n)
    keys["octave"] = rng.integers(0, 2, n)
    keys["size"], keys["angle"], keys["response"], keys["class_id"] = 31.0, rng.uniform(0, 360, n), 50.0, -1
    return keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--edges", type=int, nargs="+", default=[100, 300, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackpose_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import localmap_cases as lc
    import poseopt_cases as pc
    import trackpose_cases as tc
    from ref_shim import p
    from orbslamm_amd import MapPool, ORBextractor, ORBmatcher, level_breaks, make_grid
    from orbslamm_amd._lib import KP_DTYPE, check, lib, ptr
    from orbslamm_amd.optimizer import EDGE_DTYPE, FRAME_DTYPE, RESULT_DTYPE
    from orbslamm_amd.track_pose import TRACK_RESULT_DTYPE, pack_jobs
    L = lib()
    shim = tc.ref_lib()
    vp = C.c_void_p
    shim.trackposeref_host_edges.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    shim.trackposeref_host_epilogue.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    shim.trackposeref_host_epilogue.restype = None
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=lc.W, max_height=lc.H, max_batch=1, device=0)   # (device memory for the frames' keys)
    m = ORBmatcher(0.8, True, device=0)
    grid = make_grid(0.0, 0.0, float(lc.W), float(lc.H))
    breaks = level_breaks(lc.LOG_SF, lc.NLEVELS)
    sig = pc.inv_level_sigma2(lc.NLEVELS)
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
        q = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
        return {k: q(v) for k, v in times.items()}

    rows = []
    for E in a.edges:
        # 32 sources: frame k of set k // 4, slot k % 4; each its own keys, points, start pose and search
        rng = np.random.default_rng(E)
        view = lc.make_view(lc.rot_axis_angle([0.2, 1.0, 0.1], 0.05), [0.1, -0.05, 0.2])
        R, t = view[0]["Rcw"].reshape(3, 3).astype(np.float64), view[0]["tcw"].astype(np.float64)
        src, records = [], []
        for k in range(SETS * SLOTS):
            keys = lattice_keys(rng, N_FEAT, KP_DTYPE)
            desc = rng.integers(0, 256, (N_FEAT, 32), dtype=np.uint8)
            feat = rng.permutation(N_FEAT)[:E]
            pts = lc.points_from_keys(rng, view, keys[feat], lc.SF, desc[feat], jitter=0.4)
            pts["flags"] = lc.FLAG_OBSERVED
            off = k * E
            base = np.full(N_FEAT, -1, np.int32)
            base[feat[:E // 3]] = off + np.arange(E // 3)
            ids = (off + E // 3 + rng.permutation(E - E // 3)).astype(np.int32)
            Tcw = pc.tcw_of(lc.rot_axis_angle(rng.normal(size=3), np.deg2rad(0.2)) @ R, t + 0.005 * rng.normal(size=3))
            dk, dd, dn = up(keys), up(desc), up(np.array([N_FEAT], np.int32))
            fs, slot = sets[k // SLOTS], k % SLOTS
            fs.build(slot, 1, dk, dd, dn, N_FEAT)
            frame = m.frame_from_device(dk, dd, N_FEAT, lc.K_A, [0, 0, 0, 0, 0], grid)
            src.append(dict(fs=fs, slot=slot, back=SLOTS - 1 - slot, base=base, ids=ids, Tcw=Tcw, frame=frame))
            records.append(pts)
        records = np.concatenate(records)
        pool = MapPool(m, len(records))
        pool.set(np.arange(len(records)), records)
        pos = np.ascontiguousarray(records["pos"], np.float32)
        flags = np.ascontiguousarray(records["flags"], np.uint8)
        for fs in sets:
            fs.sync()
        for s in src:      # slot 0's search first: it lies SLOTS - 1 back once the set's four are issued
            pool.track_local_map(s["fs"], s["slot"], view, s["ids"], 1.0, lc.SF, breaks, t_occ=(s["base"] >= 0).astype(np.uint8))
        for s in src:
            assign, nm = s["fs"].results(s["back"])
            assert nm[0] >= 0.97 * (E - E // 3), (nm[0], E)
        for J in a.jobs:
            jobs = [src[j % len(src)] for j in range(J)]
            # ---- the parent's way, every buffer made once
            frames = np.zeros(J, FRAME_DTYPE)
            for j, s in enumerate(jobs):
                frames["Tcw"][j], frames["K"][j] = s["Tcw"].reshape(16), lc.K_A
            resident = (C.c_void_p * J)(*[s["frame"] for s in jobs])
            edges = np.zeros(J * N_FEAT, EDGE_DTYPE)
            start = np.zeros(J + 1, np.int32)
            merged = np.zeros((J, N_FEAT), np.int32)
            out_h = np.zeros(J, RESULT_DTYPE)
            eflags = np.zeros(J * N_FEAT, np.uint8)
            ids_h, outl_h, counts_h = np.zeros((J, N_FEAT), np.int32), np.zeros((J, N_FEAT), np.uint8), np.zeros((J, 2), np.int32)
            pa = C.c_void_p()

            def host_edges():
                m_ = 0
                for j, s in enumerate(jobs):
                    check(L.orbm_track_results(s["fs"]._h, s["back"], C.byref(pa), None, None, None))
                    m_ += shim.trackposeref_host_edges(pa, p(s["ids"]), p(s["base"]), N_FEAT, p(pos), p(merged[j]), edges[m_:].ctypes.data)
                    start[j + 1] = m_
                check(L.orbo_pose_optimize_frames(m._h, ptr(frames), resident, J, ptr(start), ptr(edges), ptr(sig), len(sig), ptr(out_h), ptr(eflags)))
                for j in range(J):
                    shim.trackposeref_host_epilogue(p(merged[j]), N_FEAT, eflags[start[j]:].ctypes.data, p(flags), 0, p(ids_h[j]), p(outl_h[j]), p(counts_h[j]))

            # ---- the new way
            rec, keep = pack_jobs([dict(fs=s["fs"], slot=s["slot"], back=s["back"], base_ids=s["base"], n=N_FEAT, discard=0, Tcw=s["Tcw"], K=lc.K_A) for s in jobs])
            out_d = np.zeros(J, TRACK_RESULT_DTYPE)
            ids_d, outl_d = np.zeros((J, N_FEAT), np.int32), np.zeros((J, N_FEAT), np.uint8)
            pi = (C.c_void_p * J)(*[ids_d[j].ctypes.data for j in range(J)])
            po = (C.c_void_p * J)(*[outl_d[j].ctypes.data for j in range(J)])

            def pool_device():
                for s in jobs:
                    check(L.orbm_track_results(s["fs"]._h, s["back"], C.byref(pa), None, None, None))
                check(L.orbq_track_pose(m._h, pool._h, ptr(rec), J, ptr(sig), len(sig), ptr(out_d), pi, po))

            # both ways' results, compared before anything is timed
            host_edges()
            pool_device()
            assert out_d["opt"].tobytes() == out_h.tobytes() and ids_d.tobytes() == ids_h.tobytes() and outl_d.tobytes() == outl_h.tobytes()
            assert np.array_equal(out_d["n_matches"], counts_h[:, 0]) and np.array_equal(out_d["n_matches_map"], counts_h[:, 1])
            assert (out_h["n_initial"] >= 0.97 * E).all() and (out_h["rounds"] == 4).all() and (counts_h[:, 0] > 0.9 * E).all()
            r = run({"host_edges": host_edges, "pool_device": pool_device})
            row = dict(what="track_pose", jobs=J, edges_per_frame=E, features_per_frame=N_FEAT, repeats=a.repeats,
                       upload_bytes_per_frame=dict(host_edges=E * EDGE_DTYPE.itemsize + FRAME_IN_BYTES, pool_device=N_FEAT * 4 + JOB_DEV_BYTES), **r)
            row["ratio_host_over_device"] = row["host_edges"]["median_ms"] / row["pool_device"]["median_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        for s in src:
            m.frame_destroy(s["frame"])
        pool.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/trackpose_bench.py",
                       note="host clock around each way's calls and results, ways alternated repeat by repeat after 1 s of warm-up; host_edges' merge, "
                            "gather and epilogue are C loops over flat arrays at g++ -O2 through ctypes (the reference chases MapPoint pointers instead); both "
                            "ways call the C entries with buffers made once; the kernels' own times are not measured (no profiler run)", rows=rows), f, indent=1)
        f.write("\n")
    print("trackpose bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
