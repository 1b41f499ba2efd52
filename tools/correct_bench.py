"""orbe_correct_sim3 through the Python mirror against the restatement on one host core: §8u's store of 1 000 keyframes
by 2 000 features, 1 600 points a keyframe, about 8 observations a point, with
  neighbourhood   K = 20 keyframes around one: LoopClosing::CorrectLoop over mvpCurrentConnectedKFs
  whole_map       all 1 000 keyframes: MultiMapper::UpdatePosesAndAdd over pMap->GetAllKeyFrames()
  device   KeyFrameStore.correct_sim3 with the commit and the copy down of both outputs
  host     tools/correct_ref.hpp at g++ -O2 on one core through ONE ctypes call into buffers made once, its observation index built ONCE
           outside the clock, followed by the orbw_pool_set of the moved points' records and the orbu_kf_set_centres of the listed
           keyframes (both assembled outside the clock) that the host way needs
After 1 s of warm-up the two ways are ALTERNATED repeat by repeat, host clock around each; every output record of both ways is compared
byte for byte before anything is timed.  Scw has scale 1 and a small motion, so that the committed positions stay finite over the
repeats.  The median and the 10th .. 90th percentile go to profiles/correct_bench.json.

    python tools/correct_bench.py [--repeats 30] [--out profiles/correct_bench.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_bench.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import correct_cases as cs
    import covis_cases as cc
    import refresh_cases as rc
    from ref_shim import p
    from refresh_bench import make_store_scene
    from orbslamm_amd import KeyFrameStore, MapPool, ORBmatcher
    from orbslamm_amd.map_pool import POINT_DTYPE
    m = ORBmatcher(0.8, True, device=0)
    rng = np.random.default_rng(1)
    r = make_store_scene(cc, rc, rng, 1000, 2000, 200, 1600, 9)
    c = cs.CScene(r, rng)
    q = np.array([0.002, -0.001, 0.0015, 1.0])
    c.Scw = np.concatenate([q / np.linalg.norm(q), [0.004, -0.003, 0.002], [1.0]])
    s = r.s
    pool = MapPool(m, s.pool_cap)
    pool.set(np.arange(s.pool_cap), r.pool_records())
    store = KeyFrameStore(pool, s.kfcap, s.stride, 4, 1 << 15)
    recs = s.records()
    for c0 in range(0, s.kfcap, 250):
        store.set(*[x[c0:c0 + 250] for x in recs])
    for k in range(s.kfcap):
        store.set_octaves(k, s.octaves[k])
    store.set_centres(np.arange(s.kfcap), r.centres)
    store.set_ref_kf(np.arange(s.pool_cap), r.ref_kf)
    shim = cs.shim()

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
        qq = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
        return {k: qq(v) for k, v in times.items()}

    rows = []
    for shape, slots, anchor_slot in (("neighbourhood", np.arange(490, 510), 500), ("whole_map", np.arange(s.kfcap), 500)):
        c.list_keyframes(slots, anchor_slot)
        # both ways' records, byte for byte, before anything is timed or committed
        wkf, wpts, _ = cs.ref_correct(c)
        kf, pts = store.correct_sim3(c.slots, c.Tiw, c.anchor, c.Scw, cs.SF, commit=False)
        assert kf.tobytes() == wkf.tobytes() and pts.tobytes() == wpts.tobytes(), shape
        assert not np.isnan(wpts["normal"]).any() and not np.isnan(wpts["pos"]).any()
        # the host way: the world's arrays the restatement overwrites, its index, the upload's records
        keep = [np.ascontiguousarray(x).copy() for x in (s.entries, s.kf_flags, s.octaves, r.centres, r.pos, r.normal, r.min_d, r.max_d, r.pt_flags(), r.ref_kf)]
        w = cs.RefWorld(s.kfcap, s.stride, p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), s.pool_cap, p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]), p(keep[8]),
                        p(keep[9]))
        idx = shim.cor_index(C.byref(w))
        slots32, Tiw, Scw, skip, sf = c.slots.copy(), c.Tiw, np.ascontiguousarray(c.Scw), np.zeros(0, np.int32), cs.SF.copy()
        args = cs.RefArgs(len(slots32), p(slots32), p(Tiw), c.anchor, p(Scw), p(skip), 0, p(sf), len(sf))
        okf, opts = np.zeros(len(slots32), cs.KF_DTYPE), np.zeros(s.pool_cap, cs.POINT_DTYPE)
        ids = np.ascontiguousarray(wpts["id"])
        up = np.zeros(len(ids), POINT_DTYPE)
        for n in ("pos", "normal", "min_distance", "max_distance"):
            up[n] = wpts[n]
        up["desc"], up["flags"] = r.pt_desc[ids], r.pt_flags()[ids]
        ctr = np.ascontiguousarray(wkf["Ow"])

        def host():
            shim.cor_correct_indexed(C.byref(w), idx, C.byref(args), p(okf), p(opts))
            pool.set(ids, up)
            store.set_centres(slots32, ctr)

        device = lambda: store.correct_sim3(c.slots, Tiw, c.anchor, Scw, sf, commit=True)
        t = run({"host": host, "device": device})
        shim.cor_index_free(idx)
        _, after = store.correct_sim3(c.slots, Tiw, c.anchor, Scw, sf, commit=False)
        assert np.isfinite(after["pos"]).all() and np.isfinite(after["normal"]).all()
        row = dict(store="1000x2000", shape=shape, keyframes_listed=int(len(slots32)), keyframes=int(s.kfcap), stride=int(s.stride), pool_points=int(s.pool_cap),
                   moved_points=int(len(wpts)), done_normal_depth=int((wpts["status"] == cs.ST_DONE).sum()), repeats=a.repeats, **t)
        print(json.dumps(row), flush=True)
        rows.append(row)
        pool.set(np.arange(s.pool_cap), r.pool_records())          # the next shape starts from the scene as generated
        store.set_centres(np.arange(s.kfcap), r.centres)
    store.close()
    pool.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/correct_bench.py",
                       note="host clock around each way, ways alternated repeat by repeat after 1 s of warm-up; host is tools/correct_ref.hpp at g++ -O2 on one "
                            "core through one ctypes call into buffers made once, over flat arrays and an observation index built outside the clock, followed by "
                            "orbw_pool_set of the moved points' records and orbu_kf_set_centres of the listed keyframes (assembled outside the clock); device is "
                            "the Python mirror's call with the commit and the copy down of both outputs; the kernels' own times are not measured (no profiler run)",
                       rows=rows), f, indent=1)
        f.write("\n")
    print("correct bench: written to %s" % a.out)


if __name__ == "__main__":
    main()
