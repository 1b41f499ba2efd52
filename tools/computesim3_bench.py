"""LoopClosing::ComputeSim3 behind the Sim3Solver in one call (orby_compute_sim3) against the parent's way, through the
Python mirrors, their losses included: 1, 8 and 64 candidates of 2 000 features (tests/computesim3_cases.py's scene, 40 entering
matches; every job names the same resident pair, which the entry allows):
  parent_way      per candidate the host gates of both passes (numpy), two resident orbm_window_best_frame calls, the host agreement
                  and the host walk into a correspondence list; then ONE optimize_sim3_batch over all candidates
  compute_sim3    ONE compute_sim3_batch
After a warm-up the ways are ALTERNATED repeat by repeat, host clock around each; the median and the 10th .. 90th percentile go to
profiles/computesim3_bench.json.  Both ways' results (OrbzResult fields, removed bytes) are compared before anything is timed.

    python tools/computesim3_bench.py [--repeats 20] [--jobs 1 8 64] [--out profiles/computesim3_bench.json]"""
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

N_FEAT = 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "computesim3_bench.json"))
    a = ap.parse_args()
    import computesim3_cases as cc
    import localmap_cases as lc
    from orbslamm_amd import KeyFrameStore, MapPool, ORBextractor, ORBmatcher, compute_sim3_batch, make_grid, optimize_sim3_batch
    from orbslamm_amd._lib import check, lib, ptr
    L = lib()
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=lc.W, max_height=lc.H, max_batch=1, device=0)   # (device memory for the frames' keys)
    m = ORBmatcher(0.7, True, device=0)
    grid = make_grid(0.0, 0.0, float(lc.W), float(lc.H))
    sig, brk = cc.sigma2(), cc.breaks()
    case = cc.make_case("inliers_in", 3, n=N_FEAT)
    fs = m.frame_set(2, 2048, lc.K_A, [0, 0, 0, 0, 0], grid, list(lc.BOUNDS), lc.SF)

    def up(arr):
        arr = np.ascontiguousarray(arr)
        d = C.c_void_p()
        check(L.orbx_device_alloc(gex._h, C.c_size_t(arr.nbytes), C.byref(d)))
        check(L.orbx_upload(gex._h, d, ptr(arr), C.c_size_t(arr.nbytes)))
        return d.value
    frames = []
    for slot, (k, d) in enumerate(((case["keys1"], case["desc1"]), (case["keys2"], case["desc2"]))):
        dk, dd, dn = up(k), up(d), up(np.array([len(k)], np.int32))
        fs.build(slot, 1, dk, dd, dn, len(k))
        frames.append(m.frame_from_device(dk, dd, len(k), lc.K_A, [0, 0, 0, 0, 0], grid))
    fs.sync()
    pool = MapPool(m, len(case["pool"]))
    pool.set(np.arange(len(case["pool"])), case["pool"])
    store = KeyFrameStore(pool, 2, N_FEAT, 0, 16)
    store.set(np.arange(2), np.zeros(2, np.uint8), [case["entries1"], case["entries2"]], [[], []], [-1, -1], [[], []])
    one = dict(fs=fs, slot1=0, slot2=1, kf1=0, kf2=1, n1=N_FEAT, n2=N_FEAT, R12=case["R12"], t12=case["t12"], s12=case["s12"],
               S12=(case["q"], case["t"], case["s"]), R1w=case["R1w"], t1w=case["t1w"], R2w=case["R2w"], t2w=case["t2w"], K1=case["K"], K2=case["K"],
               bounds1=case["bounds"], bounds2=case["bounds"], m12_id=case["m12_id"], m12_idx2=case["m12_idx2"])

    def search(to, uvr, level, qdesc):
        return m.window_best_frame(uvr, level, qdesc, None, frames[to - 1])

    def parent_way(J):
        items = [cc.model_run(None, case, search=search, solve=False)["item"] for _ in range(J)]
        return optimize_sim3_batch(m, items, sig, sig)

    def new_way(J):
        return compute_sim3_batch(m, pool, store, [one] * J, lc.SF, lc.SF, brk, brk, sig, sig)
    # the same results either way
    p0, n0 = parent_way(1)[0], new_way(1)[0]
    assert (p0["n_in"], p0["n_corr"], p0["n_bad"]) == (n0["n_in"], n0["n_corr"], n0["n_bad"]) and np.array_equal(p0["removed"], n0["removed"])
    assert all(np.asarray(p0[k]).tobytes() == np.asarray(n0[k]).tobytes() for k in ("iterations", "trials", "lambda_", "chi2"))
    rows = []
    for J in a.jobs:
        t_end = time.perf_counter() + 0.5
        while time.perf_counter() < t_end:
            new_way(J)
        parent_way(J)
        tp, tn = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter(); parent_way(J); t1 = time.perf_counter(); new_way(J); t2 = time.perf_counter()
            tp.append((t1 - t0) * 1e3); tn.append((t2 - t1) * 1e3)
        q = lambda v: [float(np.percentile(v, x)) for x in (50, 10, 90)]   # noqa: E731
        row = dict(jobs=J, features=N_FEAT, n_corr=n0["n_corr"], n_in=n0["n_in"], parent_way_ms=q(tp), compute_sim3_ms=q(tn), repeats=a.repeats)
        row["ratio"] = row["parent_way_ms"][0] / row["compute_sim3_ms"][0]
        rows.append(row)
        print("jobs %3d: parent %.3f ms [%.3f .. %.3f], compute_sim3 %.3f ms [%.3f .. %.3f], ratio %.2f" %
              (J, *row["parent_way_ms"], *row["compute_sim3_ms"], row["ratio"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/computesim3_bench.py", rows=rows), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
