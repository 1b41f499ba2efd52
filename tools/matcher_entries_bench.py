#!/usr/bin/env python3
"""Host-clock time of every matcher entry that ends in the rotation check, at 2 000 features a side (the cases of
tests/matcher_cases.py), check_ori on: median with 10th / 90th percentile over --repeats synchronising calls, one JSON row per
entry.  For A/B runs of two builds of the library (ORBSLAMM_HIP_LIB picks the other one), a fresh process per run:

    python tools/matcher_entries_bench.py --repeats 200 [--out rows.json]

bench.py's tracking_path and tools/tracking_bench.py time the frame-to-frame search in its pipeline; this times the entries alone."""
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
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from matcher_cases import make_bow_case, make_init_case, make_proj_case, make_tri_case, noisy_copies
    from vocab_cases import make_vocab
    from orbslamm_amd import ORBextractor, ORBmatcher, ORBVocabulary, make_grid
    n = a.features
    rng = np.random.default_rng(2000)
    base = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    q, t = noisy_copies(rng, base, 12), base[rng.permutation(n)]
    qa, ta = rng.uniform(0, 360, n).astype(np.float32), rng.uniform(0, 360, n).astype(np.float32)
    bow = make_bow_case(rng, n, n, 97)
    pc = make_proj_case(rng, n, n)
    ic = make_init_case(rng, n, n)
    tc = make_tri_case(rng, n, n, 60)
    tb = tc["c"]
    g, gi = make_grid(0.0, 0.0, pc["w"], pc["h"]), make_grid(0.0, 0.0, ic["w"], ic["h"])
    a0 = np.full(n, -1, np.int32)
    m = ORBmatcher(0.9, True, device=0)
    # a frame set of two frames from the initialisation case (F2 = F1 moved by a few pixels), with their BoW
    gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=1, device=0)   # (its handle owns the raw device buffers)
    voc = make_vocab(np.random.default_rng(5), 10, 4)
    G = ORBVocabulary(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=0)
    keys = np.stack([ic["k1"], ic["k2"]])
    desc = np.stack([ic["d1"], ic["d2"]])
    dk = gex.upload_frames(keys.view(np.uint8).reshape(1, 1, -1))[0]
    dd = gex.upload_frames(desc.reshape(1, 1, -1))[0]
    dc = gex.upload_frames(np.array([n, n], np.int32).view(np.uint8).reshape(1, 1, -1))[0]
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    fs = m.frame_set(2, n, [500.0, 500.0, 320.0, 240.0], [0, 0, 0, 0, 0], gi, [0.0, ic["w"], 0.0, ic["h"]], sf)
    fs.build(0, 2, dk, dd, dc, n)
    fs.compute_bow(G, 0, 2, 2)
    fs.sync()

    def track():
        fs.track([1], [0], th=15.0)
        return fs.results()[1][0]

    def set_bow():
        fs.search_by_bow([0], [1], nnratio=0.7, check_ori=True)
        return fs.bow_results()[1][0]

    def build():
        fs.build(0, 2, dk, dd, dc, n)
        fs.sync()
        return n

    calls = [
        ("match_bruteforce", lambda: m.match_bruteforce(q, qa, t, ta)[1]),
        ("search_by_bow", lambda: m.SearchByBoW(bow["qd"], bow["qa"], bow["qv"], bow["qfv"], bow["td"], bow["ta"], None, bow["tfv"], True)[1]),
        ("search_for_triangulation", lambda: m.SearchForTriangulation(tc["k1"], tb["qd"], 1 - tb["qv"], tb["qfv"], tc["k2"], tb["td"], 1 - tb["tv"], tb["tfv"],
                                                                       tc["F"], tc["ex"], tc["ey"], tc["sf2"], tc["sigma2"])[1]),
        ("search_for_initialization", lambda: m.SearchForInitialization(ic["q_xy"], 100.0, ic["k1"], ic["d1"], gi, ic["k2"], ic["d2"])[1]),
        ("search_by_projection mode 4", lambda: m.SearchByProjection(4, 100, pc["uvr"], pc["lvl"], pc["qd"], pc["qa"], pc["qv"], pc["qo"], g, pc["tk"], pc["td"],
                                                                     pc["occ"], a0)[2]),
        ("frame_set.build, 2 frames", build),
        ("frame_set.track", track),
        ("frame_set.search_by_bow", set_bow),
    ]
    rows = []
    for name, call in calls:
        for _ in range(10):
            found = call()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        row = dict(entry=name, features=n, matches=int(found), repeats=a.repeats, median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)),
                   p90_ms=float(np.percentile(ms, 90)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/matcher_entries_bench.py", library=os.environ.get("ORBSLAMM_HIP_LIB") or "orbslamm_amd/liborbslamm_hip.so", rows=rows), f, indent=1)
    fs.close(); m.close(); G.close(); gex.close()


if __name__ == "__main__":
    main()
