"""Keyframe database latency and throughput on the device against the C++ restatement on one host core.

  python tools/kfdb_bench.py [--sizes 100,1000,10000] [--queries 30] [--out profiles/kfdb_bench.json]

Synthetic k=10, L=6 vocabulary (10^6 words), keyframes of 1000 features (BowVectors of ~1000 words drawn around
places, so that keyframes of a place share words), covisibility: up to 10 keyframes of the same place.  Reports the
median latency of one DetectRelocalizationCandidates and one DetectLoopCandidates per database size (host call to
result, neighbours from the pool's table), and detect_loop_batch throughput for a 200-keyframe map against a
2000-keyframe database.  The CPU side (tools/kfdb_cpu_bench.cpp over tools/kfdb_ref.hpp, built here with g++ -O2) runs
the same query sequence on the same scene; its candidate lists must equal the device's ("parity")."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flat_vocab(k=10, L=6):
    """a full k-ary tree of depth L in loadFromTextFile order (breadth first); descriptors random, weights 1"""
    # node ids: root 0, level 1 = 1..k, level d starts after the previous levels
    parent = []
    start_prev, n_prev, nid = 0, 1, 1
    for lvl in range(L):
        parent.append(np.repeat(np.arange(start_prev, start_prev + n_prev, dtype=np.int32), k))
        start_prev, n_prev = nid, n_prev * k
        nid += n_prev
    parent = np.concatenate(parent)
    n = parent.shape[0]
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[n - k ** L:] = 1
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return parent, is_leaf, desc, np.ones(n), k ** L


def scene(rng, n_kf, n_words, nw=1000, per_place=10):
    places = max(2, n_kf // per_place)
    pw = [rng.choice(n_words, 2 * nw, replace=False) for _ in range(places)]
    place = rng.integers(0, places, n_kf)

    def bow(p):
        w = np.union1d(rng.choice(pw[p], int(nw * 0.8), replace=False), rng.integers(0, n_words, nw // 5))
        v = rng.uniform(0.05, 3.0, w.shape[0])
        return w.astype(np.uint32), v / v.sum()
    bows = [bow(int(place[i])) for i in range(n_kf)]
    by = {}
    for i in range(n_kf):
        by.setdefault(int(place[i]), []).append(i)
    covis = [[j for j in by[int(place[i])] if j != i][:10] for i in range(n_kf)]
    return bows, covis, place, bow, places


def write_scene(path, n_words, members, bows, covis, queries):
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", len(bows), n_words, members))
        for ids, vals in bows:
            f.write(struct.pack("<i", ids.shape[0]) + ids.tobytes() + vals.astype(np.float64).tobytes())
        for c in covis:
            f.write(struct.pack("<i", len(c)) + np.asarray(c, np.int32).tobytes())
        for q in queries:
            if q[0] == 0:
                _, qid, (ids, vals) = q
                f.write(struct.pack("<iQi", 0, qid, ids.shape[0]) + ids.tobytes() + vals.astype(np.float64).tobytes())
            else:
                _, qid, s, ms, conn = q
                f.write(struct.pack("<iQif", 1, qid, s, ms) + struct.pack("<i", len(conn)) + np.asarray(conn, np.int32).tobytes())


def cpu_run(exe, path):
    out = path + ".out"
    subprocess.check_call([exe, path, out])
    rows = []
    for line in open(out):
        p = line.split()
        rows.append((int(p[0]), float(p[1]), [int(x) for x in p[2:]]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--queries", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orbslamm_amd import KeyFrameDatabase, KeyFramePool, ORBVocabulary
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "kfdb_cpu_bench")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I", os.path.join(ROOT, "tools"), os.path.join(ROOT, "tools", "kfdb_cpu_bench.cpp"), "-o", exe])
    parent, is_leaf, desc, weight, n_words = flat_vocab()
    G = ORBVocabulary(10, 6, 0, 0, parent, is_leaf, desc, weight, device=0)
    rng = np.random.default_rng(7)
    rec = dict(vocabulary="k=10 L=6 (10^6 words)", features_per_keyframe=1000, neighbours="pool covisibility table", single=[], parity=True)
    nq = a.queries
    for n in [int(x) for x in a.sizes.split(",")]:
        bows, covis, place, bow, places = scene(rng, n, n_words)
        pool = KeyFramePool(G, n)
        for i, (ids, vals) in enumerate(bows):
            pool.set_bow(i, ids, vals)
        for i in range(n):
            pool.set_covisibility(i, covis[i])
        db = KeyFrameDatabase(pool)
        for i in range(n):
            db.add(i)
        queries = []
        for t in range(nq):   # fresh ids: every query a new frame / keyframe
            queries.append((0, 1000 + t, bow(int(rng.integers(0, places)))))
        for t in range(nq):
            s = int(rng.integers(0, n))
            queries.append((1, 5000 + t, s, np.float32(0.01), covis[s][:4]))
        dev, lat = [], {0: [], 1: []}
        for q in queries:
            t0 = time.perf_counter()
            if q[0] == 0:
                c = db.DetectRelocalizationCandidates(q[1], bow=q[2])
            else:
                c = db.DetectLoopCandidates(q[2], q[1], q[3], q[4])
            lat[q[0]].append((time.perf_counter() - t0) * 1e6)
            dev.append(c)
        path = os.path.join(tmp, "scene_%d.bin" % n)
        write_scene(path, n_words, n, bows, covis, queries)
        cpu = cpu_run(exe, path)
        par = [r[2] for r in cpu] == dev
        rec["parity"] = rec["parity"] and par
        cl = {0: [r[1] for r in cpu if r[0] == 0], 1: [r[1] for r in cpu if r[0] == 1]}
        # the first queries of a size load code objects and grow the scratch: the median of the rest
        row = dict(keyframes=n, queries_each=nq, parity=par,
                   gpu_reloc_us_median=float(np.median(lat[0][3:])), gpu_loop_us_median=float(np.median(lat[1][3:])),
                   cpu_reloc_us_median=float(np.median(cl[0][3:])), cpu_loop_us_median=float(np.median(cl[1][3:])),
                   candidates_mean=float(np.mean([len(c) for c in dev])))
        rec["single"].append(row)
        print(json.dumps(row), flush=True)
        db.close()
        pool.close()
    # MultiMapper's scan: a 200-keyframe map against a 2000-keyframe database
    n_old, n_new = 2000, 200
    bows, covis, place, bow, places = scene(rng, n_old + n_new, n_words)
    pool = KeyFramePool(G, n_old + n_new)
    for i, (ids, vals) in enumerate(bows):
        pool.set_bow(i, ids, vals)
    for i in range(n_old + n_new):
        pool.set_covisibility(i, covis[i])
    db = KeyFrameDatabase(pool)
    for i in range(n_old):
        db.add(i)
    slots = list(range(n_old + n_new - 1, n_old - 1, -1))
    conn = [covis[s][:4] for s in slots]
    runs = []
    out = None
    for r in range(4):   # (run 0 warms up; every run a new cycle of ids, as MultiMapper's next cycle)
        ids = [100000 * (r + 1) + s for s in slots]
        t0 = time.perf_counter()
        out = db.detect_loop_batch(slots, ids, conn, [covis[s] for s in slots])
        runs.append(time.perf_counter() - t0)
    batch_s = float(np.median(runs[1:]))
    # the same scan as single queries (minScore through orbk_pool_score) on the device, and on the CPU
    t0 = time.perf_counter()
    for q, s in enumerate(slots):
        ms = np.float32(pool.score(s, covis[s]).min(initial=np.float32(1.0)))
        db.DetectLoopCandidates(s, 900000 + s, ms, conn[q])
    single_s = time.perf_counter() - t0
    queries = []
    for s in slots:
        ms = np.float32(pool.score(s, covis[s]).min(initial=np.float32(1.0)))
        queries.append((1, 500000 + s, s, ms, covis[s][:4]))
    path = os.path.join(tmp, "scene_batch.bin")
    write_scene(path, n_words, n_old, bows, covis, queries)
    cpu = cpu_run(exe, path)
    cpu_s = sum(r[1] for r in cpu) * 1e-6
    rec["batch"] = dict(map_keyframes=n_new, database_keyframes=n_old, gpu_batch_ms=batch_s * 1e3, gpu_batch_queries_per_s=n_new / batch_s,
                        gpu_single_queries_ms=single_s * 1e3, cpu_queries_ms=cpu_s * 1e3, cpu_queries_per_s=n_new / cpu_s,
                        candidates_total=int(sum(len(c) for c in out)))
    print(json.dumps(rec["batch"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(dict(parity=rec["parity"])))


if __name__ == "__main__":
    main()
