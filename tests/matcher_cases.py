"""Shared synthetic case builders for the matcher tests (CPU and GPU)."""
import numpy as np


def noisy_copies(rng, base, nflip):
    q = base.copy()
    for i in range(len(q)):
        for b in rng.integers(0, 256, nflip):
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    return q


def naive_bruteforce(q, qa, t, ta, nnratio, th_low, check_ori):
    """independent numpy re-derivation of the headline rule"""
    nq, nt = len(q), len(t)
    match = np.full(nq, -1, np.int32)
    if nt == 0:
        return match, 0
    tb = np.unpackbits(t, axis=1)
    bins = {}
    for i in range(nq):
        d = (np.unpackbits(q[i])[None, :] != tb).sum(axis=1)
        order = np.argsort(d, kind="stable")
        b1 = int(d[order[0]])
        b2 = int(d[order[1]]) if nt > 1 else 256
        if b1 <= th_low and np.float32(b1) < np.float32(nnratio) * np.float32(b2):
            match[i] = order[0]
            if check_ori:
                rot = np.float32(qa[i]) - np.float32(ta[order[0]])
                if rot < 0:
                    rot = np.float32(rot + np.float32(360.0))
                v = np.float32(rot * np.float32(1.0 / 30))
                b = int(np.floor(v + np.float32(0.5))) if v >= 0 else int(np.ceil(v - np.float32(0.5)))
                if b == 30:
                    b = 0
                bins.setdefault(b, []).append(i)
    if check_ori and bins:
        sizes = [len(bins.get(b, [])) for b in range(30)]
        m1 = m2 = m3 = 0
        i1 = i2 = i3 = -1
        for i, s in enumerate(sizes):
            if s > m1:
                m3, m2, m1 = m2, m1, s
                i3, i2, i1 = i2, i1, i
            elif s > m2:
                m3, m2 = m2, s
                i3, i2 = i2, i
            elif s > m3:
                m3, i3 = s, i
        if np.float32(m2) < np.float32(0.1) * np.float32(m1):
            i2 = i3 = -1
        elif np.float32(m3) < np.float32(0.1) * np.float32(m1):
            i3 = -1
        for b, lst in bins.items():
            if b not in (i1, i2, i3):
                for i in lst:
                    match[i] = -1
    return match, int((match >= 0).sum())


def make_bow_case(rng, nq, nt, nnodes):
    """KeyFrame (queries) vs Frame (trains) with synthetic FeatureVectors: features are
    spread over `nnodes` vocabulary nodes; some nodes exist on one side only."""
    n = max(nq, nt)
    base = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    qd = noisy_copies(rng, base[:nq], 10)
    perm = rng.permutation(nt)
    td = base[:nt][perm] if nt <= n else base
    node_of_base = rng.integers(0, nnodes, n)
    qnode = node_of_base[:nq].copy()
    tnode = node_of_base[:nt][perm].copy()
    # a few features land in side-only nodes
    qnode[rng.integers(0, nq, max(1, nq // 20))] = nnodes + 1
    tnode[rng.integers(0, nt, max(1, nt // 20))] = nnodes + 2

    def csr(node, count):
        ids = np.unique(node)
        start = [0]
        idx = []
        for i in ids:
            members = np.nonzero(node == i)[0]
            members = members[rng.permutation(len(members))]  # stored order is arbitrary
            idx.extend(members.tolist())
            start.append(len(idx))
        return (ids.astype(np.uint32) * 7 + 3, np.array(start, np.int32), np.array(idx, np.int32))

    qa = rng.uniform(0, 360, nq).astype(np.float32)
    ta = rng.uniform(0, 360, nt).astype(np.float32)
    inv = np.argsort(perm)
    for i in range(min(nq, nt)):
        ta[inv[i]] = np.float32((qa[i] + rng.normal(0, 4)) % 360)
    return dict(qd=qd, td=td, qa=qa, ta=ta, qv=(rng.uniform(size=nq) < 0.85).astype(np.uint8),
                tv=(rng.uniform(size=nt) < 0.9).astype(np.uint8), qfv=csr(qnode, nq), tfv=csr(tnode, nt))


def make_proj_case(rng, nq, nt, w=1241.0, h=376.0):
    """train frame with keypoints/grid, queries projected near some of them"""
    from oracle import binding as ob
    tk = np.zeros(nt, dtype=ob.KP_DTYPE)
    tk["x"] = rng.uniform(0, w, nt).astype(np.float32)
    tk["y"] = rng.uniform(0, h, nt).astype(np.float32)
    tk["octave"] = rng.integers(0, 8, nt)
    tk["angle"] = rng.uniform(0, 360, nt).astype(np.float32)
    td = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    src = rng.integers(0, nt, nq)
    qd = noisy_copies(rng, td[src], 14)
    uvr = np.zeros((nq, 3), np.float32)
    uvr[:, 0] = tk["x"][src] + rng.normal(0, 4, nq)
    uvr[:, 1] = tk["y"][src] + rng.normal(0, 4, nq)
    sf = np.float32(1.2) ** tk["octave"][src]
    uvr[:, 2] = (15.0 * sf).astype(np.float32)
    lvl = np.stack([tk["octave"][src] - 1, tk["octave"][src] + 1], axis=1).astype(np.int8)
    qa = (tk["angle"][src] + rng.normal(0, 5, nq)).astype(np.float32) % np.float32(360)
    gp = ob.make_grid_params(0.0, 0.0, w, h)
    start, idx = ob.grid_build(gp, tk)
    return dict(uvr=uvr, lvl=lvl, qd=qd, qa=qa, qv=(rng.uniform(size=nq) < 0.9).astype(np.uint8),
                qo=(rng.uniform(size=nq) < 0.7).astype(np.uint8), gp=gp, tk=tk, start=start, idx=idx, td=td,
                occ=(rng.uniform(size=nt) < 0.1).astype(np.uint8), w=w, h=h)


def make_init_case(rng, n1, n2, w=640.0, h=480.0):
    """two frames for SearchForInitialization: F2 = F1 shifted by a few pixels"""
    from oracle import binding as ob
    k1 = np.zeros(n1, dtype=ob.KP_DTYPE)
    k1["x"] = rng.uniform(20, w - 20, n1).astype(np.float32)
    k1["y"] = rng.uniform(20, h - 20, n1).astype(np.float32)
    k1["octave"] = (rng.uniform(size=n1) < 0.4) * rng.integers(1, 8, n1)  # 60 % on octave 0
    k1["angle"] = rng.uniform(0, 360, n1).astype(np.float32)
    d1 = rng.integers(0, 256, size=(n1, 32), dtype=np.uint8)
    src = rng.integers(0, n1, n2)
    k2 = np.zeros(n2, dtype=ob.KP_DTYPE)
    k2["x"] = np.clip(k1["x"][src] + rng.normal(0, 12, n2), 0, w - 1).astype(np.float32)
    k2["y"] = np.clip(k1["y"][src] + rng.normal(0, 12, n2), 0, h - 1).astype(np.float32)
    k2["octave"] = k1["octave"][src]
    k2["angle"] = ((k1["angle"][src] + rng.normal(0, 5, n2)) % 360).astype(np.float32)
    d2 = noisy_copies(rng, d1[src], 12)
    gp = ob.make_grid_params(0.0, 0.0, w, h)
    start, idx = ob.grid_build(gp, k2)
    q_xy = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, gp=gp, start=start, idx=idx, q_xy=q_xy, w=w, h=h)


def make_tri_case(rng, n1, n2, nnodes, w=640.0, h=480.0):
    """two keyframes related by a pure x-translation: F12 = [t]x, epipolar lines are image rows"""
    from oracle import binding as ob
    c = make_bow_case(rng, n1, n2, nnodes)
    k1 = np.zeros(n1, dtype=ob.KP_DTYPE)
    k2 = np.zeros(n2, dtype=ob.KP_DTYPE)
    k1["x"] = rng.uniform(0, w, n1).astype(np.float32)
    k1["y"] = rng.uniform(0, h, n1).astype(np.float32)
    k1["angle"] = c["qa"]
    k1["octave"] = rng.integers(0, 8, n1)
    k2["x"] = rng.uniform(0, w, n2).astype(np.float32)
    k2["y"] = rng.uniform(0, h, n2).astype(np.float32)
    k2["angle"] = c["ta"]
    k2["octave"] = rng.integers(0, 8, n2)
    # true correspondences (nearest descriptor) lie near the same row: noise partly inside,
    # partly outside the chi-square gate of the epipolar test
    lut = np.array([bin(i).count("1") for i in range(256)], np.uint8)
    for i in range(n1):
        d = lut[np.bitwise_xor(c["qd"][i][None, :], c["td"])].sum(axis=1)
        j = int(np.argmin(d))
        if d[j] <= 50:
            k2["y"][j] = np.float32(k1["y"][i] + rng.normal(0, 2.5))
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)  # l = (0, -1, y1): |y2 - y1| distance
    return dict(c=c, k1=k1, k2=k2, F=F, ex=np.float32(-5000.0), ey=np.float32(h / 2), sf2=sf, sigma2=(sf * sf).astype(np.float32))


# ------------------------------------------------------------------ rotation consistency, designed (ORBmatcher.cc:238-287)
# The parity cases above draw angles uniformly: every reachable bin fills about evenly, the 10 % rule never fires and a tie between
# bins is an accident of the seed.  Here every match lands in a chosen bin: per class the matches per bin (bins 0..12 -- with
# factor = 1/30 (sic) a rotation below 360 reaches no further), the features that match nothing, and whether the check prunes.
ROT_CLASSES = {
    "empty": ({}, 5, False),
    "one bin": ({4: 40}, 0, False),
    "one bin, 65": ({4: 65}, 0, False),                              # a second wave with one live lane in the count reduction
    "four equal": ({2: 20, 5: 20, 7: 20, 9: 20}, 0, True),          # the earliest three win
    "later larger": ({1: 10, 3: 20, 6: 30, 8: 40}, 0, True),        # the indices shift three times; bin 1 falls out
    "second at a tenth, 10": ({0: 10, 3: 1, 5: 1}, 0, None),        # None: the float compare decides, read from the oracle
    "second at a tenth, 100": ({0: 100, 3: 10, 5: 10}, 0, None),
    "second below a tenth": ({0: 100, 3: 9, 5: 9}, 0, True),        # second and third go
    "third below, second above": ({0: 100, 3: 50, 5: 9}, 0, True),
}


def oracle_three_maxima(oracle, h):
    """(ind1, ind2, ind3) of the oracle's orc_three_maxima for thirty counts"""
    import ctypes as C
    i = [C.c_int(), C.c_int(), C.c_int()]
    h = np.ascontiguousarray(h, np.int32)
    oracle.lib().orc_three_maxima(h.ctypes.data_as(C.c_void_p), 30, C.byref(i[0]), C.byref(i[1]), C.byref(i[2]))
    return tuple(v.value for v in i)


def rot_kept_bins(oracle, counts):
    """the bins ComputeThreeMaxima keeps for {bin: count}"""
    h = np.zeros(30, np.int32)
    for b, c in counts.items():
        h[b] = c
    return {v for v in oracle_three_maxima(oracle, h) if v >= 0}


def make_rot_case(oracle, name, w=640.0, h=480.0):
    """n distinct random descriptors and their exact copies as queries: every query matches its twin (same index) at distance 0
    and passes any ratio test; ta = 0 and qa = 30 * b put the match in bin b (checked with orc_rot_bin).  The features that are
    to match nothing carry the complement of their twin.  Everything an entry needs on top travels along: keypoints of octave 0
    on a 10-pixel lattice, the same place in both frames (SearchForInitialization's and the projection searches' windows hold
    the twin; SearchForTriangulation's epipolar line, a row, runs through it), the grid, FeatureVectors of three nodes."""
    counts, nomatch, prunes = ROT_CLASSES[name]
    rng = np.random.default_rng(sorted(ROT_CLASSES).index(name) + 2024)
    bins = np.array([b for b, c in counts.items() for _ in range(c)] + [-1] * nomatch, np.int32)
    bins = bins[rng.permutation(len(bins))]
    n = len(bins)
    td = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    assert len({r.tobytes() for r in td}) == n
    qd = np.where((bins < 0)[:, None], ~td, td)
    qa = (np.float32(30.0) * np.maximum(bins, 0)).astype(np.float32)
    ta = np.zeros(n, np.float32)
    L = oracle.lib()
    assert all(L.orc_rot_bin(float(qa[i]), 0.0) == bins[i] for i in range(n) if bins[i] >= 0)
    cell = rng.permutation(60 * 44)[:n]
    k1 = np.zeros(n, dtype=oracle.KP_DTYPE)
    k1["x"] = (20 + 10 * (cell % 60)).astype(np.float32)
    k1["y"] = (20 + 10 * (cell // 60)).astype(np.float32)
    k1["size"] = 31.0
    k2 = k1.copy()
    k1["angle"] = qa
    node = np.arange(n) % 3
    ids = np.unique(node)
    idx = np.concatenate([np.nonzero(node == i)[0] for i in ids]).astype(np.int32) if n else np.zeros(0, np.int32)
    start = np.concatenate([[0], np.cumsum([(node == i).sum() for i in ids])]).astype(np.int32)
    fv = (ids.astype(np.uint32) * 7 + 3, start, idx)
    gp = oracle.make_grid_params(0.0, 0.0, w, h)
    gstart, gidx = oracle.grid_build(gp, k2)
    kept = rot_kept_bins(oracle, counts)
    if prunes is not None:
        assert prunes == bool(set(counts) - kept), name
    return dict(name=name, n=n, bins=bins, kept=kept, qd=qd, td=td, qa=qa, ta=ta, k1=k1, k2=k2, fv=fv, w=w, h=h, gp=gp, start=gstart, idx=gidx,
                q_xy=np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32),
                uvr=np.stack([k1["x"], k1["y"], np.full(n, 15.0, np.float32)], axis=1).astype(np.float32),
                lvl=np.tile(np.array([[-1, 1]], np.int8), (n, 1)),
                F=np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32), ex=np.float32(-5000.0), ey=np.float32(h / 2),
                sf2=np.ones(8, np.float32), sigma2=np.ones(8, np.float32))


def rot_oracle_entries(oracle, c):
    """name -> call(check_ori) -> (match table, count): the oracle entries behind every device entry that takes caller angles.
    Tables are by query except the projection search's (by train feature); twins share their index, so either reads alike."""
    z8, m1 = np.zeros(c["n"], np.uint8), np.full(c["n"], -1, np.int32)
    return {
        "match_bruteforce": lambda ori: oracle.match_bruteforce(c["qd"], c["qa"], c["td"], c["ta"], 0.7, 50, ori),
        "search_by_bow": lambda ori: oracle.search_by_bow(c["qd"], c["qa"], None, c["fv"], c["td"], c["ta"], None, c["fv"], 0.7, ori, True),
        "search_for_triangulation": lambda ori: oracle.search_for_triangulation(c["k1"], c["qd"], z8, c["fv"], c["k2"], c["td"], z8, c["fv"], c["F"], c["ex"],
                                                                               c["ey"], c["sf2"], c["sigma2"], False, ori),
        "search_for_initialization": lambda ori: oracle.search_for_initialization(c["q_xy"], 30.0, c["k1"], c["qd"], c["gp"], c["k2"], c["start"], c["idx"],
                                                                                 c["td"], 0.9, ori),
        "search_by_projection": lambda ori: (lambda r: (r[0], r[2]))(oracle.search_by_projection(4, 0.9, ori, 100, c["uvr"], c["lvl"], c["qd"], c["qa"], None, None,
                                                                                                c["gp"], c["k2"], c["start"], c["idx"], c["td"], z8, m1)),
    }


def assert_rot_case_is_designed(c, free, checked):
    """`free` / `checked`: an entry's (table, count) without and with the rotation check.  Without it every designed match is
    there; with it exactly the matches outside the kept bins are gone -- none where the class keeps everything."""
    (m0, n0), (m1, n1) = free, checked
    matched = c["bins"] >= 0
    assert np.array_equal(m0[:c["n"]] >= 0, matched) and n0 == matched.sum(), c["name"]
    assert np.array_equal(m0[:c["n"]][matched], np.nonzero(matched)[0])   # every match is the twin
    stays = matched & np.isin(c["bins"], sorted(c["kept"]))
    assert np.array_equal(m1[:c["n"]] >= 0, stays) and n1 == stays.sum(), c["name"]
    assert np.array_equal(m1[:c["n"]][stays], m0[:c["n"]][stays])
    assert bool((matched & ~stays).sum()) == bool(set(b for b in c["bins"] if b >= 0) - c["kept"])
