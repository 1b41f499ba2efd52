"""Designed scenes for the window searches of the matcher: SearchByProjection modes 3 - 6, window_best, SearchForInitialization and
SearchForTriangulation (oracle/orb_match.c; the census counters of oracle.binding.MATCH_BRANCHES say which branch a scene reaches).

How a scene is made.  A 640 x 480 frame with the 64 x 48 grid (cells of 10 pixels).  Features come in GROUPS, each around its own centre
on a 40-pixel lattice: a group's windows reach at most 16 pixels from its centre and its features lie within 12, so a group only ever
sees itself.  Every group has its own random base descriptor; a query flips its first `a` bits of the low half, a train feature its
first `b` bits of the high half, so inside a group the Hamming distance is exactly a + b (across groups it is about 128, and geometry
keeps those pairs apart).  Queries sit at chosen indices; the gaps are filled with queries whose window lies wholly outside the grid,
one side after the other -- so the matching queries are interleaved with those.

Candidate order is cell-major (column outer, row inner, then insertion): where "the first of equals" matters the feature that comes
first in that order is ADDED LATER, so it carries the higher index."""
import numpy as np

W, H = 640.0, 480.0
SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)                    # mvScaleFactors
SIGMA2 = (SF * SF).astype(np.float32)                                         # mvLevelSigma2
INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(8)) ** 2).astype(np.float32)   # as the parity tests make mvInvLevelSigma2
OUTSIDE = ((-50.0, 100.0), (700.0, 100.0), (100.0, -50.0), (100.0, 540.0))    # a 10-pixel window there is off the grid: left, right, top, bottom


def f32(x):
    return np.float32(x)


def up(x, n=1):
    """n binary32 steps above x"""
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(np.inf))
    return x


def down(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(-np.inf))
    return x


def adjacent(passes, a, b):
    """two neighbouring positive binary32 values (p, f) between a and b with passes(p) and not passes(f); passes(a), not passes(b)"""
    a, b = f32(a), f32(b)
    assert a > 0 and b > 0 and passes(a) and not passes(b)
    ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
    while abs(ia - ib) > 1:
        m = (ia + ib) // 2
        if passes(np.int32(m).view(np.float32)):
            ia = m
        else:
            ib = m
    return np.int32(ia).view(np.float32), np.int32(ib).view(np.float32)


class Scene:
    """trains and queries of one search, by groups"""

    def __init__(self, seed, reserved=()):
        """reserved: query indices that only an explicit `at` may take"""
        self.reserved = set(reserved)
        self.rng = np.random.default_rng(seed)
        self.t, self.q, self.bases, self.ngroups = [], {}, [], 0
        self.roles = {}   # name -> query index, for the tests that state an expectation in words

    def group(self):
        """centre of the next lattice group and its id"""
        g = self.ngroups
        self.ngroups += 1
        assert g < 15 * 11
        return self.base(), f32(30 + 40 * (g % 15)), f32(30 + 40 * (g // 15))

    def base(self):
        self.bases.append(self.rng.integers(0, 256, 32, dtype=np.uint8))
        return len(self.bases) - 1

    def train(self, gid, x, y, b, octave=0, angle=0.0, uright=-1.0, occ=0, assign=-1, invert=False):
        """invert: the complement of that descriptor (b = 0: at 256 from a query with a = 0)"""
        self.t.append(dict(g=gid, x=f32(x), y=f32(y), b=b, octave=octave, angle=f32(angle), ur=f32(uright), occ=occ, assign=assign, inv=invert))
        return len(self.t) - 1

    def query(self, gid, u, v, r, a=0, lvl=(-1, -1), at=None, angle=0.0, valid=1, obs=1, ur=0.0, octave=0, pred=0, key=None, role=None):
        """at: the query's index (None: the lowest free one).  octave / key: the query KEYPOINT (SearchForInitialization); pred: window_best"""
        if at is None:
            at = 0
            while at in self.q or at in self.reserved:
                at += 1
        assert at not in self.q
        self.q[at] = dict(g=gid, u=f32(u), v=f32(v), r=f32(r), a=a, lvl=lvl, angle=f32(angle), valid=valid, obs=obs, ur=f32(ur), octave=octave, pred=pred,
                          key=key if key is not None else (f32(u), f32(v)))
        if role:
            self.roles[role] = at
        return at

    def _desc(self, gid, n, high):
        d = np.unpackbits(self.bases[gid])
        assert 0 <= n <= 128
        d[128 * high:128 * high + n] ^= 1
        return np.packbits(d)

    def finish(self, oracle, nq=None, radius=10.0):
        """the arrays every entry takes.  Free query indices below nq are filled with queries off the grid."""
        nq = max(self.q) + 1 if nq is None and self.q else (nq or 0)
        filler = self.base()
        for i in range(nq):
            if i not in self.q:
                x, y = OUTSIDE[i % 4]
                self.query(filler, x, y, radius, at=i, octave=0)
        nt = len(self.t)
        tk = np.zeros(nt, dtype=oracle.KP_DTYPE)
        td = np.zeros((nt, 32), np.uint8)
        for i, t in enumerate(self.t):
            tk[i]["x"], tk[i]["y"], tk[i]["octave"], tk[i]["angle"], tk[i]["size"] = t["x"], t["y"], t["octave"], t["angle"], 31.0
            td[i] = ~self._desc(t["g"], t["b"], 1) if t["inv"] else self._desc(t["g"], t["b"], 1)
        qs = [self.q[i] for i in range(nq)]
        qk = np.zeros(nq, dtype=oracle.KP_DTYPE)
        qd = np.zeros((nq, 32), np.uint8)
        for i, q in enumerate(qs):
            qk[i]["x"], qk[i]["y"], qk[i]["octave"], qk[i]["angle"], qk[i]["size"] = q["key"][0], q["key"][1], q["octave"], q["angle"], 31.0
            qd[i] = self._desc(q["g"], q["a"], 0)
        gp = oracle.make_grid_params(0.0, 0.0, W, H)
        start, idx = oracle.grid_build(gp, tk)
        col = lambda k, dt: np.array([q[k] for q in qs], dt)
        return dict(nq=nq, nt=nt, tk=tk, td=td, gp=gp, start=start, idx=idx, qk=qk, qd=qd,
                    uvr=np.array([[q["u"], q["v"], q["r"]] for q in qs], np.float32).reshape(nq, 3),
                    lvl=np.array([q["lvl"] for q in qs], np.int8).reshape(nq, 2), qa=col("angle", np.float32), qv=col("valid", np.uint8),
                    qo=col("obs", np.uint8), q_ur=col("ur", np.float32), pred=col("pred", np.int8),
                    t_ur=np.array([t["ur"] for t in self.t], np.float32), occ=np.array([t["occ"] for t in self.t], np.uint8),
                    assign0=np.array([t["assign"] for t in self.t], np.int32), roles=dict(self.roles), w=W, h=H,
                    qg=col("g", np.int32), tg=np.array([t["g"] for t in self.t], np.int32))


# ------------------------------------------------------------------ window geometry (every entry that gathers candidates)
LEVEL_WINDOWS = ((-1, -1), (0, -1), (0, 0), (-1, 0), (3, 5), (7, 8))


def add_window_geometry(S, r=8.0, lvl=(-1, -1), octave=0, angle=0.0, levels=True):
    """lvl / octave: what a plain query and a plain train feature of the entry carry (SearchForInitialization: (0, 0) and 0)"""
    q = dict(lvl=lvl, angle=angle)
    # a train feature at exactly x +- r / y +- r (excluded; it would be the best) and its neighbour one step inside (included)
    for k, (dx, dy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        g, cx, cy = S.group()
        ex, ey = cx + f32(dx * r), cy + f32(dy * r)
        inx = (down(ex) if dx > 0 else up(ex)) if dx else cx
        iny = (down(ey) if dy > 0 else up(ey)) if dy else cy
        S.train(g, ex, ey, 5, octave)
        S.train(g, inx, iny, 10, octave)
        S.train(g, cx, cy, 40, octave)
        S.query(g, cx, cy, r, role="edge %d" % k, **q)
    # windows cut by each border, a feature inside the part that is left
    for k, (x, y) in enumerate(((3.0, 150.0), (637.0, 150.0), (150.0, 3.0), (150.0, 476.0))):
        g = S.base()
        S.train(g, np.clip(x, 1, 633), np.clip(y, 1, 473), 12, octave)
        S.query(g, x, y, 10.0, role="cut %d" % k, **q)
    # PosInGrid drops what rounds to col == cols or row == rows: the dropped feature would be the best
    for k, (x, y, tx, ty) in enumerate(((631.0, 250.0, 636.0, 250.0), (250.0, 471.0, 250.0, 476.0))):
        g = S.base()
        S.train(g, tx, ty, 5, octave)
        S.train(g, x, y, 30, octave)
        S.query(g, x, y, 10.0, role="dropped %d" % k, **q)
    # one cell with 70 features (the best is the 68th), empty cells all around it in the same window
    g, cx, cy = S.group()
    for k in range(70):
        S.train(g, cx + f32(0.05 * k), cy + f32(0.03 * (k % 7)), 12 if k == 67 else 30 + k % 40, octave)
    S.query(g, cx, cy, 10.0, role="crowded", **q)
    if levels:
        # every level window over the same five octaves; the nearest descriptor sits on the octave fewest windows admit
        for lo_hi in LEVEL_WINDOWS:
            g, cx, cy = S.group()
            for k, (o, b) in enumerate(((0, 30), (3, 24), (4, 18), (6, 12), (7, 6))):
                S.train(g, cx - 6 + 3 * k, cy, b, o)
            S.query(g, cx, cy, 10.0, lvl=lo_hi, angle=angle, role="levels %d,%d" % lo_hi)


# ------------------------------------------------------------------ SearchByProjection
RATIO_PAIRS = ((39, 50), (40, 50), (41, 50), (44, 50), (45, 50), (46, 50), (29, 40), (30, 40), (31, 40))


def make_proj_scene(oracle, mode, th, stereo=False, rot=False):
    """mode / th: where the thresholds lie.  stereo: the families of the right-coordinate gate on top (q_ur, t_uright).  rot: queries
    carry designed angles (modes 4 / 5 with the rotation check).  Some features are occupied and some assign entries set on entry
    (`occ`, `assign0`; a frame set starts its table at -1 and takes the occupancy alone)."""
    nq = 150
    S = Scene(1000 + 10 * mode + th, reserved=(0, 1, 62, 63, 64, 65, 66, nq - 1))
    pruned, kept2 = 270.0, 90.0   # bins 9 and 3 (30 * bin, train angle 0): a handful of matches against a crowd in bin 0
    add_window_geometry(S)
    # ---- selection
    g, cx, cy = S.group(); S.train(g, cx, cy, th); S.query(g, cx, cy, 8, role="at th")
    g, cx, cy = S.group(); S.train(g, cx, cy, th + 1); S.query(g, cx, cy, 8, role="th + 1")
    g, cx, cy = S.group(); S.train(g, cx, cy, th - 20); S.query(g, cx, cy, 8, a=20, role="at th, both sides flipped")
    for name, o2 in (("tie same level", 0), ("tie cross level", 1)):
        g, cx, cy = S.group()
        S.train(g, cx + 6, cy, 20, o2)      # later in candidate order, lower index
        S.train(g, cx - 6, cy, 20, 0)       # first in candidate order
        S.query(g, cx, cy, 8, lvl=(0, 1), role=name)
    for b1, b2 in RATIO_PAIRS:
        for o2 in (0, 1):
            g, cx, cy = S.group()
            S.train(g, cx + 6, cy, b2, o2)
            S.train(g, cx - 6, cy, b1, 0)
            S.query(g, cx, cy, 8, lvl=(0, 1), role="ratio %d/%d %s" % (b1, b2, "same" if o2 == 0 else "cross"))
    g, cx, cy = S.group()   # a second at the runner-up's distance
    for k, b in enumerate((10, 20, 20)):
        S.train(g, cx - 6 + 6 * k, cy, b)
    S.query(g, cx, cy, 8, role="equal seconds")
    g, cx, cy = S.group(); S.train(g, cx, cy, 10); S.query(g, cx, cy, 8, valid=0, role="invalid")
    # the only other candidate lies at 256: `dist < bestDist2` never records it, so there is no second and no ratio to fail
    g, cx, cy = S.group(); S.train(g, cx - 6, cy, 0, invert=True); S.train(g, cx + 6, cy, min(th, 60)); S.query(g, cx, cy, 8, role="second at 256")
    # ---- serial dependence: q0 takes A; q63 preferred A, takes B; q64 preferred B, takes C; ... the last query takes E
    g, cx, cy = S.group()
    for k in range(5):
        S.train(g, cx - 12 + 6 * k, cy, 10 + 2 * k)
    S.query(g, cx - 12, cy, 3, at=0, role="chain 0")
    for k, at in enumerate((63, 64, 65, nq - 1)):
        S.query(g, cx - 9 + 6 * k, cy, 4, at=at, role="chain %d" % (k + 1))
    # the same chain with members that do not block (modes 3 / 4: everybody takes the feature it prefers)
    g, cx, cy = S.group()
    for k in range(3):
        S.train(g, cx - 6 + 6 * k, cy, 10 << k)   # (10, 20, 40: the preferred one also passes mode 3's ratio rule)
    S.query(g, cx - 6, cy, 3, at=1, obs=0, role="free chain 0")
    S.query(g, cx - 3, cy, 4, at=62, obs=0, role="free chain 1")
    S.query(g, cx + 3, cy, 4, at=66, obs=1, role="free chain 2")
    # a feature taken twice (q_obs_pos 0 first): both bins pruned, both kept, the first pruned and the second kept, and the reverse
    for name, a1, a2 in (("pruned", pruned, pruned), ("kept", 0.0, 0.0), ("first pruned", pruned, 0.0), ("second pruned", 0.0, pruned)):
        g, cx, cy = S.group()
        S.train(g, cx - 6, cy, 10)
        S.train(g, cx + 6, cy, 20)
        S.query(g, cx, cy, 8, obs=0, angle=a1 if rot else 0.0, role="retake first, " + name)
        S.query(g, cx, cy, 8, obs=1, angle=a2 if rot else 0.0, role="retake second, " + name)
    if rot:   # bin 3 holds a third of a bin-0 crowd (kept), bin 9 a handful (below a tenth of bin 0: pruned)
        for k in range(60):
            g, cx, cy = S.group()
            S.train(g, cx, cy, 10 + k % 30)
            S.query(g, cx, cy, 6, angle=kept2 if k % 4 == 0 else 0.0)
        g, cx, cy = S.group(); S.train(g, cx, cy, 10); S.query(g, cx, cy, 6, angle=pruned, role="lone pruned")
    # ---- state on entry
    g, cx, cy = S.group()
    S.train(g, cx - 6, cy, 5, occ=1, assign=7)      # occupied: the entry survives, the query takes the other
    S.train(g, cx + 6, cy, 20, assign=9)            # overwritten
    S.train(g, cx, cy + 10, 1, assign=11)           # outside the window: untouched
    S.query(g, cx, cy, 8, role="occupied on entry")
    g, cx, cy = S.group(); S.train(g, cx, cy, 5, occ=1); S.query(g, cx, cy, 8, role="none free")
    if stereo:
        # |q_ur - t_uright| == r (kept), one step beyond (skipped; it would be the best), within; t_uright 0 and -1 are not gated
        for name, tur, qur, b in (("at r", 100.0, 108.0, 10), ("beyond r", 100.0, up(108.0), 10), ("within r", 100.0, 104.0, 10),
                                  ("uright 0", 0.0, 500.0, 10), ("uright -1", -1.0, 500.0, 10)):
            g, cx, cy = S.group()
            S.train(g, cx - 6, cy, b, uright=tur)
            S.train(g, cx + 6, cy, 30, uright=-1.0)
            S.query(g, cx, cy, 8, ur=qur, role="stereo " + name)
    return S.finish(oracle, nq=nq)


# ------------------------------------------------------------------ window_best
def _chi2_mono(u, tx, o):
    ex = f32(u) - f32(tx)
    e2 = f32(f32(ex * ex) + f32(0.0))
    return not float(f32(e2 * INV_SIGMA2[o])) > 5.99


def _chi2_stereo(qur, tur, o):
    er = f32(qur) - f32(tur)
    e2 = f32(f32(f32(0.0) + f32(0.0)) + f32(er * er))
    return not float(f32(e2 * INV_SIGMA2[o])) > 7.8


def make_window_scene(oracle, stereo):
    """window_best: pred 0 and 7 with octaves from pred - 2 to pred + 1, the chi-square gates at their edge per octave, t_uright 0 / -1,
    no candidate, ties.  stereo False: nothing carries a right coordinate (window_best_frame runs the same scene)."""
    S = Scene(2000 + stereo, reserved=range(2, 400, 5))   # (every fifth query is one off the grid)
    add_window_geometry(S, levels=False)
    for pred in (0, 3, 7):
        # the nearest descriptors sit outside [pred - 1, pred]
        g, cx, cy = S.group()
        for k, (o, b) in enumerate(((pred - 2, 5), (pred - 1, 30), (pred, 20), (pred + 1, 6))):
            if 0 <= o <= 7:
                S.train(g, cx - 6 + 4 * k, cy, b, o)
        S.query(g, cx, cy, 10, pred=pred, role="pred %d" % pred)
        g, cx, cy = S.group()   # only pred - 1 in the window
        if pred:
            S.train(g, cx, cy, 15, pred - 1)
            S.query(g, cx, cy, 10, pred=pred, role="pred %d, below only" % pred)
    g, cx, cy = S.group(); S.train(g, cx, cy, 15, 2); S.query(g, cx, cy, 10, pred=0, role="no level fits")
    g, cx, cy = S.group(); S.query(g, cx, cy, 10, role="empty window")
    g, cx, cy = S.group(); S.train(g, cx, cy, 15); S.query(g, cx, cy, 10, valid=0, role="invalid")
    g, cx, cy = S.group()
    S.train(g, cx + 6, cy, 20)
    S.train(g, cx - 6, cy, 20)
    S.query(g, cx, cy, 8, role="tie")
    g, cx, cy = S.group()   # the same half a pixel either side of the query and of a cell border: both pass the chi-square gates
    S.train(g, cx + 5.5, cy, 20)
    S.train(g, cx + 4.5, cy, 20)
    S.query(g, cx + 5, cy, 8, ur=50.0, role="tie inside the gate")
    for o in range(8):   # mono gate: the feature one step outside 5.99 would be the best
        g, cx, cy = S.group()
        p, f = adjacent(lambda tx: _chi2_mono(cx, tx, o), cx + 1, cx + 12)
        S.train(g, f, cy, 5, o)
        S.train(g, p, cy, 10, o)
        S.query(g, cx, cy, 14, pred=o, role="chi2 mono %d" % o)
    if stereo:
        for o in (0, 3, 7):   # stereo gate at 7.8: all of the error in the right coordinate
            g, cx, cy = S.group()
            p, f = adjacent(lambda tur: _chi2_stereo(50.0, tur, o), 49.0, 38.0)
            S.train(g, cx, cy, 5, o, uright=f)
            S.train(g, cx, up(cy), 10, o, uright=p)
            S.query(g, cx, cy, 14, pred=o, ur=50.0, role="chi2 stereo %d" % o)
        # t_uright exactly 0 is a right coordinate here (>= 0): judged with q_ur = 500 it fails; -1 is mono and passes
        for name, tur in (("uright 0", 0.0), ("uright -1", -1.0)):
            g, cx, cy = S.group()
            S.train(g, cx, cy, 5, uright=tur)
            S.train(g, cx + 1, cy, 30, uright=-1.0)
            S.query(g, cx, cy, 8, ur=500.0, role="chi2 " + name)
    return S.finish(oracle, nq=max(S.q) + 2)


# ------------------------------------------------------------------ SearchForInitialization
def make_init_scene(oracle, window=10.0):
    nq = 140
    S = Scene(3000, reserved=[3, 70] + list(range(7, nq, 9)))
    pruned, kept2 = 270.0, 90.0
    q = dict(lvl=(0, 0))
    add_window_geometry(S, r=window, lvl=(0, 0), levels=False)

    def two(name, qs, ts):
        """qs: (a, index or None, angle) in query order; ts: b per train feature; every query sees every feature of the group"""
        g, cx, cy = S.group()
        for k, b in enumerate(ts):
            S.train(g, cx - 4 + 4 * k, cy, b)
        for k, (a, at, ang) in enumerate(qs):
            S.query(g, cx, cy, window, a=a, at=at, angle=ang, role="%s %d" % (name, k), **q)
    two("steal", ((10, None, 0.0), (0, None, 0.0)), (10,))                                   # 20, then 10: the thief wins
    two("held better", ((0, None, 0.0), (10, None, 0.0)), (10,))                             # 10, then 20: the holder keeps it
    two("equal", ((10, None, 0.0), (10, None, 0.0)), (10, 40))                               # 20, then 20 again: skipped, takes the other at 50
    two("chain", ((20, None, 0.0), (10, None, 0.0), (0, None, 0.0)), (10, 30))               # A at 30, stolen at 20, stolen at 10
    two("stride", ((10, 3, 0.0), (0, 70, 0.0)), (10,))                                       # thief 67 queries after its victim
    two("victim pruned", ((10, None, pruned), (0, None, 0.0)), (10,))                        # the victim's push lies in a pruned bin
    two("victim kept", ((10, None, 0.0), (0, None, pruned)), (10,))                          # ... in a kept one, the thief's is pruned
    two("at 50", ((0, None, 0.0),), (50,))
    two("at 51", ((0, None, 0.0),), (51,))
    for b1, b2 in RATIO_PAIRS:
        two("ratio %d/%d" % (b1, b2), ((0, None, 0.0),), (b1, b2))
    two("equal best", ((0, None, 0.0),), (20, 20))
    # query keypoints above octave 0 do not search; train keypoints above octave 0 are not candidates (they would be the best)
    g, cx, cy = S.group(); S.train(g, cx, cy, 10); S.query(g, cx, cy, window, octave=2, role="query octave 2", **q)
    g, cx, cy = S.group(); S.train(g, cx - 3, cy, 5, 1); S.train(g, cx + 3, cy, 25, 0); S.query(g, cx, cy, window, role="train octave 1", **q)
    # vbPrevMatched is not the keypoint: the window is where q_xy says
    g, cx, cy = S.group(); S.train(g, cx, cy, 10); S.query(g, cx, cy, window, key=(f32(300.0), f32(300.0)), role="moved", **q)
    for k in range(48):   # the crowd of bin 0, a third as many in bin 3
        g, cx, cy = S.group()
        S.train(g, cx, cy, 10 + k % 30)
        S.query(g, cx, cy, window, angle=kept2 if k % 4 == 0 else 0.0, **q)
    g, cx, cy = S.group(); S.train(g, cx, cy, 10); S.query(g, cx, cy, window, angle=pruned, role="lone pruned", **q)
    c = S.finish(oracle, nq=nq, radius=window)
    c["window"] = window
    c["q_xy"] = np.ascontiguousarray(c["uvr"][:, :2])
    return c


# ------------------------------------------------------------------ SearchForTriangulation
def _line_pass(y1, y2, o):
    num = f32(f32(y2) - f32(y1))
    return float(f32(f32(num * num) / f32(1.0))) < 3.84 * float(SIGMA2[o])


TRI_X0 = 99.0
# b = x1 - X0, a = 0, c = -y1: with every query keypoint at x1 = X0 + 1 the epipolar line of (x1, y1) is the row y1 and den = 1;
# a query at x1 = X0 has a = b = 0
TRI_F = np.array([[0, 1, 0], [0, 0, -1], [0, -TRI_X0, 0]], np.float32)
TRI_EPIPOLE = (f32(320.0), f32(240.0))


def make_tri_scene(oracle, stereo):
    """Nodes are groups: a query is compared with the train features of its node, whatever their place.  Rows are epipolar lines.
    stereo: uright on one side or the other, and the only_stereo call, on top."""
    rng = np.random.default_rng(4000)
    pruned, kept2 = 270.0, 90.0
    K1, K2, D1, D2, U1, U2 = [], [], [], [], [], []
    node1, node2 = [], []   # per node id: stored member lists
    roles = {}

    def node(qs, ts, one_side=None):
        """qs: (x1, y1, a, angle, uright); ts: (x2, y2, b, octave, uright) in stored order"""
        base = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
        m1, m2 = [], []
        for x, y, a, ang, ur in qs:
            d = base.copy(); d[:a] ^= 1
            m1.append(len(K1)); K1.append((x, y, 0, ang)); D1.append(np.packbits(d)); U1.append(ur)
        for x, y, b, o, ur in ts:
            d = base.copy(); d[128:128 + b] ^= 1
            m2.append(len(K2)); K2.append((x, y, o, 0.0)); D2.append(np.packbits(d)); U2.append(ur)
        node1.append(m1 if one_side != 2 else []); node2.append(m2 if one_side != 1 else [])
        return m1, m2
    X1 = TRI_X0 + 1
    row = iter(range(20, 460, 4))
    # stored order 30, 30, 20, 20, 40: the fourth wins
    y = next(row); m1, m2 = node([(X1, y, 0, 0.0, -1)], [(50 + 10 * k, y, b, 0, -1) for k, b in enumerate((30, 30, 20, 20, 40))]); roles["last of equals"] = (m1[0], m2[3])
    # the nearest fails the epipolar gate, the next passes at 30
    y = next(row); m1, m2 = node([(X1, y, 0, 0.0, -1)], [(50, y + 30, 10, 0, -1), (60, y, 30, 0, -1)]); roles["gate before distance"] = (m1[0], m2[1])
    y = next(row); m1, m2 = node([(X1, y, 0, 0.0, -1)], [(50, y, 50, 0, -1)]); roles["at 50"] = (m1[0], m2[0])
    y = next(row); m1, m2 = node([(X1, y, 0, 0.0, -1)], [(50, y, 51, 0, -1)]); roles["at 51"] = (m1[0], -1)
    for o in (0, 3, 7):   # dsqr one step outside 3.84 * sigma2 would be the best
        y = f32(next(row) + 100)
        p, f = adjacent(lambda y2: _line_pass(y, y2, o), y + f32(0.5), y + 30)
        m1, m2 = node([(X1, y, 0, 0.0, -1)], [(50, f, 5, o, -1), (60, p, 10, o, -1)]); roles["line %d" % o] = (m1[0], m2[1])
    # the epipole inside the image: inside 100 * sf2 (skipped; it would be the best), exactly on it (kept), outside
    ex, ey = TRI_EPIPOLE
    m1, m2 = node([(X1, ey, 0, 0.0, -1)], [(ex + 9, ey, 5, 0, -1), (ex + 10, ey, 10, 0, -1), (ex + 40, ey, 20, 0, -1)]); roles["epipole"] = (m1[0], m2[1])
    m1, m2 = node([(X1, ey, 0, 0.0, -1)], [(ex - 6, ey, 5, 0, -1), (ex + 40, ey, 20, 0, -1)]); roles["epipole near"] = (m1[0], m2[1])
    m1, m2 = node([(X1, ey, 0, 0.0, -1)], [(ex - 12, ey, 5, 3, -1), (ex + 40, ey, 20, 0, -1)]); roles["epipole near, octave 3"] = (m1[0], m2[1])
    # la = lb = 0: every candidate of that query is refused
    y = next(row); m1, m2 = node([(TRI_X0, y, 0, 0.0, -1)], [(50, y, 10, 0, -1), (60, 0.0, 10, 0, -1)]); roles["degenerate line"] = (m1[0], -1)
    # 65 and 130 members: the winner in the second and third trip of the wave, equal distances across the trips (the last wins)
    for n, best in ((65, (3, 64)), (130, (5, 69, 129))):
        y = next(row)
        m1, m2 = node([(X1, y, 0, 0.0, -1), (X1, y, 2, 0.0, -1)], [(20 + 4 * k, y, 15 if k in best else 25 + k % 20, 0, -1) for k in range(n)])
        roles["node of %d" % n] = (m1[0], m2[best[-1]])
    # a query and a train feature that hold a MapPoint already (the feature would be the best)
    y = next(row); m1, m2 = node([(X1, y, 0, 0.0, -1), (X1, y, 1, 0.0, -1)], [(50, y, 5, 0, -1), (60, y, 20, 0, -1)]); roles["skipped"] = (m1[1], m2[1])
    skipped = (m1[0], m2[0])
    y = next(row); node([(X1, y, 0, 0.0, -1)], [(50, y, 10, 0, -1)], one_side=1)
    y = next(row); node([(X1, y, 0, 0.0, -1)], [(50, y, 10, 0, -1)], one_side=2)
    for k in range(48):   # the rotation crowd: bin 0, a third as many in bin 3
        y = next(row); node([(X1, y, 0, kept2 if k % 4 == 0 else 0.0, -1)], [(50 + k, y, 10 + k % 30, 0, -1)])
    y = next(row); m1, m2 = node([(X1, y, 0, pruned, -1)], [(50, y, 10, 0, -1)]); roles["lone pruned"] = (m1[0], m2[0])
    if stereo:
        # a right coordinate on either side switches the epipole test off: the feature next to the epipole is taken
        m1, m2 = node([(X1, ey, 0, 0.0, 70.0)], [(ex + 3, ey, 5, 0, -1), (ex + 40, ey, 20, 0, -1)]); roles["stereo query"] = (m1[0], m2[0])
        m1, m2 = node([(X1, ey, 0, 0.0, -1)], [(ex - 3, ey, 5, 0, 0.0), (ex + 40, ey, 20, 0, -1)]); roles["stereo train"] = (m1[0], m2[0])
        y = next(row); m1, m2 = node([(X1, y, 0, 0.0, 60.0), (X1, y, 1, 0.0, -1)], [(50, y, 5, 0, -1), (60, y, 20, 0, 33.0)]); roles["only stereo"] = (m1[0], m2[1])
    n1, n2 = len(K1), len(K2)
    k1 = np.zeros(n1, dtype=oracle.KP_DTYPE); k2 = np.zeros(n2, dtype=oracle.KP_DTYPE)
    for k, src in ((k1, K1), (k2, K2)):
        a = np.array(src, np.float32).reshape(-1, 4)
        k["x"], k["y"], k["octave"], k["angle"], k["size"] = a[:, 0], a[:, 1], a[:, 2].astype(np.int32), a[:, 3], 31.0

    def csr(nodes):
        ids = [7 * i + 3 for i, m in enumerate(nodes) if m]
        mem = [m for m in nodes if m]
        return (np.array(ids, np.uint32), np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype(np.int32),
                np.concatenate(mem).astype(np.int32))
    skip1, skip2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    skip1[skipped[0]] = skip2[skipped[1]] = 1
    return dict(n1=n1, n2=n2, k1=k1, k2=k2, d1=np.array(D1, np.uint8), d2=np.array(D2, np.uint8), fv1=csr(node1), fv2=csr(node2),
                skip1=skip1, skip2=skip2, F=TRI_F, ex=ex, ey=ey, sf2=SF, sigma2=SIGMA2,
                ur1=np.array(U1, np.float32) if stereo else None, ur2=np.array(U2, np.float32) if stereo else None, roles=roles)


# ------------------------------------------------------------------ the runs: which scene under which parameters, and the oracle's answer
PROJ_RUNS = ([dict(mode=3, th=th, ratio=r, ori=True, stereo=st) for th in (50, 64, 100) for r in (0.75, 0.8, 0.9) for st in (False, True)] +
             [dict(mode=3, th=100, ratio=0.2, ori=True, stereo=False)] +   # (0.2 * 256 < 60: a second at 256 would reject the best)
             [dict(mode=4, th=th, ratio=0.9, ori=o, stereo=st) for th in (50, 64, 100) for o in (False, True) for st in (False, True)] +
             [dict(mode=5, th=th, ratio=0.9, ori=o, stereo=False) for th in (50, 64, 100) for o in (False, True)] +
             [dict(mode=6, th=th, ratio=0.75, ori=True, stereo=False) for th in (50, 64, 100)])
_scenes = {}


def proj_scene(oracle, run):
    key = (run["mode"], run["th"], run["stereo"], run["ori"] and run["mode"] in (4, 5))
    if key not in _scenes:
        _scenes[key] = make_proj_scene(oracle, run["mode"], run["th"], stereo=run["stereo"], rot=key[3])
    return _scenes[key]


def proj_oracle(oracle, c, run, census=False, entry_assign=True):
    st = run["stereo"]
    return oracle.search_by_projection(run["mode"], run["ratio"], run["ori"], run["th"], c["uvr"], c["lvl"], c["qd"], c["qa"], c["qv"], c["qo"], c["gp"],
                                       c["tk"], c["start"], c["idx"], c["td"], c["occ"], c["assign0"] if entry_assign else np.full(c["nt"], -1, np.int32),
                                       q_ur=c["q_ur"] if st else None, t_uright=c["t_ur"] if st else None, census=census)


WINDOW_RUNS = [dict(stereo=st, chi2=x) for st in (False, True) for x in (False, True)]


def window_oracle(oracle, c, run, census=False):
    st = run["stereo"]
    return oracle.window_best(c["uvr"], c["pred"], c["qd"], c["qv"], c["gp"], c["tk"], c["start"], c["idx"], c["td"], INV_SIGMA2, run["chi2"],
                              c["q_ur"] if st else None, c["t_ur"] if st else None, census=census)


INIT_RUNS = [dict(ratio=0.9, ori=True), dict(ratio=0.9, ori=False), dict(ratio=0.8, ori=True), dict(ratio=0.75, ori=True)]


def init_oracle(oracle, c, run, census=False):
    return oracle.search_for_initialization(c["q_xy"], c["window"], c["qk"], c["qd"], c["gp"], c["tk"], c["start"], c["idx"], c["td"], run["ratio"], run["ori"],
                                            census=census)


TRI_RUNS = [dict(stereo=False, only=False, ori=o) for o in (False, True)] + [dict(stereo=True, only=on, ori=o) for on in (False, True) for o in (False, True)]


def tri_oracle(oracle, c, run, census=False):
    return oracle.search_for_triangulation(c["k1"], c["d1"], c["skip1"], c["fv1"], c["k2"], c["d2"], c["skip2"], c["fv2"], c["F"], c["ex"], c["ey"], c["sf2"],
                                           c["sigma2"], run["only"], run["ori"], c["ur1"], c["ur2"], census=census)
