"""The call table of tests/test_gpu_one_handle.py and tests/test_one_handle_cpu.py (DESIGN.md "Scratch blocks have names"): every
entry that packs its call into a matcher handle's S_BLOCK and stages through its h_stage, the three solvers that attach to a handle
and run on its stream, and five older entries as foreign neighbours -- each at a small size (the smallest case of the family's
*_cases.py that still runs its solver or search), where the family has one at an early return, and at the family's largest existing
case.

A Call has: name (the entry and its form), size ("early", "small", "large"), family (the host file whose core it runs: calls of one
family share offsets, calls of two do not), covers (the host files and the exports of include/orbslamm_hip.h it runs -- what
test_one_handle_cpu.py holds the table to), build(rig) -> world (frame sets, pool, store and resident frames made on THAT rig's
matcher: the orbq_* entries refuse a frame set of another handle), call(rig, world) -> chunks (an ordered dict label -> bytes of every
output array and record) and, where the entry has a restatement, ref(oracle) -> chunks of the same labels from the restatement alone.
verdict(ref chunks' source) names, for the tracking entries, which exit the case takes (test_one_handle_cpu.py: the table must reach
each of them)."""
import collections
import ctypes as C
import functools

import numpy as np

import computesim3_cases as cc
import init_cases as inc
import initmap_cases as imc
import localmap_cases as lc
import motionmodel_cases as mc
import pnp_cases as pnc
import poseopt_cases as pc
import reloc_cases as rc
import sim3_cases as s3c
import sim3opt_cases as soc
import trackpose_cases as tc
import trackref_cases as trc

RANK = {"early": 0, "small": 1, "large": 2}
Call = collections.namedtuple("Call", "name size family covers build call ref verdict")
CAP = rc.CAP


def chunks(*pairs):
    return collections.OrderedDict((k, np.ascontiguousarray(v).tobytes()) for k, v in pairs)


def flat(out, label="out"):
    """any nest of tuples, lists, dicts, arrays, numbers and None as (label, array) pairs"""
    if isinstance(out, dict):
        return [p for k in out for p in flat(out[k], "%s.%s" % (label, k))]
    if isinstance(out, (tuple, list)):
        return [p for i, o in enumerate(out) for p in flat(o, "%s[%d]" % (label, i))]
    if out is None:
        return [(label, np.zeros(0, np.uint8))]
    return [(label, np.asarray(out))]


def joined(ch):
    """the chunks as one byte string, as test_gpu_matcher.py's _as_bytes joins them"""
    return b"|".join(ch.values())


def first_difference(got, want):
    """the label of the first chunk that differs, and where"""
    for k in want:
        if k not in got:
            return k, "missing"
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            if a.shape != b.shape:
                return k, "%d bytes for %d" % (a.size, b.size)
            return k, "byte %d of %d" % (int(np.flatnonzero(a != b)[0]), a.size)
    return None


# ------------------------------------------------------------------ the rig
class Rig(rc.Rig):
    """reloc_cases' rig (a matcher, device memory for frames made of given keys) with what the other families' helpers read from
    theirs: the scale factors and level breaks, and the 6-node vocabulary on first use.  worlds: what the calls built on it"""

    def __init__(self, oracle=None, gex=None):
        """gex: an extractor to take device memory from (the rigs made for one call each share one: it runs nothing)"""
        from orbslamm_amd import ORBextractor, ORBmatcher
        self._own_gex = gex is None
        self.gex = ORBextractor(500, 1.2, 8, 20, 7, max_width=rc.W, max_height=rc.H, max_batch=1, device=0) if gex is None else gex
        self.m = ORBmatcher(0.9, True, device=0)
        self.grid, self.sig = rc.grid(), rc.sigma2()
        self.cfs, self._dev = [], []
        self.oracle = oracle
        self.sf = lc.SF
        self.breaks = rc.breaks()
        self.worlds = {}
        self._G = None

    @property
    def G(self):
        if self._G is None:
            from orbslamm_amd import ORBVocabulary
            v = trc.vocabulary()
            self._G = ORBVocabulary(trc.VOC_K, trc.VOC_L, 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"], device=0)
        return self._G

    def resident(self, keys, desc=None, K=lc.K_A, grid=None):
        """an opaque frame of the given (undistorted) keys on the rig's matcher"""
        desc = np.zeros((len(keys), 32), np.uint8) if desc is None else desc
        dk, dd = self._up(np.ascontiguousarray(keys, tc.KP_DTYPE)), self._up(desc)
        return self.m.frame_from_device(dk, dd, len(keys), K, rc.D0, self.grid if grid is None else grid)

    def world(self, c):
        if key(c) not in self.worlds:
            self.worlds[key(c)] = c.build(self)
        return self.worlds[key(c)]

    def run(self, c):
        return c.call(self, self.world(c))

    def close(self):
        for w in self.worlds.values():
            for k in ("store", "pool", "fs"):
                if isinstance(w, dict) and w.get(k) is not None:
                    w[k].close()
            for f in (w.get("frames", ()) if isinstance(w, dict) else ()):
                self.m.frame_destroy(f)
        self.worlds = {}
        for fs in self.cfs:
            fs.close()
        if self._G is not None:
            self._G.close()
        self.m.close()
        from orbslamm_amd._lib import check
        for d in self._dev:
            check(self.gex._L.orbx_device_free(self.gex._h, d))
        self._dev = []
        if self._own_gex:
            self.gex.close()


def alloc_stats(m):
    """orbm_alloc_stats of a matcher: (device allocations, pinned allocations)"""
    from orbslamm_amd._lib import lib
    dev, host = C.c_int64(0), C.c_int64(0)
    assert lib().orbm_alloc_stats(m._h, C.byref(dev), C.byref(host), None) == 0
    return dev.value, host.value


def _set_for(rig, n):
    return rig.new_set(CAP if n <= CAP else 2048)


# ------------------------------------------------------------------ orbo: PoseOptimization, host arrays and resident frames
PO_SIG = pc.inv_level_sigma2()


@functools.lru_cache(maxsize=None)
def _po_case(n):
    return pc.make_case("gross_30", n, 3)


def _po_call(resident):
    def call(rig, w):
        from orbslamm_amd import optimizer as opt
        c = w["case"]
        frames = np.zeros(1, dtype=opt.FRAME_DTYPE)
        frames["Tcw"][0], frames["K"][0] = c["Tcw"].reshape(16), c["K"]
        edges = opt.pack_edges(c["feature"], c["Xw"])
        code, out, flags = opt.pose_optimize_raw(rig.m._h, frames, None if resident else [c["keys_un"]], w["frames"] if resident else None, [0, c["n"]], edges,
                                                 PO_SIG)
        # (the record whole too: its padding word is the entry's to clear)
        return chunks(("rc", np.int32(code)), *[(k, out[k]) for k in pc.REF_RESULT.names], ("outlier", flags), ("record", out))
    return call


def _po_build(resident, n):
    def build(rig):
        c = _po_case(n)
        return dict(case=c, frames=[rig.resident(c["keys_un"], K=c["K"])] if resident and len(c["keys_un"]) else [])
    return build


def _po_ref(n):
    def ref(oracle):
        out, flags, _, _ = pc.ref_run(pc.DEFINED, [_po_case(n)])
        return chunks(("rc", np.int32(0)), *[(k, out[k]) for k in pc.REF_RESULT.names], ("outlier", flags[0]))
    return ref


# ------------------------------------------------------------------ orbz: OptimizeSim3
SO_SIG = soc.inv_level_sigma2()
SO_FIELDS = ("q", "t", "s", "written", "n_corr", "n_bad", "n_in", "iterations", "trials", "lambda_", "chi2")


@functools.lru_cache(maxsize=None)
def _so_case(n):
    return soc.make_case("gross_30", n, 2, 0)


def _so_call(rig, w):
    from orbslamm_amd import optimizer as opt
    c = w["case"]
    it = {k: c[k] for k in ("R1w", "t1w", "K1", "R2w", "t2w", "K2", "idx1", "obs1", "oct1", "obs2", "oct2", "X1w", "X2w", "th2", "fix_scale")}
    it["S12"] = (c["q"], c["t"], c["s"])
    code, out, flags = opt.optimize_sim3_raw(rig.m._h, opt.pack_sim3_problem(it), [0, c["n"]], opt.pack_sim3_corrs(c), SO_SIG, SO_SIG)
    return chunks(("rc", np.int32(code)), *[(k, out[k]) for k in SO_FIELDS], ("removed", flags), ("record", out))


def _so_ref(n):
    def ref(oracle):
        out, flags, _, _ = soc.ref_run(soc.DEFINED, [_so_case(n)])
        return chunks(("rc", np.int32(0)), *[(k, out[k]) for k in SO_FIELDS], ("removed", flags[0]))
    return ref


# ------------------------------------------------------------------ orbb: the initial map, host arrays and resident frames
@functools.lru_cache(maxsize=None)
def _im_case(family, n):
    return imc.make_case(family, n, 2)


def _im_fields():
    import importlib
    im = importlib.import_module("orbslamm_amd.initial_map")
    return im, [n for n in im.RESULT_DTYPE.names if n != "_pad"]


def _im_call(resident):
    def call(rig, w):
        im, fields = _im_fields()
        c = w["case"]
        problems = np.zeros(1, dtype=im.PROBLEM_DTYPE)
        problems[0] = im.pack_problem(c)
        F = w["frames"]
        code, out, points = im.initial_map_raw(rig.m._h, problems, None if resident else [c["keys_un1"]], None if resident else [c["keys_un2"]],
                                               [F[0]] if resident else None, [F[1]] if resident else None, [c["matches12"]], [c["P3D"]],
                                               imc.inv_level_sigma2(c["family"]), imc.scale_factors())
        return chunks(("rc", np.int32(code)), *[(k, out[k]) for k in fields], ("points", points[0]), ("record", out))
    return call


def _im_build(resident, family, n):
    def build(rig):
        c = _im_case(family, n)
        return dict(case=c, frames=[rig.resident(c["keys_un1"], K=c["K"]), rig.resident(c["keys_un2"], K=c["K"])] if resident else [])
    return build


def _im_ref(family, n):
    def ref(oracle):
        _, fields = _im_fields()
        res, pts, _ = imc.ref_run(_im_case(family, n), imc.DEFINED)
        return chunks(("rc", np.int32(0)), *[(k, res[k]) for k in fields], ("points", pts))
    return ref


# ------------------------------------------------------------------ orby: ComputeSim3
@functools.lru_cache(maxsize=None)
def _cs_case(family, n):
    return cc.make_case(family, 3, n=n)


def _cs_build(family, n):
    def build(rig):
        c = _cs_case(family, n)
        fs = _set_for(rig, n)
        cc.Rig.put_pair(rig, fs, 0, 1, c)
        pool, store = cc.new_world(rig, c["pool"], [c["entries1"], c["entries2"]], c["stride"])
        return dict(case=c, fs=fs, pool=pool, store=store)
    return build


def _cs_call(rig, w):
    from orbslamm_amd.compute_sim3 import compute_sim3_raw, pack_jobs
    rec, keep = pack_jobs([cc.job(w["fs"], 0, 1, 0, 1, w["case"])])
    sig, br = cc.sigma2(), cc.breaks()
    code, out, match, ids, removed, status, vn = compute_sim3_raw(rig.m._h, w["pool"]._h, w["store"]._h, rec, lc.SF, lc.SF, br, br, sig, sig, debug=True)
    return chunks(("rc", np.int32(code)), ("vn", vn[0]), ("status", status[0]), ("OrbyResult", out[0]), ("match", match[0]), ("ids", ids[0]), ("removed", removed[0]))


def _cs_ref(family, n):
    def ref(oracle):
        r = cc.ref_run(_cs_case(family, n))
        return chunks(("rc", np.int32(0)), ("vn", r["vn"]), ("status", r["status"]), ("OrbyResult", r["res"][0]), ("match", r["match"]), ("ids", r["ids"]),
                      ("removed", r["removed"]))
    return ref


# ------------------------------------------------------------------ orbw_project_sync: the two pool searches, then results() / track_status
@functools.lru_cache(maxsize=None)
def _lp_case(size):
    """search local points: a frame, a pool and a shuffled list of its points' ids"""
    if size == "large":
        s = tc.make_scene(79, 2000)
        feat = s["rng"].permutation(2000)
        return tc.with_lists(s, "big", query_feat=feat[:1000])
    s = tc.make_scene(81, 120)
    feat = s["rng"].permutation(120)
    return tc.with_lists(s, "few", query_feat=feat[:0 if size == "early" else 2])


def _lp_build(size):
    def build(rig):
        c = _lp_case(size)
        fs = _set_for(rig, c["n"])
        rig.put(fs, 0, c["keys"], c["desc"])
        return dict(case=c, fs=fs, pool=tc.new_pool(rig, c["pool"]))
    return build


def _lp_call(rig, w):
    c, fs, pool = w["case"], w["fs"], w["pool"]
    pool.track_local_map(fs, 0, c["view"], c["ids"], 1.0, lc.SF, rig.breaks)
    assign, nm = fs.results()
    return chunks(("assign", assign[0, :c["n"]]), ("n_matches", nm[0]), ("status", pool.track_status(fs)))


def _lp_ref(size):
    def ref(oracle):
        """at the small sizes the lattice leaves the search no choice: feature t takes the query that is its own point; the status
        bytes are the restatement's at every size"""
        c = _lp_case(size)
        st = ("status", lc.ref_local(c["view"], c["pool"], c["ids"], 1.0)["status"])
        if size == "large":
            return chunks(st)
        a = np.full(c["n"], -1, np.int32) if c["assign"] is None else c["assign"]
        return chunks(("assign", a.astype(np.int32)), ("n_matches", np.int32((a >= 0).sum())), st)
    return ref


def _vp_ids(size):
    """the list view_project is asked about: the search's, five times over at the large size (unordered and repeated ids; 5 000 ids
    bring 95 000 bytes down: more than the 64 KB a handle's staging block starts with)"""
    ids = _lp_case(size)["ids"]
    return np.tile(ids, 5) if size == "large" else ids


def _vp_call(size):
    def call(rig, w):
        uvr, lvl, cos, st = w["pool"].view_project(w["case"]["view"], _vp_ids(size), 3.0, lc.SF, rig.breaks)
        return chunks(("status", st), ("uvr", uvr), ("lvl", lvl), ("viewcos", cos))
    return call


def _vp_ref(size):
    def ref(oracle):
        c = _lp_case(size)
        r = lc.ref_local(c["view"], c["pool"], _vp_ids(size), 3.0)
        return chunks(("status", r["status"]), ("uvr", r["uvr"]), ("lvl", r["lvl"]), ("viewcos", r["viewcos"]))
    return ref


@functools.lru_cache(maxsize=None)
def _mm_case(size):
    if size == "large":
        return mc.big_case()
    if size == "wide":
        return mc.family_case("wide_rescues")
    if size == "early":
        return mc.family_case("too_few")
    return mc.make_case("first_enough", 2, n=40, nq=30, counts=(21, 0, 0, None))


def _mm_set(rig, c):
    from orbslamm_amd import make_grid
    if c["n"] <= CAP:
        return rig.new_set()
    return rig.m.frame_set(2, mc.BIG_N, mc.BIG_K, rc.D0, make_grid(0.0, 0.0, float(mc.BIG_W), float(mc.BIG_H)), list(c["bounds"]), lc.SF)


def _fp_build(size):
    def build(rig):
        c = _mm_case(size)
        fs = _mm_set(rig, c)
        mc.Rig.put_case(rig, fs, 0, 1, c)
        Tpred = mc.model_pose_product(c["velocity"], c["last_Tcw"])
        return dict(case=c, fs=fs, pool=mc.new_pool(rig, c["pool"]), view=mc.view_of_pose(np.asarray(Tpred, np.float32).reshape(4, 4), c["K"], c.get("bounds", lc.BOUNDS)))
    return build


def _fp_call(rig, w):
    """SearchByProjection(CurrentFrame, LastFrame) from the pool, as TrackWithMotionModel issued it before orbq_track_motion_model"""
    c, fs, pool = w["case"], w["fs"], w["pool"]
    occ = (np.arange(fs.cap) >= c["n"]).astype(np.uint8)
    pool.track_frame_pose(fs, 1, 0, w["view"], c["last_ids"], np.float32(mc.TH), lc.SF, occ, th_dist=100, nnratio=0.9, check_ori=True, mode=4)
    assign, nm = fs.results()
    return chunks(("assign", assign[0, :c["n"]]), ("n_matches", nm[0]), ("status", pool.track_status(fs)))


def _fp_ref(size):
    def ref(oracle):
        """the motion-model restatement's first search: its table where the call did not go on to the wide one, and its count and
        status bytes always"""
        r = mc.ref_run(_mm_case(size))
        out = [("n_matches", np.int32(r[1]["n_search"][0][0])), ("status", r[5][0])]
        if not r[1]["wide"][0]:
            out.insert(0, ("assign", r[4]))
        return chunks(*out)
    return ref


def _vf_call(rig, w):
    """the frame/frame gate set of the projection kernel alone: the octaves come from the resident LastFrame (slot 0)"""
    uvr, lvl, _, st = w["pool"].view_project(w["view"], w["case"]["last_ids"], mc.TH, lc.SF, None, last=(w["fs"], 0))
    return chunks(("status", st), ("uvr", uvr), ("lvl", lvl))


def _vf_ref(size):
    def ref(oracle):
        c = _mm_case(size)
        view = mc.view_of_pose(np.asarray(mc.model_pose_product(c["velocity"], c["last_Tcw"]), np.float32).reshape(4, 4), c["K"], c.get("bounds", lc.BOUNDS))
        r = lc.ref_frame(view, c["pool"], c["last_ids"], c["lkeys"]["octave"][:len(c["last_ids"])], mc.TH)
        return chunks(("status", r["status"]), ("uvr", r["uvr"]), ("lvl", r["lvl"]))
    return ref


# ------------------------------------------------------------------ orbq: the four tracking entries
@functools.lru_cache(maxsize=None)
def _tp_case(size):
    if size == "large":
        s = tc.make_scene(79, 2000)
        feat = s["rng"].permutation(2000)
        c = tc.with_lists(s, "big", base_feat=feat[:500], query_feat=feat[300:1300])
        c["base_ids"][feat[:120]] = c["own"][feat[1500:1620]]          # gross outliers: another feature's point
        return c
    return tc.family_cases("edges_10" if size == "small" else "edges_2")[0]


def _tp_build(size):
    def build(rig):
        c = _tp_case(size)
        fs = _set_for(rig, c["n"])
        rig.put(fs, 0, c["keys"], c["desc"])
        pool = tc.new_pool(rig, c["pool"])
        pool.track_local_map(fs, 0, c["view"], c["ids"], 1.0, lc.SF, rig.breaks)
        assign = fs.results()[0][0, :c["n"]].copy()
        assert c["assign"] is None or np.array_equal(assign, c["assign"])
        return dict(case=c, fs=fs, pool=pool)
    return build


def _tp_call(rig, w):
    code, out, ids, flags = tc.call(rig, w["pool"], [tc.job(w["fs"], 0, w["case"], 0, 1)], sig=tc.sigma2())
    return chunks(("rc", np.int32(code)), ("OrbqResult", out[0]), ("ids", ids[0]), ("outlier", flags[0]))


def _tp_ref(size):
    def ref(oracle):
        code, out, ids, outl, br = tc.ref_run(_tp_case(size), 1)
        return chunks(("rc", np.int32(code)), ("OrbqResult", out[0]), ("ids", ids), ("outlier", outl))
    return ref


def _tp_verdict(size):
    r = tc.ref_run(_tp_case(size), 1)[1][0]
    return "early return" if r["opt"]["rounds"] == 0 else "TRACKED"


@functools.lru_cache(maxsize=None)
def _tr_case(size):
    if size == "large":
        return trc.make_case("mixed", 3, n=2000)
    if size == "early":
        return trc.family_case("empty_kf")
    return trc.make_case("all_valid", 6, n=40)


TR_MIN = {"small": 15, "few": 60, "early": 15, "large": 15}


def _tr_build(size):
    def build(rig):
        c = _tr_case("small" if size == "few" else size)
        fs = _set_for(rig, c["n"])
        trc.Rig.put_pair(rig, fs, 0, 1, c)
        pool, store = trc.new_world(rig, c["pool"], [c["entries"]], c["stride"])
        return dict(case=c, fs=fs, pool=pool, store=store)
    return build


def _tr_call(size):
    def call(rig, w):
        code, out, ids, flags, match = trc.call(rig, w["pool"], w["store"], [trc.job(w["fs"], 0, 1, 0, w["case"])], min_matches=TR_MIN[size], sig=tc.sigma2())
        return chunks(("rc", np.int32(code)), ("match", match[0]), ("OrbqRefResult", out[0]), ("ids", ids[0]), ("outlier", flags[0]))
    return call


def _tr_whole(oracle, size):
    c = _tr_case("small" if size == "few" else size)
    return c, trc.ref_whole(oracle, c, 1, TR_MIN[size], voc=trc.oracle_voc(oracle))


def _tr_ref(size):
    def ref(oracle):
        c, (wm, nb, (code, out, ids, outl, br), valid) = _tr_whole(oracle, size)
        return chunks(("rc", np.int32(code)), ("match", np.asarray(wm[:c["n"]], np.int32)), ("OrbqRefResult", out[0]), ("ids", ids), ("outlier", outl))
    return ref


def _tr_verdict(oracle, size):
    c, whole = _tr_whole(oracle, size)
    if size == "early":
        assert whole[1] == 0
        return "early return"
    return {trc.TRACKED: "TRACKED", trc.TOO_FEW: "TOO_FEW"}[int(whole[2][1]["status"][0])]


@functools.lru_cache(maxsize=None)
def _rl_case(size):
    if size == "large":
        # at the set's cap, with 180 row entries for the wide search to list: more than the 64 entries a job that the arena test leaves it
        return rc.make_case("third_succeeds", 5, n=CAP, nk=280, counts=(40, 20, 150, 30, 6.0, 0.0))
    if size == "early":
        return rc.family_case("rejected")
    if size == "few":
        return rc.family_case("wide_short")
    return rc.make_case("first", 2, n=64, nk=54, counts=(50, 0, 0, 0, 0.0, 0.0))


def _rl_build(size):
    def build(rig):
        c = _rl_case(size)
        fs = _set_for(rig, c["n"])
        rig.put_case(fs, 0, 1, c)
        pool, store = rc.new_world(rig, c["pool"], [c["entries"]], c["stride"])
        return dict(case=c, fs=fs, pool=pool, store=store)
    return build


def _rl_call(rig, w):
    c = w["case"]
    code, out, ids, flags, status = rc.call(rig, w["pool"], w["store"], [rc.job(w["fs"], 0, 1, 0, c)], log_sf=c["log_sf"])
    return chunks(("rc", np.int32(code)), ("status", status[0]), ("ids", ids[0]), ("outlier", flags[0]), ("OrbqRelocResult", out[0]))


def _rl_ref(size):
    def ref(oracle):
        code, out, ids, outl, status, br = rc.ref_run(_rl_case(size))
        return chunks(("rc", np.int32(code)), ("status", status), ("ids", ids), ("outlier", outl), ("OrbqRelocResult", out[0]))
    return ref


def _rl_verdict(size):
    e = int(rc.ref_run(_rl_case(size))[1]["exit"][0])
    return {rc.REJECTED: "early return", rc.FIRST: "TRACKED", rc.WIDE_SHORT: "TOO_FEW", rc.NARROW_SHORT: "TOO_FEW", rc.SECOND: "wide search", rc.THIRD: "wide search"}[e]


def _mm_build(size):
    def build(rig):
        c = _mm_case(size)
        fs = _mm_set(rig, c)
        mc.Rig.put_case(rig, fs, 0, 1, c)
        return dict(case=c, fs=fs, pool=mc.new_pool(rig, c["pool"]))
    return build


def _mm_min(size):
    """the large case with min_matches one above its first count, as test_gpu_motionmodel.py runs it: the wide search runs too"""
    return int(mc.ref_run(_mm_case(size))[1]["n_search"][0][0]) + 1 if size == "large" else mc.MIN_MATCHES


def _mm_call(size):
    def call(rig, w):
        code, out, ids, flags, assign, status = mc.call(rig, w["pool"], [mc.job(w["fs"], 0, 1, w["case"])], min_matches=_mm_min(size))
        return chunks(("rc", np.int32(code)), ("status", status[0]), ("assign", assign[0]), ("ids", ids[0]), ("outlier", flags[0]), ("OrbqMotionResult", out[0]))
    return call


def _mm_ref(size):
    def ref(oracle):
        code, out, ids, outl, asg, status, br = mc.ref_run(_mm_case(size), min_matches=_mm_min(size))
        return chunks(("rc", np.int32(code)), ("status", status), ("assign", asg), ("ids", ids), ("outlier", outl), ("OrbqMotionResult", out[0]))
    return ref


def _mm_verdict(size):
    r = mc.ref_run(_mm_case(size), min_matches=_mm_min(size))[1][0]
    if r["status"] == mc.TOO_FEW:
        return "TOO_FEW"
    return "wide search" if r["wide"] else "TRACKED"


# ------------------------------------------------------------------ the three solvers: made on the handle, run once
@functools.lru_cache(maxsize=None)
def _ini_case(size):
    n = {"small": (8, 30, 30), "large": (500, 1000, 950)}[size]
    keys1, keys2, m12, _, _ = inc.make_scene(np.random.default_rng(100 + n[0]), n_match=n[0], n1=n[1], n2=n[2], noise=0.5, outliers=0.3 if n[0] > 8 else 0.0)
    from orbslamm_amd.initializer import make_sets
    return keys1, keys2, m12, make_sets(int((m12 >= 0).sum()), 200)


def _ini_chunks(r):
    return chunks(*flat({k: r["res"][k] for k in sorted(r["res"])}, "res"), ("ok", np.int32(r["ok"])), ("R21", np.asarray(r["R21"], np.float32)),
                  ("t21", np.asarray(r["t21"], np.float32)), ("p3d", np.asarray(r["p3d"], np.float32)), ("triangulated", np.asarray(r["triangulated"], np.uint8)))


def _ini_call(size):
    def call(rig, w):
        from orbslamm_amd.initializer import Initializer
        keys1, keys2, m12, sets = _ini_case(size)
        ini = Initializer(rig.m, keys1, inc.K_TUM, sigma=1.0, iterations=200, model="HF")
        r = ini.initialize(keys2, m12, sets)
        again = ini.initialize(keys2, m12, sets)         # the solver's own blocks: the same object twice
        ini.close()
        assert joined(_ini_chunks(r)) == joined(_ini_chunks(again)), "the same Initializer twice"
        return _ini_chunks(r)
    return call


def _ini_ref(size):
    def ref(oracle):
        keys1, keys2, m12, sets = _ini_case(size)
        return _ini_chunks(inc.ref_initialize(keys1, keys2, m12, sets, K=inc.K_TUM, sigma=1.0, model="HF"))
    return ref


def _ransac_chunks(table, fields, r, ints, bits):
    return chunks(*[("table." + k, table[k]) for k in fields], *[("find." + k, np.int64(r[k])) for k in ints], *[("find." + k, np.asarray(r[k])) for k in bits])


S3_FIELDS = ("n_inliers", "s12", "T12", "R12", "t12")


@functools.lru_cache(maxsize=None)
def _s3_case(size):
    return s3c.family_case("general", 3, n={"small": 10, "large": 2000}[size], outliers=0.2, noise=0.002)


@functools.lru_cache(maxsize=None)
def _s3_sets(size):
    """drawn once: the sets come from libc's rand(), which is the process's, and the two-thread test runs the calls side by side"""
    case = _s3_case(size)
    probe = s3c.RefSolver(case)
    probe.set_ransac(*case["ransac"])
    return s3c.case_sets(case, probe.max_iterations, 0)


def _s3_call(size):
    def call(rig, w):
        from orbslamm_amd.sim3 import run_all
        case = _s3_case(size)
        dev = s3c.device_solver(rig.m, case)
        sets = _s3_sets(size)
        assert len(sets) == dev.max_iterations
        run_all([dev], [sets])
        first = dev.hypotheses().copy()
        run_all([dev], [sets])                           # the solver's own blocks: the same object twice
        assert first.tobytes() == dev.hypotheses().tobytes(), "the same Sim3Solver twice"
        out = _ransac_chunks(first, S3_FIELDS, dev.find(), s3c.RESULT_INTS, s3c.RESULT_BITS)
        dev.close()
        return out
    return call


def _s3_ref(size):
    def ref(oracle):
        s = s3c.ref_solve(_s3_case(size), sets=_s3_sets(size))
        return _ransac_chunks(s.all_hypotheses(), S3_FIELDS, s.find(), s3c.RESULT_INTS, s3c.RESULT_BITS)
    return ref


@functools.lru_cache(maxsize=None)
def _pn_case(size):
    return pnc.family_case("wrong_20", 3, n={"small": 10, "large": 3000}[size])


@functools.lru_cache(maxsize=None)
def _pn_sets(size):
    """drawn once, as _s3_sets"""
    case = _pn_case(size)
    probe = pnc.RefSolver(case)
    probe.set_ransac(*case["ransac"])
    return pnc.case_sets(case, probe.max_iterations + pnc.EXTRA_SETS, 0)


def _pn_call(size):
    def call(rig, w):
        from orbslamm_amd.pnp import run_all
        case = _pn_case(size)
        dev = pnc.device_solver(rig.m, case)
        sets = _pn_sets(size)
        assert len(sets) == dev.max_iterations + pnc.EXTRA_SETS
        run_all([dev], [sets])
        first = dev.hypotheses().copy()
        run_all([dev], [sets])                           # the solver's own blocks: the same object twice
        assert first.tobytes() == dev.hypotheses().tobytes(), "the same PnPsolver twice"
        out = _ransac_chunks(first, pnc.TABLE_FIELDS, dev.find(), pnc.RESULT_INTS, pnc.RESULT_BITS)
        dev.close()
        return out
    return call


def _pn_ref(size):
    def ref(oracle):
        s = pnc.ref_solve(_pn_case(size), sets=_pn_sets(size))
        return _ransac_chunks(s.all_hypotheses(), pnc.TABLE_FIELDS, s.find(), pnc.RESULT_INTS, pnc.RESULT_BITS)
    return ref


# ------------------------------------------------------------------ five older entries as foreign neighbours (test_gpu_matcher.py's table)
@functools.lru_cache(maxsize=None)
def _old_case(n):
    import fuse_cases as fc
    import loopfuse_cases as lfc
    from conftest import random_descriptors
    from matcher_cases import make_bow_case, make_proj_case
    from orbslamm_amd import local_mapping as lm, make_grid
    rng = np.random.default_rng(9000 + n)
    q, t = random_descriptors(rng, n), random_descriptors(rng, n + 5)
    qa, ta = rng.uniform(0, 360, n).astype(np.float32), rng.uniform(0, 360, n + 5).astype(np.float32)
    pcase = make_proj_case(rng, n, n + 7)
    return dict(q=q, t=t, qa=qa, ta=ta, bow=make_bow_case(rng, n, n + 3, max(1, n // 20)), pc=pcase, g=make_grid(0.0, 0.0, pcase["w"], pcase["h"]),
                a0=np.full(n + 7, -1, np.int32), breaks=lm.level_breaks(fc.LOG_SF, fc.NLEVELS),
                fuse=fc.make_case(n, targets=(2, 2), points=(60, 60), feats=n), loop=lfc.make_dense(n + 1, targets=(2, 2), points=(60, 60), feats=n))


def proj_search(m, o):
    c = o["pc"]
    return m.SearchByProjection(4, 100, c["uvr"], c["lvl"], c["qd"], c["qa"], c["qv"], c["qo"], o["g"], c["tk"], c["td"], c["occ"], o["a0"])


def _old_bruteforce(m, o):
    return m.match_bruteforce(o["q"], o["qa"], o["t"], o["ta"])


def _old_prepared(m, o):
    m.ProjectionPrepare(o["g"], o["pc"]["tk"], o["pc"]["td"])
    return proj_search(m, o)


def _old_bow(m, o):
    b = o["bow"]
    return m.SearchByBoW(b["qd"], b["qa"], b["qv"], b["qfv"], b["td"], b["ta"], None, b["tfv"], True)


def _old_fuse(m, o):
    from orbslamm_amd import local_mapping as lm
    f = o["fuse"]
    return lm.fuse_batch(m, f["targets"], f["points"], f["jobs"], f["sf"], f["inv_sigma2"], o["breaks"], th=f["th"])


def _old_loop(m, o):
    from orbslamm_amd import loop_closing as lo
    f = o["loop"]
    return lo.search_and_fuse(m, f["targets"], f["points"], f["sf"], o["breaks"], th=f["th"], capacity=len(f["targets"]) * len(f["points"]), want_status=True)


def _old(fn, n):
    return lambda rig, w: chunks(*flat(fn(rig.m, _old_case(n))))


OLD_N = {"small": 96, "large": 700}


# ------------------------------------------------------------------ the table
def _none(rig):
    return {}


def _table():
    T = []

    def add(name, size, family, covers, build, call, ref=None, verdict=None):
        T.append(Call(name, size, family, tuple(covers), build, call, ref, verdict))
    for size, n in (("early", 2), ("small", 10), ("large", 2000)):
        add("pose_optimize_raw host arrays", size, "orbo_host.inc", ("orbo_host.inc", "orbo_pose_optimize"), _po_build(False, n), _po_call(False), _po_ref(n))
        add("pose_optimize_raw resident frames", size, "orbo_host.inc", ("orbo_host.inc", "orbo_pose_optimize_frames", "orbm_frame_create", "orbm_frame_destroy"),
            _po_build(True, n), _po_call(True), _po_ref(n))
    for size, n in (("early", 9), ("small", 10), ("large", 1000)):
        add("optimize_sim3_raw", size, "orbz_host.inc", ("orbz_host.inc", "orbz_optimize_sim3"), lambda rig, n=n: dict(case=_so_case(n)), _so_call, _so_ref(n))
    for size, fam, n in (("early", "no_points", 64), ("small", "noisy", 2), ("large", "noisy", 600)):
        add("initial_map_raw host arrays", size, "orbb_host.inc", ("orbb_host.inc", "orbb_initial_map"), _im_build(False, fam, n), _im_call(False), _im_ref(fam, n))
        add("initial_map_raw resident frames", size, "orbb_host.inc", ("orbb_host.inc", "orbb_initial_map_frames"), _im_build(True, fam, n), _im_call(True), _im_ref(fam, n))
    for size, fam, n in (("early", "below_ten", 300), ("small", "all_new", 40), ("large", "inliers_in", 2000)):
        add("compute_sim3", size, "orby_host.inc", ("orby_host.inc", "orby_compute_sim3", "orbw_pool_create", "orbw_pool_set", "orbw_pool_destroy", "orbm_frameset_create",
                                                    "orbm_frameset_build", "orbm_frameset_sync", "orbm_frameset_destroy"), _cs_build(fam, n), _cs_call, _cs_ref(fam, n))
    for size in ("early", "small", "large"):
        add("track_pose_raw", size, "orbq_host.inc", ("orbq_host.inc", "orbq_track_pose"), _tp_build(size), _tp_call, _tp_ref(size), lambda o, s=size: _tp_verdict(s))
    for size in ("early", "few", "small", "large"):
        add("track_reference", "small" if size == "few" else size, "orbq_host.inc", ("orbq_host.inc", "orbq_track_reference", "orbm_frameset_compute_bow"),
            _tr_build(size), _tr_call(size), _tr_ref(size), lambda o, s=size: _tr_verdict(o, s))
    for size in ("early", "few", "small", "large"):
        add("relocalize_raw", "small" if size == "few" else size, "orbq_reloc_host.inc", ("orbq_reloc_host.inc", "orbq_relocalize"), _rl_build(size), _rl_call, _rl_ref(size),
            lambda o, s=size: _rl_verdict(s))
    for size in ("early", "wide", "small", "large"):
        add("track_motion_model", "small" if size == "wide" else size, "orbq_motion_host.inc", ("orbq_motion_host.inc", "orbq_track_motion_model"), _mm_build(size),
            _mm_call(size), _mm_ref(size), lambda o, s=size: _mm_verdict(s))
    for size in ("early", "small", "large"):
        add("search local points, results, track_status", size, "orbw_host.inc", ("orbw_host.inc", "orbw_track_local_map", "orbm_track_results", "orbw_track_status"),
            _lp_build(size), _lp_call, _lp_ref(size))
        add("track_frame_pose, results, track_status", size, "orbw_host.inc", ("orbw_host.inc", "orbw_track_frame_pose", "orbm_track_results", "orbw_track_status"),
            _fp_build(size), _fp_call, _fp_ref(size))
        # orbw_project_sync itself: the projection kernel alone packs ids, arrays and flags into S_BLOCK, under both gate sets
        add("view_project", size, "orbw_host.inc", ("orbw_host.inc", "orbw_view_project"), _lp_build(size), _vp_call(size), _vp_ref(size))
        add("view_project_frame", size, "orbw_host.inc", ("orbw_host.inc", "orbw_view_project_frame"), _fp_build(size), _vf_call, _vf_ref(size))
    for size in ("small", "large"):
        add("Initializer", size, "orbi_host.inc", ("orbi_create", "orbi_initialize", "orbi_destroy"), _none, _ini_call(size), _ini_ref(size))
        add("Sim3Solver", size, "orbs_host.inc", ("orbs_create", "orbs_set_ransac", "orbs_max_iterations", "orbs_run", "orbs_hypotheses", "orbs_iterate", "orbs_destroy"),
            _none, _s3_call(size), _s3_ref(size))
        add("PnPsolver", size, "orbp_host.inc", ("orbp_create", "orbp_set_ransac", "orbp_max_iterations", "orbp_run", "orbp_hypotheses", "orbp_iterate", "orbp_destroy"),
            _none, _pn_call(size), _pn_ref(size))
        n = OLD_N[size]
        add("match_bruteforce", size, "orbm_host.inc", ("orbm_match_bruteforce",), _none, _old(_old_bruteforce, n))
        add("search_by_projection prepared", size, "orbt_host.inc", ("orbm_projection_prepare", "orbm_search_by_projection"), _none, _old(_old_prepared, n))
        add("search_by_bow", size, "orbt_host.inc", ("orbm_search_by_bow",), _none, _old(_old_bow, n))
        add("fuse_batch", size, "orbl_host.inc", ("orbl_host.inc", "orbl_fuse_batch"), _none, _old(_old_fuse, n))
        add("search_and_fuse", size, "orbc_host.inc", ("orbc_host.inc", "orbc_search_and_fuse"), _none, _old(_old_loop, n))
    return T


TABLE = _table()
NAMES = tuple(dict.fromkeys(c.name for c in TABLE))
TRACKING = ("track_pose_raw", "track_reference", "relocalize_raw", "track_motion_model")
# what each tracking entry can end as: orbq_track_pose has neither a match gate nor a second search
VERDICTS = {"track_pose_raw": ("TRACKED", "early return"), "track_reference": ("TRACKED", "TOO_FEW", "early return"),
            "relocalize_raw": ("TRACKED", "TOO_FEW", "wide search", "early return"), "track_motion_model": ("TRACKED", "TOO_FEW", "wide search")}


def key(c):
    return c.name, c.size, TABLE.index(c)


def of(name, size=None):
    """the calls of an entry, or those of one size"""
    return [c for c in TABLE if c.name == name and (size is None or c.size == size)]


def size_order(sizes=("large", "small", "large")):
    """every call of the table in the order large, small (the early returns with it), large"""
    return [c for s in sizes for c in TABLE if c.size == s or (s == "small" and c.size == "early")]


def schedule(seed, length=60):
    """about `length` calls drawn with a seeded generator: the entries in a shuffled order, each at a small size (or its early return)
    directly behind a large call of another family, and random calls of any size between those pairs"""
    rng = np.random.default_rng(seed)
    large = [c for c in TABLE if c.size == "large"]
    out = []
    spare = max(length - 2 * len(NAMES), 0)
    for i, k in enumerate(rng.permutation(len(NAMES))):
        mine = [c for c in TABLE if c.name == NAMES[k]]
        small = [c for c in mine if c.size != "large"]
        other = [c for c in large if c.family != mine[0].family]
        out += [other[rng.integers(len(other))], small[rng.integers(len(small))]]
        for _ in range(spare // len(NAMES) + (i < spare % len(NAMES))):
            out.append(TABLE[rng.integers(len(TABLE))])
    return out
