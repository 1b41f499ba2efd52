"""KeyFrameDatabase (src/KeyFrameDatabase.cc) over a device-resident keyframe pool (include/orbslamm_hip.h: orbk_*).

Keyframes are pool slots.  A slot holds the keyframe's mBowVec in HBM and its six query fields (mnRelocQuery, mnRelocWords,
mRelocScore, mnLoopQuery, mnLoopWords, mLoopScore), which persist across queries and across every database over the pool.
Results equal the reference bit for bit."""
import ctypes as C

import numpy as np

from ._lib import check, lib, ptr

NEIGHBOURS = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32))
MAX_NEIGHBOURS = 10


def _bow(ids, vals):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    if ids.shape != vals.shape or ids.ndim != 1:
        raise ValueError("BowVector: word ids and values of one length")
    return ids, vals


class KeyFramePool:
    def __init__(self, voc, slots=0):
        self._L = lib()
        self._h = C.c_void_p()
        self.voc = voc   # (kept alive: the pool reads its tree size and device)
        check(self._L.orbk_pool_create(voc._h, int(slots), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbk_pool_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = C.c_int()
        check(self._L.orbk_pool_size(self._h, C.byref(n)))
        return n.value

    def set_bow(self, slot, ids, vals):
        """the keyframe's mBowVec (word ids ascending)"""
        ids, vals = _bow(ids, vals)
        check(self._L.orbk_pool_set_bow(self._h, int(slot), ptr(ids), ptr(vals), ids.shape[0]))

    def set_bow_from_frameset(self, slot, frameset, fs_slot):
        """mBowVec of a frame set slot (orbm_frameset_compute_bow), copied device to device"""
        check(self._L.orbk_pool_set_bow_from_frameset(self._h, int(slot), frameset._h, int(fs_slot)))

    def score(self, slot, others):
        """[(float)ORBVocabulary::score(slot's mBowVec, o's mBowVec) for o in others]"""
        o = np.ascontiguousarray(others, dtype=np.int32)
        out = np.zeros(max(o.shape[0], 1), np.float32)
        check(self._L.orbk_pool_score(self._h, int(slot), ptr(o), o.shape[0], ptr(out)))
        return out[:o.shape[0]]

    def set_covisibility(self, slot, best):
        """GetBestCovisibilityKeyFrames(10) of the slot (detect_loop_batch, and queries given no neighbour callable)"""
        b = np.ascontiguousarray(best, dtype=np.int32)
        check(self._L.orbk_pool_set_covisibility(self._h, int(slot), ptr(b), b.shape[0]))

    def state(self):
        """the six fields of every slot: dict of arrays"""
        n = len(self)
        rq, lq = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        rw, lw = np.zeros(n, np.int32), np.zeros(n, np.int32)
        rs, ls = np.zeros(n, np.float32), np.zeros(n, np.float32)
        check(self._L.orbk_pool_read_state(self._h, ptr(rq), ptr(rw), ptr(rs), ptr(lq), ptr(lw), ptr(ls), n))
        return dict(mnRelocQuery=rq, mnRelocWords=rw, mRelocScore=rs, mnLoopQuery=lq, mnLoopWords=lw, mLoopScore=ls)


class KeyFrameDatabase:
    """the reference's member names; keyframes are slots of `pool`"""

    def __init__(self, pool):
        self._L = lib()
        self.pool = pool
        self._h = C.c_void_p()
        check(self._L.orbk_db_create(pool._h, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbk_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, slot):
        check(self._L.orbk_db_add(self._h, int(slot)))

    def erase(self, slot):
        check(self._L.orbk_db_erase(self._h, int(slot)))

    def clear(self):
        check(self._L.orbk_db_clear(self._h))

    def size(self):
        n = C.c_int()
        check(self._L.orbk_db_size(self._h, C.byref(n)))
        return n.value

    def empty(self):
        e = C.c_int()
        check(self._L.orbk_db_empty(self._h, C.byref(e)))
        return bool(e.value)

    def last_scored(self):
        """lScoreAndMatch of the last single query: (slots, float32 scores) in list order"""
        n = C.c_int()
        cap = max(len(self.pool), 1)
        sl, sc = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        check(self._L.orbk_db_last_scored(self._h, ptr(sl), ptr(sc), cap, C.byref(n)))
        return sl[:n.value].copy(), sc[:n.value].copy()

    @staticmethod
    def _callback(neighbours):
        """neighbours: callable slot -> up to 10 slots (GetBestCovisibilityKeyFrames(10) at the time of the call), or None"""
        if neighbours is None:
            return NEIGHBOURS(), []
        err = []

        def cb(_user, slot, out):
            try:
                nb = [int(x) for x in neighbours(int(slot))]
                if len(nb) > MAX_NEIGHBOURS:
                    raise ValueError("more than %d neighbours" % MAX_NEIGHBOURS)
                for i, x in enumerate(nb):
                    out[i] = x
                return len(nb)
            except Exception as e:  # noqa: BLE001 -- reported after the call
                err.append(e)
                return -1
        return NEIGHBOURS(cb), err

    def _run(self, fn, *args, neighbours=None):
        cap = max(len(self.pool), 1)
        out = np.zeros(cap, np.int32)
        n = C.c_int()
        cb, err = self._callback(neighbours)
        rc = fn(self._h, *args, cb, None, ptr(out), cap, C.byref(n))
        if err:
            raise err[0]
        check(rc)
        return out[:n.value].tolist()

    def DetectRelocalizationCandidates(self, query_id, bow=None, frameset=None, fs_slot=0, neighbours=None):
        """vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F): F->mnId = query_id, F->mBowVec = bow (ids, values)
        or frame set slot fs_slot; returns candidate slots in the reference's order"""
        if frameset is not None:
            return self._run(self._L.orbk_detect_relocalization_candidates_frameset, C.c_uint64(int(query_id)), frameset._h, int(fs_slot),
                             neighbours=neighbours)
        ids, vals = _bow(*bow)
        return self._run(self._L.orbk_detect_relocalization_candidates, C.c_uint64(int(query_id)), ptr(ids), ptr(vals), ids.shape[0],
                         neighbours=neighbours)

    def DetectLoopCandidates(self, slot, query_id, minScore, connected=(), neighbours=None):
        """vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore): pKF = slot, pKF->mnId = query_id,
        connected = pKF->GetConnectedKeyFrames()"""
        conn = np.ascontiguousarray(sorted(set(int(c) for c in connected)), dtype=np.int32)
        return self._run(self._L.orbk_detect_loop_candidates, int(slot), C.c_uint64(int(query_id)), ptr(conn), conn.shape[0],
                         C.c_float(float(np.float32(minScore))), neighbours=neighbours)

    def detect_loop_batch(self, slots, query_ids, connected, covisible):
        """MultiMapper::DetectLoop's scan: for each keyframe q, minScore over covisible[q] (GetVectorCovisibleKeyFrames()
        without the bad ones), then DetectLoopCandidates(q, minScore) with connected[q]; the same as the queries one after
        another.  Neighbours come from the pool's covisibility table.  Returns one candidate list per query."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ids = np.ascontiguousarray(query_ids, dtype=np.uint64)
        n = sl.shape[0]
        if ids.shape[0] != n or len(connected) != n or len(covisible) != n:
            raise ValueError("one id, connected set and covisible list per query")

        def csr(lists):
            start = np.zeros(n + 1, np.int32)
            start[1:] = np.cumsum([len(x) for x in lists])
            idx = np.ascontiguousarray(np.concatenate([np.asarray(list(x), np.int32) for x in lists]) if n else np.zeros(0), dtype=np.int32)
            return start, idx
        cs, ci = csr([sorted(set(int(c) for c in x)) for x in connected])
        vs, vi = csr([list(x) for x in covisible])
        out_start = np.zeros(n + 1, np.int32)
        cap = max(n * len(self.pool), 1)   # (a query returns each slot at most once)
        out = np.zeros(cap, np.int32)
        check(self._L.orbk_detect_loop_batch(self._h, n, ptr(sl), ptr(ids), ptr(cs), ptr(ci), ptr(vs), ptr(vi), ptr(out_start), ptr(out), cap))
        return [out[out_start[q]:out_start[q + 1]].tolist() for q in range(n)]
