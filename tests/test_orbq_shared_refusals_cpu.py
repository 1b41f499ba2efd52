"""The argument checks that orbq_track_pose, orbq_track_reference, orbq_relocalize and orbq_track_motion_model share (orbq_scaffold.inc,
DESIGN.md §8s): one table of bad arguments, each row refused by every entry with the same code and the same fragment of the message.
No handle, no GPU: each entry is called the way its own *_cpu.py file calls it, and every row is refused before a handle is looked at."""
import importlib

import numpy as np
import pytest

import localmap_cases as lc
import reloc_cases as rc
import trackpose_cases as tc
from orbslamm_amd import _lib

tp = importlib.import_module("orbslamm_amd.track_pose")   # (the package exports a function of the module's name)

MAX_FRAMES, MAX_EDGES, MAX_CALL_EDGES, MAX_LEVELS = 4096, 65535, 1 << 22, 16
E_INVALID, E_UNSUPPORTED = _lib.ORBX_E_INVALID, _lib.ORBX_E_UNSUPPORTED
FS, H_ = 0x1000, 0x10   # never followed: every row is refused before


def _pose(jobs):
    return tp.pack_jobs([dict(fs=fs, slot=0, back=0, base_ids=None, n=0, discard=0, Tcw=np.eye(4), K=lc.K_A) for fs, n in jobs]), tp.TRACK_RESULT_DTYPE


def _ref(jobs):
    return (tp.pack_ref_jobs([dict(fs=fs, kf_slot=0, slot=1, kf=0, n=0) for fs, n in jobs]), []), tp.REF_RESULT_DTYPE


def _reloc(jobs):
    return tp.pack_reloc_jobs([dict(fs=fs, slot=1, kf_slot=0, kf=0, n=0, ids=np.full(1, -1, np.int32)) for fs, n in jobs]), tp.RELOC_RESULT_DTYPE


def _motion(jobs):
    return tp.pack_motion_jobs([dict(fs=fs, cur_slot=1, last_slot=0, n=0, last_ids=np.full(1, -1, np.int32), nq=1) for fs, n in jobs]), tp.MOTION_RESULT_DTYPE


def _call_pose(L, rec, n_jobs, sig, nlevels, out, ids, outl):
    return L.orbq_track_pose(None, None, rec, n_jobs, sig, nlevels, out, ids, outl)


def _call_ref(L, rec, n_jobs, sig, nlevels, out, ids, outl):
    return L.orbq_track_reference(None, None, None, rec, n_jobs, 0.7, 1, 15, sig, nlevels, out, ids, outl, None)


def _call_reloc(L, rec, n_jobs, sig, nlevels, out, ids, outl):
    return L.orbq_relocalize(H_, H_, H_, rec, n_jobs, 1, sig, _lib.ptr(lc.SF), _lib.ptr(BREAKS), nlevels, out, ids, outl, None)


def _call_motion(L, rec, n_jobs, sig, nlevels, out, ids, outl):
    return L.orbq_track_motion_model(H_, H_, rec, n_jobs, 15.0, 20, 1, sig, _lib.ptr(lc.SF), nlevels, out, ids, outl, None, None)


BREAKS = rc.breaks()
ENTRIES = {"track_pose": (_pose, _call_pose), "track_reference": (_ref, _call_ref), "relocalize": (_reloc, _call_reloc),
           "track_motion_model": (_motion, _call_motion)}

# the two words of a shared message that are an entry's own: how it names a level table that is not there, and a job's null array
WORDS = {"track_pose": (b"no sigma table", b"null output array"), "track_reference": (b"no sigma table", b"null output array"),
         "relocalize": (b"no level table", b"null array"), "track_motion_model": (b"no level table", b"null array")}

# (what, code, the fragment every entry's message holds, the call's arguments: jobs as (fs, n) pairs; own: which of WORDS ends the message)
ROWS = [
    ("n_jobs -1", E_INVALID, b"negative job count", dict(n_jobs=-1)),
    ("n_jobs above ORBO_MAX_FRAMES", E_UNSUPPORTED, b"%d jobs: above %d" % (MAX_FRAMES + 1, MAX_FRAMES), dict(n_jobs=MAX_FRAMES + 1)),
    ("a null out", E_INVALID, b"null argument", dict(out=False)),
    ("nlevels 0", E_INVALID, b"nlevels 0 outside [1, %d]" % MAX_LEVELS, dict(nlevels=0)),
    ("nlevels above ORBX_MAX_LEVELS", E_INVALID, b"nlevels %d outside [1, %d]" % (MAX_LEVELS + 1, MAX_LEVELS), dict(nlevels=MAX_LEVELS + 1)),
    ("a null sigma table", E_INVALID, b"outside [1, %d] or no " % MAX_LEVELS, dict(sig=False, own=0)),
    ("job 1 of 2 with a null frame set", E_INVALID, b"job 1: null frame set", dict(jobs=[(FS, 4), (0, 4)])),
    ("n -1", E_INVALID, b"job 0: negative feature count", dict(jobs=[(FS, -1)])),
    ("n above ORBO_MAX_EDGES", E_UNSUPPORTED, b"job 0: %d features: above %d" % (MAX_EDGES + 1, MAX_EDGES), dict(jobs=[(FS, MAX_EDGES + 1)])),
    ("a null per-job ids_out with n 1", E_INVALID, b"job 0: null ", dict(jobs=[(FS, 1)], ids=False, own=1)),
    ("a null per-job outlier_out with n 1", E_INVALID, b"job 0: null ", dict(jobs=[(FS, 1)], outl=False, own=1)),
    # (a job takes at most ORBO_MAX_EDGES features, so the fewest jobs that reach the call's bound: full ones, and the last a feature past it)
    ("jobs whose n sum to ORBO_MAX_CALL_EDGES + 1", E_UNSUPPORTED, b"more than %d features in one call (reached at job %d)" % (MAX_CALL_EDGES, MAX_CALL_EDGES // MAX_EDGES),
     dict(jobs=[(FS, MAX_EDGES)] * (MAX_CALL_EDGES // MAX_EDGES) + [(FS, MAX_CALL_EDGES % MAX_EDGES + 1)])),
]
assert sum(n for _, n in ROWS[-1][3]["jobs"]) == MAX_CALL_EDGES + 1


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("what,code,fragment,kw", ROWS, ids=[r[0] for r in ROWS])
def test_a_shared_bad_argument_is_refused_alike(entry, what, code, fragment, kw):
    L = _lib.lib()
    pack, call = ENTRIES[entry]
    jobs = kw.get("jobs", [(FS, 4), (FS, 4)])
    (rec, keep), result_dtype = pack(jobs)
    rec["n"] = [n for _, n in jobs]
    out = np.zeros(len(jobs), result_dtype)
    ids = [np.full(4, 7, np.int32) for _ in jobs]
    outl = [np.full(4, 7, np.uint8) for _ in jobs]
    sig = tc.sigma2()
    got = call(L, _lib.ptr(rec), kw.get("n_jobs", len(jobs)), _lib.ptr(sig) if kw.get("sig", True) else None, kw.get("nlevels", sig.shape[0]),
               _lib.ptr(out) if kw.get("out", True) else None, _lib.table(ids if kw.get("ids", True) else [None] * len(jobs)),
               _lib.table(outl if kw.get("outl", True) else [None] * len(jobs)))
    msg = L.orbx_last_error()
    assert got == code, (entry, what, got, msg)
    assert fragment in msg, (entry, what, msg)
    if "own" in kw:
        assert msg.endswith(WORDS[entry][kw["own"]]), (entry, what, msg)
    # a refusal writes nothing
    assert out.tobytes() == bytes(out.nbytes) and all((a == 7).all() for a in ids) and all((a == 7).all() for a in outl), (entry, what)
