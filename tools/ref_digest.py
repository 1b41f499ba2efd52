#!/usr/bin/env python3
"""SHA-256 of everything the restatements (tools/*_ref.hpp behind tests/cpp/*_ref_capi.cpp) return to the CPU suite.

    python tools/ref_digest.py [ROOT [pytest arguments, such as -k pnp]] > digests.json

Runs ROOT's CPU tests (default: this checkout) in this process with ref_shim.build_ref_shim wrapped: every shim the case
modules build is built by ref_shim as always, and every call through it adds, after it returns, the bytes of each array
argument (inputs and outputs, the drawn RANSAC sets among them) and its scalar return value to the digest of
(restatement, exported function).  That is every family of every *_cases.py at the seeds the CPU tests use, through the
modules' own ref_* helpers.  Addresses are left out: void* returns, the integers that carry them back, and the pointer
fields of a structure passed by reference.  So is what ctypes reads as the return value of a function the shim declares
void.  The result is one JSON object {restatement: {function: [calls, sha256]}}.

It is for comparing two checkouts ON ONE MACHINE (a refactor of the restatements against its parent): the bytes depend
on libm, so the digests are not a fixture."""
import ctypes as C
import hashlib
import json
import os
import re
import sys


class _Fn:
    """one exported function: argtypes / restype pass through, a call is digested after it returns"""

    def __init__(self, fn, rec, returns):
        object.__setattr__(self, "_fn", fn)
        object.__setattr__(self, "_rec", rec)
        object.__setattr__(self, "_returns", returns)

    def __setattr__(self, k, v):
        setattr(self._fn, k, v)

    def __getattr__(self, k):
        return getattr(self._fn, k)

    def __call__(self, *args):
        r = self._fn(*args)
        h = self._rec[1]
        for a in args:
            arr = getattr(a, "_arr", None)            # what ndarray.ctypes.data_as keeps alive: the array itself
            if arr is not None:
                h.update(arr.tobytes())
            elif hasattr(a, "_obj"):                  # ctypes.byref(structure)
                for name, t in getattr(a._obj, "_fields_", ()):
                    if t is not C.c_void_p and not hasattr(t, "contents"):
                        v = getattr(a._obj, name)
                        h.update(bytes(v) if isinstance(v, C.Array) else repr(v).encode())
        if self._returns and self._fn.restype is not C.c_void_p and isinstance(r, (int, float)):
            h.update(repr(r).encode())
        self._rec[0] += 1
        return r


class _Lib:
    def __init__(self, lib, recs, source):
        self._lib, self._recs, self._fns = lib, recs, {}
        self._void = set(re.findall(r"^void (\w+)\(", open(source).read(), flags=re.M))   # (a void* function reads `void* name(`)

    def __getattr__(self, k):
        if k not in self._fns:
            self._fns[k] = _Fn(getattr(self._lib, k), self._recs.setdefault(k, [0, hashlib.sha256()]), k not in self._void)
        return self._fns[k]


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import pytest
    import ref_shim
    assert os.path.dirname(os.path.abspath(ref_shim.__file__)) == os.path.join(root, "tests"), ref_shim.__file__
    digests = {}
    build = ref_shim.build_ref_shim
    ref_shim.build_ref_shim = lambda name: _Lib(build(name), digests.setdefault(name, {}), os.path.join(root, "tests", "cpp", name + "_capi.cpp"))
    stdout = sys.stdout
    sys.stdout = sys.stderr                           # pytest's report goes to stderr, the JSON alone to stdout
    rc = pytest.main([os.path.join(root, "tests"), "-m", "not gpu", "-q", "-x", "-p", "no:cacheprovider", "--rootdir", root] + sys.argv[2:])
    sys.stdout = stdout
    json.dump({lib: {fn: [n, h.hexdigest()] for fn, (n, h) in sorted(fns.items()) if n} for lib, fns in sorted(digests.items())},
              sys.stdout, indent=1, sort_keys=True)
    print()
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
