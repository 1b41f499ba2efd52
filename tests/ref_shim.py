"""What the case modules (tests/*_cases.py) share.  A restatement's C shim (tests/cpp/*_ref_capi.cpp over tools/*_ref.hpp) is
built with g++ -ffp-contract=off into a temporary directory and loaded, once per process; which files a restatement is made
of; bit equality; the rotation the scene generators use."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_shims = {}


def build_ref_shim(name):
    """tests/cpp/<name>_capi.cpp as a loaded shared object"""
    out = os.path.join(tempfile.mkdtemp(prefix=name + "_"), "lib%s.so" % name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", name + "_capi.cpp"), "-o", out])
    return C.CDLL(out)


def cached_shim(name, declare=None):
    """build_ref_shim(name) once per process; declare(lib) sets the argtypes and checks the record sizes on the first call"""
    if name not in _shims:
        lib = build_ref_shim(name)
        if declare is not None:
            declare(lib)
        _shims[name] = lib
    return _shims[name]


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def declared(header, prefix=""):
    """the C entries include/<header> declares whose names begin with `prefix`, sorted -- as the loader itself reads the headers
    (_lib.declarations()), so a family's test and the library's signatures cannot come from two readings"""
    from orbslamm_amd import _lib
    return sorted(n for n, d in _lib.declarations().items() if d.header == header and n.startswith(prefix))


def quoted_includes(path):
    """every file reached from `path` through #include "..." (resolved beside the including file, as g++ does first),
    transitively, `path` itself first: absolute paths.  A quoted include that does not exist there is an error: the
    restatements are built with no -I."""
    reached, todo = [], [os.path.abspath(path)]
    while todo:
        f = todo.pop(0)
        if f in reached:
            continue
        reached.append(f)
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(f).read(), flags=re.M):
            target = os.path.normpath(os.path.join(os.path.dirname(f), inc))
            assert os.path.exists(target), "%s includes %s, which is not beside it" % (f, inc)
            todo.append(target)
    return reached


def assert_shares_no_code_with_the_library(path):
    """a restatement shares no code with the library it checks: every file it reaches lies in tools/, and none of them
    names a header or a source of the library"""
    tools = os.path.join(ROOT, "tools") + os.sep
    for f in quoted_includes(path):
        assert f.startswith(tools), "%s reaches %s, outside tools/" % (path, f)
        code = open(f).read().split("#pragma once", 1)[1]   # (the leading comment says which file of the library it checks)
        for word in ("orbx_", "orbslamm_", "include/", "orbslamm_amd/"):
            assert word not in code, "%s names %s" % (f, word)


def same(a, b):
    """equal as bits (NaNs included), dtype and shape too"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rot_axis_angle(axis, angle, scale_first=False):
    """Rodrigues' rotation in binary64.  scale_first writes the last term as ((1 - cos)*Kx) @ Kx, which is how the scenes of
    fuse_cases, localmap_cases and newpoints_cases were generated; it differs from (1 - cos)*(Kx @ Kx) in the last bit, and
    their seeds, floors and shares were measured on those scenes."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    KK = ((1 - np.cos(angle)) * Kx) @ Kx if scale_first else (1 - np.cos(angle)) * (Kx @ Kx)
    return np.eye(3) + np.sin(angle) * Kx + KK
