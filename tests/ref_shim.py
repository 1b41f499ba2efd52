"""Builds a restatement's C shim (tests/cpp/*_ref_capi.cpp over tools/*_ref.hpp) with g++ -ffp-contract=off into a
temporary directory and loads it: the checkers' side of init_cases.py and sim3_cases.py."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_ref_shim(name):
    """tests/cpp/<name>_capi.cpp as a loaded shared object"""
    out = os.path.join(tempfile.mkdtemp(prefix=name + "_"), "lib%s.so" % name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", name + "_capi.cpp"), "-o", out])
    return C.CDLL(out)


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
