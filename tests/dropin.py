"""How a drop-in program (tests/cpp/<name>.cpp: a header of include/ instantiated on mocks, linked to the library) is built and
run.  One set of flags for all of them: warnings are errors, and -ffp-contract=off because the programs compare floats by
bits against restatements that are built the same way (ref_shim.py)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", CPP, "-I", os.path.join(ROOT, "tools")]
WARN = ["-std=c++11", "-Wall", "-Werror"]


def _source(name_or_path):
    return name_or_path if os.path.isabs(name_or_path) else os.path.join(CPP, name_or_path + ".cpp")


def build(name, extra=(), oracle=False, opt="-O2", pthread=True):
    """tests/cpp/<name>.cpp as a program in a fresh temporary directory, linked to the library (built first if it is stale)
    and, when asked, to the oracle; `extra` goes in front of the source (-D, -I).  Returns the program's path."""
    from orbslamm_amd import _lib
    _lib.build()
    dirs = [os.path.join(ROOT, "orbslamm_amd")]
    libs = ["-lorbslamm_hip"]
    if oracle:
        from oracle import binding
        binding.build()
        dirs.append(os.path.join(ROOT, "oracle"))
        libs.append("-lorb_oracle")
    exe = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name)
    subprocess.check_call(["g++"] + WARN + [opt, "-ffp-contract=off"] + (["-pthread"] if pthread else []) + INCLUDES + list(extra) +
                          [_source(name), "-o", exe] + ["-L" + d for d in dirs] + libs +
                          ["-Wl,-rpath," + d for d in dirs + ["/opt/rocm/lib"]])
    return exe


def run(exe, *args, timeout=None, marker=None):
    """runs the program; it must exit 0 and, when a marker is given, print it.  Returns its standard output."""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, errors="replace", timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert marker is None or marker in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


def syntax_only(name_or_path, includes=()):
    """g++ -fsyntax-only of tests/cpp/<name>.cpp (or of a path), warnings as errors: a header instantiated on its mocks where
    nothing can be linked or run"""
    subprocess.check_call(["g++"] + WARN + ["-fsyntax-only"] + INCLUDES + [a for d in includes for a in ("-I", d)] + [_source(name_or_path)])
