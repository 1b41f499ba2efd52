"""The bundle-adjustment pieces beside the g2o core (orbslamm_amd/csrc/orbg_schur.hip) on the host, no GPU: its scalar pieces are
__host__ __device__, and tests/cpp/schur_core_check.hip holds their host instantiations -- the two-vertex edge with both Jacobians,
BaseBinaryEdge's quadratic form (robust and plain, free and fixed pose), Eigen's 3 x 3 inverse, a landmark's Schur share, the
back-substitution, the reduced system's assembly and the unpivoted LDLt at 6 and 12 -- to the restatement's functions
(tools/initmap_ref.hpp) as bits on seeded inputs.  The reduced solve's refusals and a point on a camera's plane are reached by few
of the scene families; the program's classes reach them, and it asserts that none of its classes is empty.  The same program is
built once more with the address and undefined-behaviour sanitizers on its host code and run as a stand-alone program."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbslamm_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "schur_core_check.hip")


def _run(exe):
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    print(out)
    assert run.returncode == 0 and "MISMATCH" not in out and "EMPTY" not in out and out.rstrip().endswith("schur core ok"), out
    return out


def test_host_instantiations_equal_the_restatement_by_bits(tmp_path):
    exe = str(tmp_path / "schur_core_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-o", exe, SOURCE])
    out = _run(exe)
    m = re.search(r"inverse3: (\d+) regular, (\d+) not finite", out)
    assert m and all(int(g) > 0 for g in m.groups()), out
    for n in (6, 12):
        m = re.search(r"ldlt_plain<%d>: (\d+) solved, (\d+) zero pivots, (\d+) pivots not finite" % n, out)
        assert m and all(int(g) > 0 for g in m.groups()), out
    m = re.search(r"points: (\d+) \((\d+) robust edges, (\d+) with the Huber branch, (\d+) plain, (\d+) on fixed poses, (\d+) points on a camera's plane\)", out)
    assert m and all(int(g) > 0 for g in m.groups()), out


def test_the_same_program_under_the_host_sanitizers(tmp_path):
    """address and undefined-behaviour sanitizers on the HOST code of the program (its own main, no device, nothing loaded into
    python): an index past a block, a stack array or the reduced system's 144 words would end it"""
    exe = str(tmp_path / "schur_core_check_san")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, SOURCE])
    out = _run(exe)
    assert "runtime error" not in out and "AddressSanitizer" not in out


def test_the_new_file_needs_nothing_of_the_library():
    """orbg_schur.hip includes orbg_kernels.hip alone, and the initial map's kernels ask it, not the other way round"""
    text = open(os.path.join(CSRC, "orbg_schur.hip")).read()
    assert re.findall(r"#include (\S+)", text) == ['"orbg_kernels.hip"']
    code = text.split("#pragma once", 1)[1]
    for word in ("orbm::", "orbx::", "orbo::", "orbb::", "Orbb", "ORBB_"):
        assert word not in code, word
    assert "orbg::levenberg_full" in open(os.path.join(CSRC, "orbb_kernels.hip")).read()
