"""The g2o / Eigen core of the device optimizers (orbslamm_amd/csrc/orbg_kernels.hip) on the host, no GPU: its scalar pieces are
__host__ __device__, and tests/cpp/g2o_core_check.hip holds their host instantiations -- ldlt_solve<6> and <7>, sincos_defined,
exp_defined, the NaN canonicalisers, quat_of_matrix, normalize_rotation, and the two oplus functions and the Sim3 inverse that
are built from the shared quaternion and so(3) pieces -- to the restatements' Defined functions (tools/poseopt_ref.hpp,
tools/sim3opt_ref.hpp) as bits on seeded inputs.  The scene families of the GPU tests never take the LDLT's cutoff break and never
refuse a finite matrix; the program's matrix classes do, and it asserts that none of its classes is empty."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbslamm_amd", "csrc")


def test_host_instantiations_equal_the_restatements_by_bits(tmp_path):
    exe = str(tmp_path / "g2o_core_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpp", "g2o_core_check.hip")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    print(out)
    assert run.returncode == 0 and "MISMATCH" not in out and out.rstrip().endswith("g2o core: all equal"), out
    for n in (6, 7):
        m = re.search(r"ldlt_solve<%d>: .*zero rows and columns (\d+), negated (\d+), indefinite (\d+), zero 1, NaN on the diagonal (\d+), NaN off it (\d+), "
                      r"one infinity (\d+); solved (\d+), refused (\d+)" % n, out)
        assert m and all(int(g) > 0 for g in m.groups()), out
    m = re.search(r"sincos_defined: (\d+) arguments", out)
    assert m and int(m.group(1)) >= 10 ** 6
    m = re.search(r"exp_defined: (\d+) arguments", out)
    assert m and int(m.group(1)) >= 10 ** 6
    m = re.search(r"positive trace (\d+), largest diagonal 0 / 1 / 2: (\d+) / (\d+) / (\d+)", out)
    assert m and all(int(g) > 0 for g in m.groups())
    m = re.search(r"theta below / above 1e-5: (\d+) / (\d+), \|sigma\| above with theta below / above: (\d+) / (\d+); fix_scale (\d+)", out)
    assert m and all(int(g) > 0 for g in m.groups())


def test_each_shared_piece_is_defined_once():
    """the pieces the two optimizers share have one definition under csrc, in orbg_kernels.hip, and orbz asks orbo for nothing"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".inc", ".h"))}
    defs = {"ldlt_solve": r"bool ldlt_solve\w*\(", "load_edge": r"EdgeReg load_edge\(", "edge_chi2": r"double edge_chi2\(", "rotate": r"void rotate\(",
            "EdgeReg": r"struct EdgeReg\b", "the lambda growth": r"lambda \*= (st\.)?growth", "sincos_defined": r"void sincos_defined\(",
            "exp_defined": r"double exp_defined\(", "quat_of_matrix": r"quat_of_matrix\(const", "huber": r"void huber\(", "wave_sum": r"double wave_sum\("}
    for what, pat in defs.items():
        where = [f for f, t in text.items() for _ in re.findall(pat, t)]
        assert where == ["orbg_kernels.hip"], (what, where)
    assert "orbo::" not in text["orbz_kernels.hip"] and "orbz::oplus" in text["orbz_kernels.hip"]
    assert re.findall(r"#include (\S+)", text["orbg_kernels.hip"]) == ["<hip/hip_runtime.h>", "<cstdint>"]
