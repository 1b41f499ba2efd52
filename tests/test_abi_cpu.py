"""The C-ABI library loads, exports exactly the symbols include/orbslamm_*.h declare,
its host-side tables agree with the oracle, and compute entries refuse to run
without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dynamic_symbols(path):
    """the defined dynamic symbols of a shared object, by whichever of nm and llvm-readelf is here; None without either"""
    import shutil
    import subprocess
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.split()}
    if shutil.which("llvm-readelf"):
        out = subprocess.run(["llvm-readelf", "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
        rows = [line.split() for line in out.splitlines()]
        return {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    return None


def test_the_mirror_reads_its_signatures_from_the_headers():
    """_lib.declarations() is the library's ABI as include/orbslamm_*.h states it: the derivation pinned on entries that use every
    form, a type outside the table refused, and the declared names equal to the library's defined dynamic symbols in both directions"""
    from orbslamm_amd import _lib
    d = _lib.declarations()
    vp, i = C.c_void_p, C.c_int
    assert (d["orbx_last_error"].restype, d["orbx_last_error"].argtypes) == (C.c_char_p, [])
    assert d["orbx_scale_factor"].restype is C.c_float and d["orbm_destroy"].restype is None and d["orbx_create"].restype is i
    assert d["orbx_extract_batch_device"].argtypes == [vp, vp, i, i, i, i, C.c_size_t]
    a = d["orbq_track_reference"].argtypes
    assert len(a) == 14 and a[5] is C.c_float and [k for k, t in enumerate(a) if t is i] == [4, 6, 7, 9]
    assert [k for k, t in enumerate(a) if t is vp] == [0, 1, 2, 3, 8, 10, 11, 12, 13]
    assert d["orbq_relocalize"].argtypes[-3:] == [vp, vp, vp] and d["orbq_relocalize"].header == "orbslamm_reloc.h"   # int32_t* const*, uint8_t* const*
    assert d["orbm_frameset_create"].argtypes[3] is vp                                                                 # const float K[4]
    assert d["orbl_level_breaks"].argtypes == [C.c_float, i, vp, vp]                                                   # orbl_predict_fn
    assert d["orbk_detect_loop_candidates"].argtypes == [vp, i, C.c_uint64, vp, i, C.c_float, vp, vp, vp, i, vp]                     # orbk_neighbours_fn at 6
    assert d["orbm_descriptors_to_text"].argtypes == [vp, i, i, vp, C.c_size_t, vp]                                    # size_t, size_t*
    assert "orbq_reloc_n_good" not in d            # it has a body in its header: not an entry of the library
    assert len(d) >= 195 and len({x.header for x in d.values()}) >= 13
    # fed as text: the forms above parse, a type the table does not know raises and names the entry and the header
    one = _lib._parse_header("/* c */\n#define X 1\nint orbx_f(const float K[4], size_t n, orbl_predict_fn fn); // d\nvoid orbx_g(void);", "t.h")
    assert one == {"orbx_f": (i, [vp, C.c_size_t, vp], "t.h"), "orbx_g": (None, [], "t.h")}
    for text in ("int orbx_f(long n);", "int orbx_f(OrbmGrid grid);", "long orbx_f(int n);", "float* orbx_f(int n);", "int orbx_f(unsigned);"):
        with pytest.raises(RuntimeError, match=r"t\.h.*orbx_f"):
            _lib._parse_header(text, "t.h")
    L = _lib.lib()
    for name, x in d.items():
        fn = getattr(L, name)
        assert fn.restype is x.restype and list(fn.argtypes) == x.argtypes, name
    exported = dynamic_symbols(os.environ.get("ORBSLAMM_HIP_LIB") or _lib.SO_PATH)
    if exported is None:
        pytest.skip("neither nm nor llvm-readelf is on this machine: the library's symbols are not compared with the headers (the rest passed)")
    assert sorted(d) == sorted(n for n in exported if re.fullmatch(r"orb[a-z]_[a-z0-9_]+", n))


@pytest.mark.parametrize("nf,sf,nl", [(1000, 1.2, 8), (2000, 1.2, 8), (4000, 1.2, 8), (500, 1.5, 5), (1500, 1.1, 12)])
def test_host_tables_match_oracle(oracle, nf, sf, nl):
    from orbslamm_amd import ORBextractor
    ex = ORBextractor(nf, sf, nl, 20, 7, max_width=752, max_height=480, device=-1)
    oe = oracle.Extractor(nf, sf, nl, 20, 7)
    assert ex.GetLevels() == nl
    assert ex.GetScaleFactor() == np.float32(sf)
    assert np.array_equal(ex.GetScaleFactors(), oe.scale_factors())
    assert np.array_equal(ex.GetInverseScaleFactors(), np.array(oe.ex.mvInvScaleFactor[:nl], dtype=np.float32))
    assert np.array_equal(ex.GetScaleSigmaSquares(), np.array(oe.ex.mvLevelSigma2[:nl], dtype=np.float32))
    assert np.array_equal(ex.GetInverseScaleSigmaSquares(), np.array(oe.ex.mvInvLevelSigma2[:nl], dtype=np.float32))
    assert ex.features_per_level().tolist() == oe.features_per_level()
    assert ex.umax().tolist() == oe.umax()
    assert ex.max_keypoints >= nf


def test_bad_parameters_are_rejected():
    from orbslamm_amd import ORBextractor, OrbError
    for args in [(0, 1.2, 8, 20, 7), (1000, 1.0, 8, 20, 7), (1000, 1.2, 0, 20, 7), (1000, 1.2, 17, 20, 7)]:
        with pytest.raises(OrbError) as e:
            ORBextractor(*args, device=-1)
        assert e.value.code == -1


def test_no_cpu_fallback():
    """Without a device the product refuses to compute.  (On the GPU box this test is
    still valid: the host-only handle must refuse regardless.)"""
    from orbslamm_amd import ORBextractor, OrbError
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-1)
    with pytest.raises(OrbError) as e:
        ex(np.zeros((480, 640), np.uint8))
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_product_never_imports_oracle():
    """grep-level guard: nothing under orbslamm_amd/ or include/ references oracle/"""
    for base in ("orbslamm_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".inc")):
                    txt = open(os.path.join(dp, f), errors="replace").read()
                    assert "oracle" not in txt.lower().replace("no cpu fallback", ""), os.path.join(dp, f)


def test_mapserializer_descriptor_text():
    """`os << pKF->mDescriptors` (src/MapSerializer.cc:344-347): OpenCV 3.0's default cv::Mat formatter for CV_8U --
    "[" rows "]", "%3d" elements, ", " between elements, ";\\n " between rows.  Host-side formatting: runs without a GPU."""
    from orbslamm_amd import matcher
    m = np.array([[1, 20, 255], [0, 7, 100]], dtype=np.uint8)
    assert matcher.descriptors_to_text(m) == "[  1,  20, 255;\n   0,   7, 100]"
    assert matcher.descriptors_to_text(np.zeros((0, 32), np.uint8)) == "[]"
    rng = np.random.default_rng(3)
    d = rng.integers(0, 256, size=(57, 32), dtype=np.uint8)
    t = matcher.descriptors_to_text(d)
    assert t.count("\n") == 56 and t.count(",") == 57 * 31 and len(t) == 2 + 57 * (32 * 3 + 31 * 2) + 56 * 3
    assert np.array_equal(matcher.descriptors_from_text(t), d)
    one = matcher.descriptors_to_text(d[5])       # MapPoint::GetDescriptor(): 1 x 32
    assert one.startswith("[") and "\n" not in one and np.array_equal(matcher.descriptors_from_text(one)[0], d[5])
    from orbslamm_amd import OrbError
    with pytest.raises(OrbError):
        matcher.descriptors_from_text("[1, 2; 3]", cols=2)


def test_multi_robot_example_builds_against_the_abi():
    """examples/multi_robot.cpp (the reference's multi-robot main loop on the C ABI + RCCL) compiles and links here, where
    there is no GPU; without one it refuses to run instead of falling back to anything"""
    import subprocess
    import __graft_entry__ as ge
    exe = ge.build_examples(force=True)
    r = subprocess.run([exe, "--frames", "1"], capture_output=True, text=True, timeout=120)
    from orbslamm_amd import _lib
    if _lib.lib().orbx_device_count() == 0:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr


def test_staging_row_copy_equals_memcpy():
    """orbx_debug_stage_rows: the streaming-store row copy of the pageable-frame staging (orbx_handle.inc stage_rows) against a
    plain copy -- widths with every tail length, unaligned sources, aligned and unaligned destinations (the latter take memcpy),
    bytes outside the rows untouched"""
    from orbslamm_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7)
    ran_streaming = 0
    for w in list(range(120, 200)) + [1241, 640, 1920, 1279]:
        for src_off, dst_off in ((0, 0), (1, 0), (13, 0), (5, 32), (0, 8)):
            rows, spitch, dpitch = 7, w + 19, (w + 63) // 64 * 64 + 64
            src = rng.integers(0, 256, rows * spitch + 64, dtype=np.uint8)
            raw = np.full(rows * dpitch + 128, 0xA5, dtype=np.uint8)
            base = (-raw.ctypes.data) % 64 + dst_off      # 64-byte aligned start, then the offset under test
            rc = L.orbx_debug_stage_rows(raw.ctypes.data + base, dpitch, src.ctypes.data + src_off, spitch, w, rows)
            assert rc >= 0
            ran_streaming += rc
            want = np.full_like(raw, 0xA5)
            for y in range(rows):
                want[base + y * dpitch: base + y * dpitch + w] = src[src_off + y * spitch: src_off + y * spitch + w]
            assert np.array_equal(raw, want), (w, src_off, dst_off)
    assert L.orbx_debug_stage_rows(None, 0, None, 0, 0, 0) < 0
    import platform
    if platform.machine() == "x86_64" and os.environ.get("ORBX_STAGE_NT") != "0":
        assert ran_streaming > 0   # the aligned cases took the streaming path on this host
