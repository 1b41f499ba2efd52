"""ctypes loader for liborbslamm_hip.so (the C ABI of include/orbslamm_hip.h).

The library is the product: there is no Python/CPU compute path behind it.  If
the shared object is missing this module raises -- loudly -- instead of falling
back to anything."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
SO_PATH = os.path.join(_PKG, "liborbslamm_hip.so")
SRC = os.path.join(_PKG, "csrc", "orbslamm_hip.hip")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]

ORBX_MAX_LEVELS = 16
ORBX_PROF_MAX = 16
ORBX_OK, ORBX_E_INVALID, ORBX_E_NO_DEVICE, ORBX_E_HIP, ORBX_E_CAPACITY, ORBX_E_UNSUPPORTED = 0, -1, -2, -3, -4, -5

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


class OrbxParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scaleFactor", C.c_float), ("nlevels", C.c_int32),
                ("iniThFAST", C.c_int32), ("minThFAST", C.c_int32)]


class OrbxProfile(C.Structure):
    _fields_ = [("n", C.c_int32), ("name", C.c_char_p * ORBX_PROF_MAX), ("ms", C.c_double * ORBX_PROF_MAX),
                ("launches", C.c_int64 * ORBX_PROF_MAX)]


class OrbxStreamOpts(C.Structure):
    _fields_ = [("match_prev", C.c_int32), ("nnratio", C.c_float), ("th_low", C.c_int32), ("check_ori", C.c_int32)]


class OrbxBatchView(C.Structure):
    _fields_ = [("B", C.c_int32), ("cap", C.c_int32), ("n", C.c_void_p), ("kps", C.c_void_p), ("desc", C.c_void_p),
                ("match", C.c_void_p), ("nmatch", C.c_void_p)]


class OrbxBatchOut(C.Structure):
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_void_p), ("match", C.c_void_p), ("nmatch", C.c_void_p), ("cap", C.c_int32)]


class OrbmFeatVec(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("start", C.c_void_p), ("idx", C.c_void_p)]


class OrbmGrid(C.Structure):
    _fields_ = [("minX", C.c_float), ("minY", C.c_float), ("invW", C.c_float), ("invH", C.c_float),
                ("cols", C.c_int32), ("rows", C.c_int32)]


class OrbmProjParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("nnratio", C.c_float), ("check_ori", C.c_int32), ("th_dist", C.c_int32)]


# what a prototype of include/orbslamm_*.h may return and take by value; everything with a `*` or a `[`, and a `_fn` typedef, is a pointer
_RETURNS = {"int": C.c_int, "void": None, "float": C.c_float, "const char*": C.c_char_p}
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32,
            "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
Declaration = collections.namedtuple("Declaration", "restype argtypes header")
_declarations = None


def _parse_header(text, header):
    """{name: Declaration} of the prototypes `ret name(args);` in a header's text.  Comments, preprocessor lines, the extern "C"
    bracket, typedefs and whatever has a body are not prototypes; a statement that is none of these, or a type outside the two tables,
    raises -- a signature is never guessed"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?^[ \t]*#endif[^\n]*$", "", text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", "", text, flags=re.M)
    n = 1
    while n:
        text, n = re.subn(r"\{[^{}]*\}", "\0", text)          # a body, innermost first
    out = {}
    for stmt in re.sub(r"\)\s*\0", ")\0;", text).split(";"):   # a function's body ends its statement
        stmt = " ".join(stmt.split())
        if not stmt or stmt.startswith("typedef ") or "\0" in stmt:
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if not m:
            raise RuntimeError("%s: cannot read `%s` as a prototype" % (header, stmt))
        ret, name, params = re.sub(r" ?\* ?", "*", m.group(1).strip()), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise RuntimeError("%s: %s returns `%s`, which the mirror has no ctypes type for" % (header, name, ret))
        argtypes = []
        for prm in ([] if params in ("", "void") else params.split(",")):
            words = [w for w in prm.split() if w != "const"]
            kind = " ".join(words[:-1]) if len(words) > 1 else words[0] if words else ""
            if "*" in prm or "[" in prm or kind.endswith("_fn"):
                argtypes.append(C.c_void_p)
            elif kind in _SCALARS:
                argtypes.append(_SCALARS[kind])
            else:
                raise RuntimeError("%s: %s takes `%s`, which the mirror has no ctypes type for" % (header, name, prm.strip()))
        if name in out:
            raise RuntimeError("%s declares %s twice" % (header, name))
        out[name] = Declaration(_RETURNS[ret], argtypes, header)
    return out


def declarations():
    """{name: Declaration(restype, argtypes, header)} of every C entry include/orbslamm_*.h declares: the one statement of the ABI that a
    compiler checks, read once per process.  lib() installs it on the library; the tests take their lists of names from it"""
    global _declarations
    if _declarations is None:
        inc = os.path.join(_ROOT, "include")
        headers = sorted(f for f in os.listdir(inc) if re.fullmatch(r"orbslamm_\w+\.h", f)) if os.path.isdir(inc) else []
        if not headers:
            raise RuntimeError("%s holds no orbslamm_*.h: the signatures of liborbslamm_hip.so are read from these headers" % inc)
        decl = {}
        for f in headers:
            with open(os.path.join(inc, f)) as fh:
                one = _parse_header(fh.read(), f)
            twice = sorted(set(one) & set(decl))
            if twice:
                raise RuntimeError("%s declares %s again (%s has it)" % (f, twice[0], decl[twice[0]].header))
            if not one:     # e.g. an extern "C" bracket in a form this reader does not set aside swallows the whole header as a body
                raise RuntimeError("%s: no prototype read" % f)
            decl.update(one)
        _declarations = decl
    return _declarations


def build(force=False):
    """hipcc the extension in-tree for gfx950 (cross-compiles without a GPU)."""
    deps = [os.path.join(d, f) for d in (os.path.join(_PKG, "csrc"), os.path.join(_ROOT, "include")) for f in os.listdir(d)]
    if not force and os.path.exists(SO_PATH) and all(os.path.getmtime(SO_PATH) >= os.path.getmtime(d) for d in deps):
        return SO_PATH
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-o", SO_PATH, SRC]
    subprocess.check_call(cmd)
    return SO_PATH


_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so.7; if
    this library pulled in /opt/rocm's copy first, a later `import torch` in the same
    process would find the GPU already owned by the other runtime ("No HIP GPUs are
    available").  So when torch is installed, its runtime is loaded (not torch itself)
    before liborbslamm_hip.so, whose NEEDED libamdhip64.so.7 then resolves to it."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError("liborbslamm_hip.so is missing (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                               "there is no CPU fallback for the ORB front-end")
        _preload_hip_runtime()
        # ORBSLAMM_HIP_LIB: load another build of the same library (A/B timing of kernel variants, tools/ab_bench.sh)
        L = C.CDLL(os.environ.get("ORBSLAMM_HIP_LIB") or SO_PATH)
        for name, d in declarations().items():
            fn = getattr(L, name)     # every declared entry resolves, or this raises
            fn.restype, fn.argtypes = d.restype, d.argtypes
        _lib = L
    return _lib


class OrbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbslamm_hip error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    if rc != 0:
        raise OrbError(rc, lib().orbx_last_error().decode(errors="replace"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def table(arrays):
    """the pointer table of per-job arrays (None: a null inside it)"""
    return (C.c_void_p * max(len(arrays), 1))(*[None if a is None else a.ctypes.data for a in arrays])


def handle_value(fs):
    """a frame set's handle as the integer a job record holds: of a FrameSet, a c_void_p or a raw value (None: 0)"""
    h = getattr(fs, "_h", fs)
    return (h.value if isinstance(h, C.c_void_p) else h) or 0


def K4(K):
    """a camera matrix as the C ABI takes it: float32 (fx, fy, cx, cy), from that or from the 3x3 K"""
    K = np.asarray(K, dtype=np.float32)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=np.float32)
    return np.ascontiguousarray(K.reshape(4))


RAND_MAX = 2147483647   # glibc's
_libc = None


def libc():
    """the process's libc, for the rand() stream the reference's RANSAC draws consume"""
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.rand.restype = C.c_int
    return _libc


def seed_rand(seed):
    """DUtils::Random::SeedRandOnce(seed) is srand(seed); None continues the process's stream"""
    if seed is not None:
        libc().srand(C.c_uint(int(seed)))


def random_int(k):
    """DUtils::Random::RandomInt(0, k - 1): int(rand() / (RAND_MAX + 1.0) * k), one call of libc's rand()"""
    return int((float(libc().rand()) / (RAND_MAX + 1.0)) * k)


def device_pci_bus_id(device):
    """"0000:c1:00.0" or None"""
    buf = C.create_string_buffer(32)
    try:
        return buf.value.decode().lower() if lib().orbx_device_pci_bus_id(int(device), buf, 32) == 0 else None
    except Exception:
        return None


def shader_clock_mhz(device):
    """the shader clock the device runs at now (orbx_device_shader_clock_mhz), or None"""
    v = C.c_float(0)
    try:
        return float(v.value) if lib().orbx_device_shader_clock_mhz(int(device), C.byref(v)) == 0 else None
    except Exception:
        return None


def numa_cpus_of_device(device):
    """(numa node, cpu ids) next to a HIP device, from sysfs; (None, None) where the platform does not say"""
    buf = C.create_string_buffer(32)
    try:
        if lib().orbx_device_pci_bus_id(int(device), buf, 32) != 0:
            return None, None
        bus = buf.value.decode().lower()
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bus).read())
        if node < 0:
            return None, None
        cpus = []
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.extend(range(int(a), int(b or a) + 1))
        return node, cpus
    except (OSError, ValueError):
        return None, None
