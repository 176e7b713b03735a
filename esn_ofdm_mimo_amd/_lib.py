"""ctypes binding of libesn_hip.so, read from include/esn_hip.h: the header is the one statement of the C ABI.
SIGNATURES, the enum constants and ABI_VERSION are parsed from it when this module is imported (regular expressions
over plain C99 text; no compiler, no library and no GPU needed), so a new entry point is declared in the header,
defined in csrc/esn_api.hip, and there is nothing to type here.  Fails loudly: a declaration the parser cannot type,
a missing library or a missing GPU is an error, never a guess or a silent CPU path."""
import ctypes as C
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ESN_HIP_LIB") or os.path.join(_PKG, "libesn_hip.so")   # env: tuning builds only
HEADER_PATH = os.path.join(_PKG, "..", "include", "esn_hip.h")


class Shape(C.Structure):                        # struct esn_shape; callers construct it positionally
    _fields_ = [("n_res", C.c_int), ("n_in", C.c_int), ("n_out", C.c_int),
                ("teacher_forcing", C.c_int), ("n_wsets", C.c_int),
                ("leak_rate", C.c_double)]       # extension: 0 or 1 = the reference's update (include/esn_hip.h)


class EsnHipError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "double": C.c_double,
            "uint64_t": C.c_uint64, "size_t": C.c_size_t, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong}
# pointers travel as integers (c_void_p: device pointers, streams, NULL) but for these two pointees
_POINTEES = {"char": C.c_char_p, "esn_shape_t": C.POINTER(Shape)}


def strip_header(text):
    """C99 text without block comments, line comments and preprocessor lines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)


def _ctype(decl, where):
    """ctypes type of one return type or parameter (its name, if any, included)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return _POINTEES.get(" ".join(words[:words.index("*")]), C.c_void_p)
    if words[:1] == ["enum"] and len(words) in (2, 3):
        return C.c_int
    for n in (len(words), len(words) - 1):       # unnamed, then named
        if " ".join(words[:n]) in _SCALARS and all(w.isidentifier() for w in words[n:]):
            return _SCALARS[" ".join(words[:n])]
    raise EsnHipError(f"{where}: cannot type `{' '.join(decl.split())}`; teach esn_ofdm_mimo_amd/_lib.py the type")


def parse_signatures(text):
    """{name: (restype, argtypes)} of every `ret esn_name(args);` of a header text."""
    text = strip_header(text)
    out = {}
    for statement in re.split(r"[;{}]", text):
        m = re.fullmatch(r"([^()]*?)\b(esn_\w+)\s*\(([^()]*)\)\s*", statement)
        if not m:
            continue                             # enumerators, struct members, extern "C"; `missed` below names the rest
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else args.split(",")
        out[name] = (_ctype(ret, name), [_ctype(a, name) for a in args])
    missed = sorted(set(re.findall(r"\b(esn_\w+)\s*\(", text)) - set(out))
    if missed:
        raise EsnHipError(f"cannot read the declaration of {', '.join(missed)}")
    return out


def parse_enums(text):
    """{enum tag: {enumerator: value}} of a header text."""
    out = {}
    for tag, body in re.findall(r"\benum\s+(\w+)\s*\{([^{}]*)\}", strip_header(text)):
        out[tag], value = {}, -1
        for item in filter(str.strip, body.split(",")):
            name, _, given = item.partition("=")
            value = int(given, 0) if given.strip() else value + 1
            out[tag][name.strip()] = value
    return out


def parse_define(text, name):
    """Integer value of `#define name value` in a header text."""
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(-?\w+)[ \t]*$" % re.escape(name),
                  re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.M)
    if not m:
        raise EsnHipError(f"{name} is not defined")
    return int(m.group(1), 0)


with open(HEADER_PATH) as _f:
    _HEADER = _f.read()
SIGNATURES = parse_signatures(_HEADER)
# the one override: esn_device_info fills three host ints, passed with byref(c_int()); every other pointer is an address
SIGNATURES["esn_device_info"][1][:3] = [C.POINTER(C.c_int)] * 3
ENUMS = parse_enums(_HEADER)
ABI_VERSION = parse_define(_HEADER, "ESN_ABI_VERSION")

F64, F32, F16, BF16 = (ENUMS["esn_precision"][k] for k in ("ESN_F64", "ESN_F32", "ESN_F16", "ESN_BF16"))
PRECISIONS = {"f64": F64, "f32": F32, "f16": F16, "bf16": BF16}
NOISE_NONE, NOISE_TENSOR, NOISE_COUNTER = (ENUMS["esn_noise_mode"][k] for k in
                                           ("ESN_NOISE_NONE", "ESN_NOISE_TENSOR", "ESN_NOISE_COUNTER"))
MEM_DEVICE, MEM_HOST = (ENUMS["esn_mem_kind"][k] for k in ("ESN_MEM_DEVICE", "ESN_MEM_HOST"))
# enum esn_path, by value: the recurrence kernel a call dispatches to (recur_path below)
PATHS = tuple(k[len("ESN_PATH_"):].lower() for k, v in sorted(ENUMS["esn_path"].items(), key=lambda kv: kv[1]))
if sorted(ENUMS["esn_path"].values()) != list(range(len(PATHS))):
    raise EsnHipError("enum esn_path must count 0, 1, 2, ...: PATHS is indexed by value")

_lib = None


def load():
    """Load (once) and type the library.  Raises EsnHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EsnHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the ESN hot path.")
    # torch first: libesn_hip.so must resolve libamdhip64 to the copy torch has already loaded -- loaded before torch it
    # binds the system ROCm runtime instead, the process ends up with two HIP runtimes and every launch of this
    # library fails with hipErrorNoDevice (seen with build() + smoke() in one process)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.esn_abi_version() != ABI_VERSION:
        raise EsnHipError(f"libesn_hip.so ABI {lib.esn_abi_version()} != binding {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().esn_last_error().decode(errors="replace")
        raise EsnHipError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """data_ptr of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise EsnHipError("no HIP device visible: the ESN hot path runs on the GPU only "
                          "(no CPU fallback is provided)")
    return torch


def stream_handle():
    import torch
    return torch.cuda.current_stream().cuda_stream


def debug_set(key, value):
    """Tuning knob of the library (benchmarks / A-B tests): see esn_debug_set in include/esn_hip.h."""
    check(load().esn_debug_set(key.encode(), None if value is None else str(value).encode()), "esn_debug_set")


def recur_path(harvest, precision, shape, n_sequences, frames_per_group=1, have_workspace=True):
    """Name (PATHS) of the kernel esn_harvest_batch (harvest) / esn_predict_batch runs for this call under the current
    knobs: esn_recur_path in include/esn_hip.h.  `precision` is a key of PRECISIONS."""
    rc = load().esn_recur_path(int(bool(harvest)), PRECISIONS[precision], C.byref(shape), int(n_sequences),
                               int(frames_per_group), int(bool(have_workspace)))
    if rc < 0:
        check(rc, "esn_recur_path")
    return PATHS[rc]


def device_info():
    lib = load()
    cu, lds, clk = C.c_int(), C.c_int(), C.c_int()
    name = C.create_string_buffer(64)
    check(lib.esn_device_info(C.byref(cu), C.byref(lds), C.byref(clk), name, 64), "esn_device_info")
    return dict(cu_count=cu.value, lds_bytes_per_cu=lds.value, clock_khz=clk.value,
                arch=name.value.decode())
