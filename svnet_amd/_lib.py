"""ctypes binding of libsvnet_hip.so (the C ABI declared in include/svnet_hip.h).

There is no CPU fallback: if the library is missing, or a tensor is not on a HIP device, the call
raises.  `build()` compiles the library in-tree with hipcc (gfx950 cross-compiles without a GPU).
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVNET_DIAG_LIB") or os.path.join(_HERE, "libsvnet_hip.so")    # (SVNET_DIAG_LIB: an ablation build, tools/ only)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "svnet_hip.h")
_lib = None

c_p = ctypes.c_void_p
c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_f = ctypes.c_float
c_sz = ctypes.c_size_t
SCALARS = {"int": c_int, "int64_t": c_i64, "float": c_f, "size_t": c_sz, "uint32_t": ctypes.c_uint32}     # every by-value type the header uses


class SvnetHipError(RuntimeError):
    pass


def _declare(text, structs, param):
    """[(name, ctype)] of one declaration `TYPE a, *b`.  A pointer is a c_void_p, or POINTER(struct) for a parameter that points at a
    parsed struct; a struct by value is a field only; anything else is a SCALARS entry or refused."""
    m = re.fullmatch(r"\s*(?:const\s+)?(\w+(?: \w+)*?)\s*(\*?\s*\b\w+(?:\s*,\s*\*?\s*\w+)*)\s*", text)
    if not m:
        raise SvnetHipError("svnet_hip.h: cannot parse the declaration %r" % text.strip())
    base, out = m.group(1), []
    for star, name in re.findall(r"(\*?)\s*(\w+)", m.group(2)):
        if star:
            out.append((name, ctypes.POINTER(structs[base]) if param and base in structs else c_p))
        elif base in SCALARS or (base in structs and not param):
            out.append((name, SCALARS.get(base) or structs[base]))
        else:
            raise SvnetHipError("svnet_hip.h: no ctypes type for %r in %r" % (base, text.strip()))
    return out


def parse_header(text):
    """(structs, signatures, defines) of a header in the dialect of include/svnet_hip.h: `typedef struct NAME { fields } NAME;`,
    `RET svnet_name(ARGS);` and `#define NAME integer`.  It is no C parser: whatever else it meets it refuses, quoting the text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    structs, signatures, defines = {}, {}, {}
    for name, params, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(\(?)[ \t]*(.*?)[ \t]*$", text, flags=re.M):
        if value and not params:                                # (the include guard has no value, SVNET_SLICED_LEN(L) takes a parameter)
            if not re.fullmatch(r"\d+|\(-\d+\)", value):
                raise SvnetHipError("svnet_hip.h: #define %s %s is not an integer" % (name, value))
            defines[name] = int(value.strip("()"))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def struct(m):
        if m.group(1) != m.group(3) or re.search(r"[{\[(:]|\bunion\b", m.group(2)):
            raise SvnetHipError("svnet_hip.h: cannot parse the struct %r" % m.group(0))
        fields = [f for decl in m.group(2).split(";") if decl.strip() for f in _declare(decl, structs, False)]
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    for decl in filter(str.strip, text.split(";")):
        m = re.fullmatch(r"\s*(?:(const\s+char\s*\*)|(\w+)\s)\s*(svnet_\w+)\s*\(([^()\[\]]*)\)\s*", decl)
        if not m or not (m.group(1) or m.group(2) in SCALARS):
            raise SvnetHipError("svnet_hip.h: cannot parse the declaration %r" % decl.strip())
        args = [] if m.group(4).strip() == "void" else [_declare(a, structs, True)[0][1] for a in m.group(4).split(",")]
        signatures[m.group(3)] = (ctypes.c_char_p if m.group(1) else SCALARS[m.group(2)], args)
    return structs, signatures, defines


# The header is the one statement of the ABI: struct layouts, name -> (restype, argtypes) of every entry point, and the constants.
with open(HEADER_PATH) as _f:
    STRUCTS, SIGNATURES, DEFINES = parse_header(_f.read())

GemmDesc = STRUCTS["svnet_gemm_desc"]
GateFwdJob = STRUCTS["svnet_gate_fwd_job"]
GateBwdJob = STRUCTS["svnet_gate_bwd_job"]
BlockTailDesc = STRUCTS["svnet_block_tail_desc"]
EdgeBlockDesc = STRUCTS["svnet_edgeblock_desc"]
EdgeBlockBwdDesc = STRUCTS["svnet_edgeblock_bwd_desc"]
XyzBlockDesc = STRUCTS["svnet_xyzblock_desc"]
XyzBlockBwdDesc = STRUCTS["svnet_xyzblock_bwd_desc"]
BinHeadDesc = STRUCTS["svnet_binhead_desc"]
BatchDesc = STRUCTS["svnet_batch_desc"]

ABI_VERSION = DEFINES["SVNET_ABI_VERSION"]      # argument lists / buffer-length contracts of the header; lib() refuses a library built for another
EDGE_FWD_TWO = DEFINES["SVNET_EDGE_FWD_TWO"]
WGRAD_TERN5, WGRAD_AFF2 = DEFINES["SVNET_WGRAD_TERN5"], DEFINES["SVNET_WGRAD_AFF2"]
KD_ROWS, KD_CHANNEL_MAJOR = DEFINES["SVNET_KD_ROWS"], DEFINES["SVNET_KD_CHANNEL_MAJOR"]
KD_WORKSPACE_FLOATS = DEFINES["SVNET_KD_WORKSPACE_FLOATS"]


def build(force=False, verbose=False):
    """Compile svnet_amd/csrc/*.hip into svnet_amd/libsvnet_hip.so (hipcc, --offload-arch=gfx950)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise SvnetHipError("building libsvnet_hip.so failed")
    return LIB_PATH


def lib():
    """The loaded library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SvnetHipError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (or make -C svnet_amd/csrc). "
                "svnet_amd has no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        if handle.svnet_version() != ABI_VERSION:               # a stale library: its entry points need not match the header's
            raise SvnetHipError("%s was built for ABI %d, include/svnet_hip.h declares %d (SVNET_ABI_VERSION): rebuild it"
                                % (LIB_PATH, handle.svnet_version(), ABI_VERSION))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().svnet_last_error()
        raise SvnetHipError("%s failed (%d): %s" % (what, code, msg.decode() if msg else "?"))


class KernelTimer:
    """Optional HIP-event stopwatch around ONE entry point (bench.py's roofline legs): events are recorded on
    the stream the kernel is launched on, immediately before and after the launch call.  `select(args)`
    may narrow the timing to launches with particular arguments (e.g. one layer's shape)."""

    def __init__(self, name, select=None):
        self.name, self.select, self.pairs = name, select, []

    def elapsed_ms(self):
        return [a.elapsed_time(b) for a, b in self.pairs]


TIMERS = []          # KernelTimer objects that are live (bench.py only; empty in normal operation)


class StepClock:
    """Diagnostic (tools/step_clock.py): start times of a step's C-ABI launches without a profiler.  While `CLOCK` is set, call()
    puts a one-thread kernel that stores the device's 100 MHz clock in front of every launch whose entry point passes `select`, on
    the launch's stream; captured into a HIP graph the stamps are replayed with it, and `read()` returns, for the last replay,
    [(microseconds since the first stamp, entry point, stream id)] in time order.  Each stamp costs ~2 us of stream time."""

    def __init__(self, device, select=None, slots=4096):
        import torch
        self.buf = torch.zeros(slots, dtype=torch.int64, device=device)
        self.names, self.select = [], select

    def mark(self, name):
        import torch
        if self.select is not None and not self.select(name):
            return
        i = len(self.names)
        if i >= self.buf.numel():
            return
        st = torch.cuda.current_stream(self.buf.device)
        self.names.append((name, st.cuda_stream))
        lib().svnet_stamp_u64(ctypes.c_void_p(self.buf.data_ptr() + 8 * i), ctypes.c_void_p(st.cuda_stream))

    def read(self):
        t = self.buf[:len(self.names)].cpu().tolist()
        t0 = min(t) if t else 0
        return sorted(((x - t0) / 100.0, n, s) for x, (n, s) in zip(t, self.names))


CLOCK = None         # a StepClock while tools/step_clock.py measures; None in normal operation


def call(name, *args):
    """Invoke one C-ABI entry point and raise on a non-zero return code."""
    fn = getattr(lib(), name)
    if CLOCK is not None:
        CLOCK.mark(name)
    hit = [t for t in TIMERS if t.name == name and (t.select is None or t.select(args))] if TIMERS else None
    if hit:
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream()
        a.record(st)
        rc = fn(*args)
        b.record(st)
        for t in hit:
            t.pairs.append((a, b))
    else:
        rc = fn(*args)
    check(rc, name)
