"""CPU tests of the binding's one source: svnet_amd/_lib.py derives its ctypes structs, argument lists and constants from
include/svnet_hip.h.  The witnesses here are independent of that parser: the host C compiler for the layouts, a plain regex and the built
library for the names, synthetic headers for what the parser must refuse."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from svnet_amd import _lib
from svnet_amd._lib import SvnetHipError, parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "svnet_hip.h")


def _host_cc():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cc in ("cc", os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "llvm", "bin", "clang")):
        path = shutil.which(cc)
        if path:
            return path
    pytest.fail("no host C compiler (cc, or the clang of the ROCm tree): build() needs one as well")


def test_struct_layouts_equal_the_host_compilers(tmp_path):
    """sizeof of every parsed struct and offsetof of every parsed field, as the C compiler lays the header out, against ctypes."""
    lines, want = [], {}
    for name, cls in _lib.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want[name] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
            want["%s.%s" % (name, field)] = getattr(cls, field).offset
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "svnet_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([_host_cc(), "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert len(got) == sum(len(c._fields_) for c in _lib.STRUCTS.values()) + len(_lib.STRUCTS)
    assert len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", open(HEADER).read()))     # no struct was passed over


def test_every_declared_entry_point_is_parsed_and_exported():
    header = open(HEADER).read()
    declared = set(re.findall(r"\b(svnet_[a-z0-9_]+)\s*\(", header)) - set(_lib.STRUCTS)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", header))
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert {n for n in _lib.SIGNATURES if hasattr(handle, n)} == declared


@pytest.mark.parametrize("text,quoted", [
    ("int svnet_f(__int128 x);", "__int128"),                                       # a type outside the table
    ("typedef struct svnet_s { unsigned x; } svnet_s;", "unsigned"),
    ("int svnet_f(float x[3]);", "float x[3]"),                                     # an array parameter
    ("typedef struct svnet_s { float x[3]; } svnet_s;", "float x[3]"),
    ("int svnet_f(int (*cb)(int), void* stream);", "(*cb)"),                        # a function pointer
    ("typedef struct svnet_s { int a; } svnet_s;\nint svnet_f(svnet_s s);", "svnet_s s"),      # a struct by value as a parameter
    ("typedef struct svnet_s { int a : 3; } svnet_s;", "a : 3"),                    # a bit-field
    ("typedef struct svnet_s { union { int a; float b; } u; } svnet_s;", "union"),
    ("int svnet_f(int a)\nint svnet_g(void);", "svnet_f(int a)"),                   # a declaration that does not end in `);`
    ("int svnet_f(int a", "svnet_f(int a"),
    ("void svnet_f(int a);", "void svnet_f"),                                       # a return type outside the table
    ("int svnet_f(float** rows);", "float** rows"),
    ("#define SVNET_HALF 0.5", "SVNET_HALF"),
])
def test_parser_refuses_what_it_does_not_understand(text, quoted):
    with pytest.raises(SvnetHipError) as err:
        parse_header(text)
    assert quoted in str(err.value)


def test_parser_reads_a_well_formed_header():
    structs, signatures, defines = parse_header("""
        #ifndef SVNET_T_H
        #define SVNET_T_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define SVNET_T_A 7     /* a comment with svnet_not_a_function( in it */
        #define SVNET_T_B (-3)
        #define SVNET_T_LEN(L) (2 * (L))
        typedef struct svnet_in { const float *a, *b; int64_t M, N; float s; } svnet_in;
        typedef struct svnet_out {
            int n; svnet_in in;        /* by value */
            long long* nbt; size_t bytes; uint32_t mask;
        } svnet_out;
        int svnet_t_run(const svnet_out* d, const uint64_t* planes, int64_t n, float x /* unit */, size_t bytes,
                        uint32_t mask, void* stream);
        const char* svnet_t_error(void);
        size_t svnet_t_bytes(int64_t n);
        int64_t svnet_t_stride(int n);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    c_p, c_i64, c_int, c_f, c_sz, c_u32 = _lib.c_p, _lib.c_i64, _lib.c_int, _lib.c_f, _lib.c_sz, ctypes.c_uint32
    assert defines == {"SVNET_T_A": 7, "SVNET_T_B": -3}
    assert list(structs) == ["svnet_in", "svnet_out"]
    assert structs["svnet_in"]._fields_ == [("a", c_p), ("b", c_p), ("M", c_i64), ("N", c_i64), ("s", c_f)]
    assert structs["svnet_out"]._fields_ == [("n", c_int), ("in", structs["svnet_in"]), ("nbt", c_p), ("bytes", c_sz), ("mask", c_u32)]
    assert signatures == {
        "svnet_t_run": (c_int, [ctypes.POINTER(structs["svnet_out"]), c_p, c_i64, c_f, c_sz, c_u32, c_p]),
        "svnet_t_error": (ctypes.c_char_p, []),
        "svnet_t_bytes": (c_sz, [c_i64]),
        "svnet_t_stride": (c_i64, [c_int]),
    }


def test_spot_pins_of_the_derived_tables():
    S, D = _lib.SIGNATURES, _lib.DEFINES
    assert S["svnet_ball_query_f32"][1][5] is _lib.c_f
    assert S["svnet_last_error"] == (ctypes.c_char_p, [])
    assert S["svnet_knn_workspace_bytes"][0] is ctypes.c_size_t
    assert S["svnet_gemm_f32"][1] == [ctypes.POINTER(_lib.GemmDesc), _lib.c_p]
    for query in ("svnet_gemm_tier", "svnet_gemm_variant"):                          # the dispatch queries take the descriptor alone
        assert S[query] == (_lib.c_int, [ctypes.POINTER(_lib.GemmDesc)])
    assert [D["SVNET_GEMM_" + n] for n in ("TN_TERN", "TN_FP32", "ROWS", "ROWS_LDS", "ROWS_SPLIT", "DOT", "TILE")] == [1, 2, 3, 4, 5, 6, 7]
    assert D["SVNET_ABI_VERSION"] >= 436
    assert dict(_lib.BlockTailDesc._fields_)["gate"] is _lib.GateFwdJob and isinstance(_lib.BlockTailDesc().gate, _lib.GateFwdJob)
    assert dict(_lib.BinHeadDesc._fields_)["nbt"] is _lib.c_p                        # `long long* nbt` is a pointer
    assert D["SVNET_E_UNSUPPORTED"] == -2
    assert "SVNET_HIP_H" not in D and "SVNET_SLICED_LEN" not in D
    assert D["SVNET_ABI_VERSION"] == _lib.ABI_VERSION == _lib.lib().svnet_version()
