"""dalle_hip.abi reads include/dalle_hip.h as data (signatures, struct fields, constants) and the bindings take all three from
it.  Here: the reader on small literal declarations, the whole header against an independent scan of its names and against what
dh.lib() ends up bound with, and the two structs against the host compiler's own sizeof / offsetof."""
import ctypes
import os
import shutil
import subprocess
from ctypes import c_char_p, c_int, c_int64, c_uint32, c_void_p

import pytest

import dalle_hip as dh
from dalle_hip import abi
from test_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declaration_over_three_lines_with_a_comment_in_the_parameter_list():
    h = abi.parse("""int dmi_embed(const int32_t* tokens, uint16_t* x,   // the output
                                   int64_t rows /*B*S*/, int S,
                                   float eps, void* stream);""")
    assert h.functions == {"dmi_embed": (c_int, [c_void_p, c_void_p, c_int64, c_int, ctypes.c_float, c_void_p],
                                         ["tokens", "x", "rows", "S", "eps", "stream"])}


def test_pointer_forms_void_list_and_return_types():
    h = abi.parse("""
        /* dmi_in_a_comment(is not a declaration) */
        int dmi_finish(const void* const* p, float* const* dgs, void** out, const int64_t* rows, const char* name, size_t n, double g);
        const char* dmi_last_error_string(void);
        uint32_t dmi_crc(const void* data, size_t n);
        int64_t dmi_bytes( void );
        uint64_t dmi_key(uint64_t seed, uint32_t lane, int32_t v);""")
    assert h.functions["dmi_finish"][:2] == (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_char_p, ctypes.c_size_t, ctypes.c_double])
    assert h.functions["dmi_finish"][2] == ["p", "dgs", "out", "rows", "name", "n", "g"]
    assert h.functions["dmi_last_error_string"] == (c_char_p, [], [])
    assert h.functions["dmi_crc"] == (c_uint32, [c_void_p, ctypes.c_size_t], ["data", "n"])
    assert h.functions["dmi_bytes"] == (c_int64, [], [])
    assert h.functions["dmi_key"] == (ctypes.c_uint64, [ctypes.c_uint64, c_uint32, ctypes.c_int32], ["seed", "lane", "v"])
    assert sorted(h.functions) == ["dmi_bytes", "dmi_crc", "dmi_finish", "dmi_key", "dmi_last_error_string"]


def test_structs_defines_and_status_enumerators():
    h = abi.parse("""
        #define DMI_GEMM_BIAS 1
        #define DMI_GEMM_GELU 512   /* a flag */
        #define DMI_HEX 0x20
        #define NOT_OURS 3
        typedef enum { DMI_OK = 0, DMI_ERR_INVALID = -1,   /* bad size */
                       DMI_ERR_LAUNCH = -2 } dmi_status;
        typedef struct dmi_item { const float* slabs; float* out; int nsplit; int64_t n4;
                                  void* workspace; } dmi_item;
        int dmi_reduce(const dmi_item* items, int n, void* stream);""")
    assert h.structs == {"dmi_item": [("slabs", c_void_p), ("out", c_void_p), ("nsplit", c_int), ("n4", c_int64), ("workspace", c_void_p)]}
    assert h.constants == {"DMI_GEMM_BIAS": 1, "DMI_GEMM_GELU": 512, "DMI_HEX": 32, "DMI_OK": 0, "DMI_ERR_INVALID": -1, "DMI_ERR_LAUNCH": -2}
    assert h.functions["dmi_reduce"][1] == [c_void_p, c_int, c_void_p]


def test_unknown_type_raises_and_names_function_and_parameter():
    with pytest.raises(abi.HeaderError, match=r"dmi_step, rows.*long"):
        abi.parse("int dmi_ok(int a);\nint dmi_step(float* p, long rows);")
    with pytest.raises(abi.HeaderError, match=r"dmi_step, item.*dmi_item"):
        abi.parse("int dmi_step(dmi_item item);")          # a struct by value is not something ctypes is told here
    with pytest.raises(abi.HeaderError, match=r"dmi_step, return value.*void"):
        abi.parse("void dmi_step(int a);")
    with pytest.raises(abi.HeaderError, match="dmi_step"):
        abi.parse("int dmi_step(int);")                    # a parameter without a name


def test_a_declaration_the_reader_cannot_consume_raises():
    with pytest.raises(abi.HeaderError, match=r"dmi_foo"):
        abi.parse("int dmi_ok(int a);\nint dmi_foo(int (*callback)(int), void* stream);")
    with pytest.raises(abi.HeaderError, match=r"dmi_foo"):
        abi.parse("static inline int dmi_foo(int a) { return a; }")
    with pytest.raises(abi.HeaderError, match=r"dmi_foo"):
        abi.parse("int dmi_foo(int a)")                    # no terminating semicolon


def test_whole_header_names_and_bindings():
    h = abi.header()
    assert abi.header() is h                              # read once per process
    names = _declared()
    assert sorted(h.functions) == names == dh.declared_symbols() and len(names) >= 131
    L = dh.lib()
    for name in names:
        res, args, params = h.functions[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args and len(params) == len(args), name
    zero = sorted(n for n in names if not h.functions[n][1])
    assert zero == ["dmi_comm_unique_id_bytes", "dmi_last_error_string", "dmi_mse_workspace_bytes", "dmi_version",
                    "dmi_vq_loss_workspace_bytes"]
    assert all(list(getattr(L, n).argtypes) == [] for n in zero)
    assert L.dmi_crc32c.argtypes[0] is c_void_p and L.dmi_crc32c.restype is c_uint32      # the header's const void*
    for data in (b"123456789", (ctypes.c_char * 9).from_buffer(bytearray(b"123456789"))):     # what c_void_p accepts
        assert L.dmi_crc32c(data, 9) == 0xE3069283          # the CRC-32C check value


def test_constants_and_struct_classes_come_from_the_header():
    c = abi.header().constants
    flags = {n: c["DMI_GEMM_" + n] for n in ("BIAS", "RELU", "RESIDUAL", "RELU_MASK", "OUT_F32", "ROWSCALE", "GELU")}
    assert flags == dict(BIAS=1, RELU=2, RESIDUAL=4, RELU_MASK=8, OUT_F32=16, ROWSCALE=32, GELU=512)
    assert all(getattr(dh, "GEMM_" + n) == v for n, v in flags.items())
    assert dh.AF_FIELDS == c["DMI_AF_FIELDS"] == 17
    assert (c["DMI_OK"], c["DMI_ERR_INVALID"], c["DMI_ERR_LAUNCH"], c["DMI_ERR_UNSUPPORTED"]) == (0, -1, -2, -3)
    s = abi.header().structs
    assert sorted(s) == ["dmi_reduce_item", "dmi_tn_problem"]
    assert dh.ReduceItem._fields_ == s["dmi_reduce_item"] and dh.TnProblem._fields_ == s["dmi_tn_problem"]


def test_struct_layout_matches_the_host_compiler(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "abi_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "abi_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "abi_layout_check: ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    compiled = dict(line.rsplit(" ", 1) for line in r.stdout.splitlines() if not line.startswith("abi_layout_check"))
    ours = {}
    for name, cls in (("dmi_reduce_item", dh.ReduceItem), ("dmi_tn_problem", dh.TnProblem)):
        ours[name + " sizeof"] = str(ctypes.sizeof(cls))
        ours.update({f"{name}.{field}": str(getattr(cls, field).offset) for field, _ in cls._fields_})
    assert compiled == ours                               # every field of the header's structs, and no other
    assert ours["dmi_reduce_item sizeof"] == "32" and ours["dmi_tn_problem sizeof"] == "72"
