"""CPU-only checks of the ctypes binding derived from include/ctgcn_hip.h: every rule of ctgcn_amd/_cdecl.py on snippets (its loud
failures included), then the real header against anchors written out by hand."""
import ctypes
import importlib.util
import os
import shutil
from ctypes import POINTER, c_char, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from conftest import ROOT
from test_host_logic import _declared_symbols

from ctgcn_amd import _cdecl, _lib

HEADER = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()


def _one(decl):
    (sig,) = _cdecl.functions(decl).values()
    return sig


# ------------------------------------------------------------------------------------ functions, on snippets
@pytest.mark.parametrize("ctype, expected", [
    ("int64_t", c_int64), ("int32_t", c_int32), ("uint32_t", c_uint32), ("uint64_t", c_uint64), ("int", c_int), ("size_t", c_size_t),
    ("float", c_float), ("double", c_double), ("char", c_char)])
def test_scalar_parameters_and_returns(ctype, expected):
    assert _one("%s ctgcn_f(%s a, const %s b);" % (ctype, ctype, ctype)) == (expected, [expected, expected])


def test_char_pointers_are_strings_as_parameter_and_as_return():
    assert _one("const char *ctgcn_f(const char *path_host, char *name_host, const char *plain);") == (c_char_p, [c_char_p] * 3)
    assert _one("char *ctgcn_f(void);") == (c_char_p, [])


def test_host_suffix_makes_a_typed_pointer_only_for_nonconst_single_scalar_pointers():
    assert _one("int ctgcn_f(int64_t *nnz_host, int *cu_host, int32_t *m_host, double *t_host);")[1] == [
        POINTER(c_int64), POINTER(c_int), POINTER(c_int32), POINTER(c_double)]
    assert _one("int ctgcn_f(const int32_t *a_host);")[1] == [c_void_p]          # const: an input array, passed by address
    assert _one("int ctgcn_f(int32_t **a_host);")[1] == [c_void_p]               # double pointer
    assert _one("int ctgcn_f(int32_t *a);")[1] == [c_void_p]                     # no suffix: a device pointer
    assert _one("int ctgcn_f(int32_t *a_hosts, int32_t *host);")[1] == [c_void_p, c_void_p]
    assert _one("int ctgcn_f(void *a_host, uint8_t *b_host);")[1] == [c_void_p, c_void_p]   # not pointers to a bound scalar


def test_every_other_pointer_is_an_address():
    src = """typedef struct { int32_t k; } ctgcn_g_t;
             int ctgcn_f(void *a, const void *b, const float *c, float *d, const float *const *e, float *const *f, const uint8_t *g,
                         uint8_t *h, const ctgcn_g_t *i, const int64_t *j, const uint32_t *k, const void *const *l, double *m);"""
    assert _one(src) == (c_int, [c_void_p] * 13)
    assert _one("int32_t *ctgcn_f(void);") == (c_void_p, [])


def test_void_parameter_list_a_char_scalar_and_a_void_return():
    assert _one("int ctgcn_f(void);") == (c_int, [])
    assert _one("size_t ctgcn_f( void );") == (c_size_t, [])
    assert _one("int ctgcn_f(const char *path, char sep, int32_t digits);") == (c_int, [c_char_p, c_char, c_int32])
    assert _one("void ctgcn_f(int a);") == (None, [c_int])


def test_multi_line_declarations_comments_and_the_cplusplus_bracket():
    src = """
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        /* int ctgcn_ghost(int a);  a declaration inside a comment is no declaration */
        int ctgcn_f(int64_t n,   /* rows */
                    const float *x,
                    /* ctgcn_other(1, 2) is mentioned here; */ int64_t ldx,   // elements
                    float
                        ln_eps, void *stream);
        size_t
        ctgcn_g(int32_t groups);
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */
    """
    assert _cdecl.functions(src) == {"ctgcn_f": (c_int, [c_int64, c_void_p, c_int64, c_float, c_void_p]), "ctgcn_g": (c_size_t, [c_int32])}
    assert _cdecl.constants(src) == {} and _cdecl.structs(src) == {}


# ------------------------------------------------------------------------------------ structs and constants, on snippets
def test_struct_with_shared_base_types_has_the_c_layout():
    src = """typedef struct {
                 const int32_t *row_ptr, *col_idx;   /* 0, 8 */
                 float eps;                          /* 16 */
                 int32_t steps;                      /* 20 */
                 char tag;                           /* 24, then 7 bytes of padding */
                 int64_t ld, work;                   /* 32, 40 */
                 uint32_t flags;                     /* 48, then 4 bytes of padding */
                 void *ws, *const *tables;           /* 56, 64 */
                 char *name_host;                    /* 72: pointers in a struct are addresses, whatever their name */
                 size_t bytes;                       /* 80 */
                 double tol;                         /* 88 */
                 float tail;                         /* 96, then 4 bytes to the struct's alignment of 8 */
             } ctgcn_demo_t;
             typedef struct { float a, b; const ctgcn_demo_t *next; } ctgcn_two_t;"""
    parsed = _cdecl.structs(src)
    assert list(parsed) == ["ctgcn_demo_t", "ctgcn_two_t"]
    assert parsed["ctgcn_demo_t"] == [
        ("row_ptr", c_void_p), ("col_idx", c_void_p), ("eps", c_float), ("steps", c_int32), ("tag", c_char), ("ld", c_int64), ("work", c_int64),
        ("flags", c_uint32), ("ws", c_void_p), ("tables", c_void_p), ("name_host", c_void_p), ("bytes", c_size_t), ("tol", c_double),
        ("tail", c_float)]
    demo = type("Demo", (ctypes.Structure,), {"_fields_": parsed["ctgcn_demo_t"]})
    assert ctypes.sizeof(demo) == 104
    assert [getattr(demo, f).offset for f, _ in demo._fields_] == [0, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96]
    assert parsed["ctgcn_two_t"] == [("a", c_float), ("b", c_float), ("next", c_void_p)]
    assert _cdecl.functions(src) == {}


def test_constants_from_defines_and_enumerators():
    src = """#ifndef G
             #define G
             #define CTGCN_ABI_VERSION 31
             #define CTGCN_MASK 0x1F   /* hex */
             enum {
                 CTGCN_OK = 0,
                 CTGCN_E_INVALID = -1,   /* bad argument, e.g. (K = 0) */
                 CTGCN_E_HIP = -2
             };
             enum { /* flags */ CTGCN_F_A = 1, CTGCN_F_B = 4, };
             #endif"""
    assert _cdecl.constants(src) == {"CTGCN_ABI_VERSION": 31, "CTGCN_MASK": 31, "CTGCN_OK": 0, "CTGCN_E_INVALID": -1, "CTGCN_E_HIP": -2,
                                     "CTGCN_F_A": 1, "CTGCN_F_B": 4}
    assert _cdecl.functions(src) == {} and _cdecl.structs(src) == {}


# ------------------------------------------------------------------------------------ loud failures
@pytest.mark.parametrize("reader, src, quoted", [
    (_cdecl.functions, "int ctgcn_ok(int a);\nint ctgcn_f(int64_t n, unsigned flags);", "unsigned flags"),          # unknown base type
    (_cdecl.functions, "int ctgcn_f(long n);", "long n"),
    (_cdecl.functions, "int16_t ctgcn_f(void);", "int16_t"),                                                      # ... as return type
    (_cdecl.functions, "int ctgcn_f(const ctgcn_nowhere_t *g);", "ctgcn_nowhere_t *g"),                           # ... behind a pointer
    (_cdecl.functions, "int ctgcn_f(int64_t n, float w[4]);", "float w[4]"),                                      # array parameter
    (_cdecl.functions, "int ctgcn_f(int64_t n, void (*done)(int), void *stream);", "void (*done)(int)"),          # function pointer
    (_cdecl.functions, "int ctgcn_f(void *a, void b);", "void b"),
    (_cdecl.functions, "int ctgcn_f(uint8_t slot);", "uint8_t slot"),                                             # by value: not in the table
    (_cdecl.functions, "int ctgcn_f();", "ctgcn_f()"),
    # a ctgcn_*( that is no plain prototype
    (_cdecl.functions, "int ctgcn_ok(int a);\nint ctgcn_f(int a) __attribute__((cold));", "ctgcn_f(int a) __attribute__"),
    (_cdecl.functions, "static inline int ctgcn_f(int a) { return a; }", "ctgcn_f(int a)"),
    (_cdecl.functions, "#define CTGCN_CALL(x) \\\n    ctgcn_f(x)\nint ctgcn_ok(int a);", "CTGCN_CALL(x)"),
    (_cdecl.functions, "int ctgcn_f(int a)\nint ctgcn_g(int b);", "ctgcn_f(int a)"),                              # lost semicolon
    (_cdecl.functions, "int ctgcn_f(int a);\nint ctgcn_f(int a, int b);", "ctgcn_f(int a, int b)"),
    (_cdecl.functions, "struct ctgcn_s { int a; };", "struct ctgcn_s"),
    (_cdecl.structs, "typedef struct { int32_t steps; uint32_t fresh : 1; } ctgcn_t;", "uint32_t fresh : 1"),     # bit-field
    (_cdecl.structs, "typedef struct { float w[4]; } ctgcn_t;", "float w[4]"),
    (_cdecl.structs, "typedef struct { int a; void (*cb)(int); } ctgcn_t;", "void (*cb)(int)"),
    (_cdecl.structs, "typedef struct { int a; short b; } ctgcn_t;", "short b"),
    (_cdecl.structs, "typedef struct { int a; uint8_t slot; } ctgcn_t;", "uint8_t slot"),
    (_cdecl.structs, "typedef struct { int a; float; } ctgcn_t;", "float"),
    (_cdecl.constants, "#define CTGCN_A 1\n#define CTGCN_SCALE 1.5f", "CTGCN_SCALE 1.5f"),
    (_cdecl.constants, "#define CTGCN_TWICE(x) (2 * (x))", "CTGCN_TWICE(x)"),
    (_cdecl.constants, "enum { CTGCN_A = 1, CTGCN_B };", "CTGCN_B"),                                              # implicit value
    (_cdecl.constants, "enum { CTGCN_A = 1, CTGCN_B = CTGCN_A + 1 };", "CTGCN_B = CTGCN_A + 1"),
])
def test_unreadable_declarations_raise_and_quote_themselves(reader, src, quoted):
    with pytest.raises(_cdecl.CDeclError) as e:
        reader(src)
    assert quoted in str(e.value)


def test_a_struct_with_nested_braces_is_not_skipped():
    src = "typedef struct { int a; struct { int b; } in; } ctgcn_t;\nint ctgcn_f(const ctgcn_t *g);"
    with pytest.raises(_cdecl.CDeclError):
        _cdecl.functions(src)


def test_missing_header_is_a_loud_import_error(tmp_path):
    pkg = tmp_path / "elsewhere" / "ctgcn_amd"
    pkg.mkdir(parents=True)
    shutil.copy(_lib.__file__, pkg / "_lib.py")
    spec = importlib.util.spec_from_file_location("ctgcn_amd._lib_elsewhere", str(pkg / "_lib.py"))
    with pytest.raises(RuntimeError) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "CtgcnHipError"
    assert os.path.join(str(tmp_path), "elsewhere", "include", "ctgcn_hip.h") in str(e.value)


# ------------------------------------------------------------------------------------ the real header
def test_every_declared_entry_point_is_bound():
    declared = _declared_symbols()
    assert len(_lib.SIGNATURES) == len(declared) == 175
    assert sorted(_lib.SIGNATURES) == declared
    assert _lib.SIGNATURES == _cdecl.functions(HEADER)


_I, _I32, _I64, _SZ, _VP = c_int, c_int32, c_int64, c_size_t, c_void_p

# written by hand from the prototypes, not produced by the parser
ANCHORS = {
    "ctgcn_device_info": (_I, [c_char_p, _SZ, POINTER(c_int)]),
    "ctgcn_kcore_i32": (_I, [_I64, _VP, _VP, _VP, _VP, _SZ, _I32, POINTER(c_int32), _VP]),
    "ctgcn_write_embedding_tsv": (_I, [c_char_p, _I64, _I32, _VP, _I64, c_char_p, _VP, c_char, _I32]),
    "ctgcn_pool_conv_fwd_f32": (_I, [_I64, _I32, _VP, _VP, _VP, _VP, _I64, _VP, _I64, c_float, _VP, _VP, _I64, _I32, c_double, c_uint64,
                                     _VP, _VP, _I64, _VP, _I32, _I32, _VP, _SZ, _VP]),
    "ctgcn_gru_cell_fwd_f32": (_I, [_I64, _I32, _VP, _I64, _VP, _I64, _VP, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _I32, _VP]),
}


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_anchor_signatures(name):
    assert _lib.SIGNATURES[name] == ANCHORS[name]


def test_host_out_parameters_follow_the_header_convention():
    assert _lib.SIGNATURES["ctgcn_cent_eigenvector"][1][6] == POINTER(c_int32)       # stop_step_host
    assert _lib.SIGNATURES["ctgcn_pgnn_anchor_dist"][1][13] == POINTER(c_int32)      # levels_run_host
    assert _lib.SIGNATURES["ctgcn_edges_to_csr"][1][8] == POINTER(c_int64)           # nnz_host
    typed = {n for n, (_, args) in _lib.SIGNATURES.items() if any(issubclass(a, ctypes._Pointer) for a in args)}
    assert typed == {"ctgcn_device_info", "ctgcn_edges_to_csr", "ctgcn_kcore_i32", "ctgcn_cent_eigenvector", "ctgcn_pgnn_anchor_dist"}


def test_descriptor_structs_and_constants():
    assert [ctypes.sizeof(s) for s in (_lib.AggSplitGroup, _lib.GruLayerGroup, _lib.GruSeqGroup)] == [120, 104, 96]
    assert all(issubclass(s, ctypes.Structure) for s in (_lib.AggSplitGroup, _lib.GruLayerGroup, _lib.GruSeqGroup))
    assert [f for f, _ in _lib.AggSplitGroup._fields_] == [
        "row_ptr", "col_idx", "val", "slot", "X", "ldx", "K", "flags", "row_order", "tile_mask", "workspace", "workspace_bytes", "planes1",
        "planes2", "scales", "tile_base"]
    assert (_lib.GruLayerGroup.ln_eps.offset, _lib.GruLayerGroup.steps.offset, _lib.GruLayerGroup.work.offset) == (56, 60, 96)
    assert (_lib.GruSeqGroup.ln_eps.offset, _lib.GruSeqGroup.steps.offset, _lib.GruSeqGroup.tile_base.offset) == (40, 44, 80)
    assert (_lib.ABI_VERSION, _lib.F_SELF_LOOP, _lib.F_RELU, _lib.F_NESTED, _lib.ACT_NONE, _lib.ACT_SELU, _lib.CLS_NODE, _lib.CLS_HADAMARD,
            _lib.CLS_DOT, _lib.OP_KCORE, _lib.OP_INGEST, _lib.MAX_SLOTS) == (31, 1, 2, 4, 0, 1, 0, 1, 2, 1, 2, 255)
    consts = _cdecl.constants(HEADER)
    assert (consts["CTGCN_OK"], consts["CTGCN_E_INVALID"], consts["CTGCN_E_LIMIT"], consts["CTGCN_SPLIT_F16X2"]) == (0, -1, -5, 2)
