"""ctypes binding of libctgcn_hip.so (C ABI: include/ctgcn_hip.h).

There is NO fallback: if the shared library is missing or a call fails, an exception is raised.
Build it with `python -m ctgcn_amd.build` (hipcc --offload-arch=gfx950) or __graft_entry__.build().
"""
import ctypes
import os

from . import _cdecl

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTGCN_HIP_LIB") or os.path.join(_HERE, "csrc", "libctgcn_hip.so")   # env override: kernel A/B builds

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ctgcn_hip.h")


class CtgcnHipError(RuntimeError):
    pass


# The header is the binding: an entry point is declared there, defined in a .hip file and called from Python.  Its prototypes, descriptor
# structs and constants are read here, once, at import; nothing below repeats a type, a field or a value of it.
try:
    with open(HEADER_PATH) as _f:
        _header = _f.read()
except OSError as e:
    raise CtgcnHipError("C header %s not readable (%s): the ctypes binding is derived from it" % (HEADER_PATH, e)) from None

SIGNATURES, _structs, _const = _cdecl.parse(_header)     # SIGNATURES: name -> (restype, argtypes) of every symbol the header declares

# The top-k link ranking is declared in a header of its own (the entry points of ctgcn_hip.h are a pinned set): same reader, same rules.
TOPK_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ctgcn_topk.h")
try:
    with open(TOPK_HEADER_PATH) as _f:
        _topk = _cdecl.parse(_f.read())
except OSError as e:
    raise CtgcnHipError("C header %s not readable (%s): the ctypes binding is derived from it" % (TOPK_HEADER_PATH, e)) from None
TOPK_SIGNATURES = _topk.functions


def _struct(cname):
    return type(cname, (ctypes.Structure,), {"_fields_": _structs[cname], "__doc__": "%s (include/ctgcn_hip.h)" % cname})


AggSplitGroup = _struct("ctgcn_agg_split_group_t")
GruLayerGroup = _struct("ctgcn_gru_layer_group_t")
GruSeqGroup = _struct("ctgcn_gru_seq_group_t")

(ABI_VERSION, F_SELF_LOOP, F_RELU, F_NESTED, ACT_NONE, ACT_SELU, CLS_NODE, CLS_HADAMARD, CLS_DOT, OP_KCORE, OP_INGEST, MAX_SLOTS) = (
    _const["CTGCN_" + k] for k in ("ABI_VERSION", "F_SELF_LOOP", "F_RELU", "F_NESTED", "ACT_NONE", "ACT_SELU", "CLS_NODE", "CLS_HADAMARD",
                                   "CLS_DOT", "OP_KCORE", "OP_INGEST", "MAX_SLOTS"))

TOPK_NO_SELF, TOPK_UPPER = _topk.constants["CTGCN_TOPK_NO_SELF"], _topk.constants["CTGCN_TOPK_UPPER"]      # flags of ctgcn_topk_scores_f32

_lib = None


def load():
    """Load the library (once). Raises CtgcnHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CtgcnHipError(
            "libctgcn_hip.so not found at %s — the HIP extension is required (no CPU fallback). "
            "Build it with `python -m ctgcn_amd.build`." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(TOPK_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.ctgcn_abi_version() != ABI_VERSION:
        raise CtgcnHipError("libctgcn_hip.so ABI %d != binding ABI %d; rebuild" % (lib.ctgcn_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().ctgcn_last_error()
        raise CtgcnHipError("%s failed (code %d): %s" % (what, rc, msg.decode("utf-8", "replace") if msg else ""))


def ptr(t):
    """Device (or host) address of a torch tensor, None -> NULL."""
    return None if t is None else t.data_ptr()
