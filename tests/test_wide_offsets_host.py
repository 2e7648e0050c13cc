"""Host side of the wide-offset coverage (no GPU needed): the table of tests/test_gpu_wide_offsets.py lists every entry point of
include/ctgcn_hip.h that takes a leading dimension or row stride, and names nothing the header does not have; the wide layouts of
tests/_wide_ref.py keep every 32-bit truncation of a row's offset inside the allocation; ctgcn_gru_weight_grad_f32 refuses strides its
buffer descriptors cannot address, at exactly the bound its kernel's arithmetic gives."""
import ctypes
import os
import re

import pytest

import _wide_ref as W
import test_gpu_wide_offsets as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE_NAME = re.compile(r"^(ld\w*|\w*stride\w*)$")


def header_functions(text=None):
    """name -> (all parameter names, the int64_t parameters whose name says leading dimension or stride)"""
    if text is None:
        with open(os.path.join(ROOT, "include", "ctgcn_hip.h")) as fh:
            text = fh.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|int32_t|int64_t|uint64_t)\s+(ctgcn_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        params = [p.strip() for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        names = [re.split(r"[\s\*]+", p)[-1] for p in params]
        strides = [n for p, n in zip(params, names) if re.match(r"^(const\s+)?int64_t\s+\w+$", p) and STRIDE_NAME.match(n)]
        out[m.group(1)] = (names, strides)
    return out


def table_problems(table, funcs):
    bad = []
    for name, (_, strides) in funcs.items():
        if strides and name not in table:
            bad.append("%s takes %s and is not in the table" % (name, ", ".join(strides)))
    for name, row in table.items():
        if name not in funcs:
            bad.append("the table names %s, which the header does not declare" % name)
            continue
        names, strides = funcs[name]
        listed = set(row["wide"]) | set(row["dense"])
        for p in listed:
            if p not in names:
                bad.append("%s: the table names operand %s, which the header does not have" % (name, p))
        for p in strides:
            if p not in listed:
                bad.append("%s: stride parameter %s is neither driven wide nor given a reason" % (name, p))
        for p, why in row["dense"].items():
            if not (isinstance(why, str) and why.strip()):
                bad.append("%s: %s is kept dense without a reason" % (name, p))
        if row["deferred"] is not None and not (isinstance(row["deferred"], str) and row["deferred"].strip()):
            bad.append("%s: deferred without a reason" % name)
        if row["deferred"] is None and name not in T.DRIVERS:
            bad.append("%s: not deferred, and no driver" % name)
        for p, layouts in row["wide"].items():
            if not layouts or any(l not in W.LAYOUTS for l in layouts):
                bad.append("%s: %s has no or unknown layouts %r" % (name, p, layouts))
    return bad


def test_the_header_parser_sees_the_strided_entry_points():
    funcs = header_functions()
    assert funcs["ctgcn_gru_weight_grad_f32"][1] == ["ldg01", "ldg2", "ldx"]
    assert funcs["ctgcn_gru_layer_f32"][1] == ["ldx", "ld_out", "ld_row"] and "step_offsets" in funcs["ctgcn_gru_layer_f32"][0]
    assert funcs["ctgcn_rowsel_conv_fwd_f32"][1] == ["lds", "col_stride", "ldy"]
    assert funcs["ctgcn_kcore_i32"][1] == [] and funcs["ctgcn_abi_version"] == ([], [])
    assert sum(1 for _, s in funcs.values() if s) >= 81
    # a kernel added later: found by the same rules
    extra = header_functions("int ctgcn_new_op_f32(int64_t n, const float *a, int64_t lda, float *b, int64_t row_stride_b, void *stream);")
    assert extra == {"ctgcn_new_op_f32": (["n", "a", "lda", "b", "row_stride_b", "stream"], ["lda", "row_stride_b"])}


def test_the_table_lists_every_strided_entry_point_and_nothing_else():
    bad = table_problems(T.TABLE, header_functions())
    assert not bad, "\n".join(bad)


def test_the_completeness_check_notices_a_missing_row_a_missing_operand_and_a_stranger():
    funcs = header_functions()
    short = {k: v for k, v in T.TABLE.items() if k != "ctgcn_spmm_csr_f32"}
    assert any("ctgcn_spmm_csr_f32 takes ldx, ldy" in b for b in table_problems(short, funcs))
    row = dict(T.TABLE["ctgcn_spmm_csr_f32"], wide={"ldx": T.BOTH})
    assert any("stride parameter ldy" in b for b in table_problems(dict(T.TABLE, ctgcn_spmm_csr_f32=row), funcs))
    row = dict(T.TABLE["ctgcn_spmm_csr_f32"], wide={"ldx": T.BOTH, "ldy": T.BOTH, "ldz": T.BOTH})
    assert any("operand ldz" in b for b in table_problems(dict(T.TABLE, ctgcn_spmm_csr_f32=row), funcs))
    assert any("ctgcn_nothing_f32" in b for b in table_problems(dict(T.TABLE, ctgcn_nothing_f32=T.TABLE["ctgcn_spmm_csr_f32"]), funcs))
    funcs2 = dict(funcs, ctgcn_new_op_f32=(["n", "a", "lda"], ["lda"]))
    assert any("ctgcn_new_op_f32 takes lda" in b for b in table_problems(T.TABLE, funcs2))


def test_every_case_of_the_gpu_module_comes_from_the_table():
    cases = T.cases()
    assert len(cases) == len(set(cases)) > 0
    for fn, param, layout in cases:
        assert T.TABLE[fn]["deferred"] is None and layout in T.TABLE[fn]["wide"][param]
    driven = {fn for fn, _, _ in cases}
    assert driven == {fn for fn, row in T.TABLE.items() if row["deferred"] is None} == set(T.DRIVERS)


@pytest.mark.parametrize("layout", sorted(W.LAYOUTS))
def test_every_truncated_offset_of_a_wide_layout_stays_inside_the_allocation(layout):
    """plain integers: for every row, its element offset and its byte offset cut to 32 bits, signed or unsigned, land inside the
    allocation and on no other row; rows exist in [2^31, 2^32) elements and at >= 2^32 elements (>= 2^34 bytes)"""
    assert W.layout_problems(layout) == []
    base, ld = W.LAYOUTS[layout]
    alloc = W.ALLOC_ELEMS * W.ITEM
    assert alloc < 32 * (1 << 30)
    seen = set()
    for r in range(W.MAX_ROWS):
        e = r * ld
        for cut in (e, e & 0xFFFFFFFF, ((e + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31):
            seen.add(cut != e)
            assert 0 <= base * 4 + cut * 4 and base * 4 + cut * 4 + (W.MAX_WIDTH + W.GUARD) * 4 <= alloc, (r, cut)
        b = e * 4
        for cut in (b & 0xFFFFFFFF, ((b + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31):
            assert 0 <= base * 4 + cut and base * 4 + cut + (W.MAX_WIDTH + W.GUARD) * 4 <= alloc, (r, cut)
    assert seen == {False, True}                             # some rows really are beyond 32 bits
    if layout == "odd":
        assert ld % 2 == 1 and (base * 4) % 16 == 4
        assert {(base + r * ld) % 4 for r in range(W.MAX_ROWS)} == {0, 1, 2, 3}      # rows of every alignment class


def test_the_layout_check_notices_a_layout_that_could_fault(monkeypatch):
    monkeypatch.setitem(W.LAYOUTS, "aligned", (1 << 20, (1 << 27) + 256))            # base too low: a signed truncation lands before the buffer
    assert any("outside the allocation" in b for b in W.layout_problems("aligned"))
    monkeypatch.setitem(W.LAYOUTS, "aligned", (1 << 31, 1 << 27))                    # ld = 2^27 exactly: row 32 folds back onto row 0
    assert any("lands on row" in b for b in W.layout_problems("aligned"))
    monkeypatch.setitem(W.LAYOUTS, "aligned", (1 << 31, 1 << 20))                    # nothing beyond 2^31
    assert any("no row at an element offset" in b for b in W.layout_problems("aligned"))


# ------------------------------------------------------------------------------- the weight gradient's descriptor bound
def _weight_grad(lib, rows=64, ldg01=256, ldg2=128, ldx=128, shift=0, n_pairs=8):
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused before any launch
    rc = lib.ctgcn_gru_weight_grad_f32(rows, 4, 128, p, ldg01, p, ldg2, p, ldx, shift, p, n_pairs, 0, None)
    return rc, lib.ctgcn_last_error().decode()


@pytest.mark.parametrize("rows,n_pairs,shift", [(64, 8, 0), (64, 8, 1), (32, 8, 1), (65, 8, 0), (33, 8, 1), (1000, 8, 0), (1000, 8, 1), (1000, 16, 1), (20000, 128, 1)])
def test_weight_gradient_refuses_a_stride_just_above_its_descriptor_bound(rows, n_pairs, shift):
    """CTGCN_E_UNSUPPORTED one element above the largest leading dimension the kernel can address (the bound re-derived in
    test_gpu_wide_offsets.dw_max_ld), for each operand, with the operand and the bound in the message; the GPU test
    test_weight_gradient_just_below_the_descriptor_bound pins the other side."""
    from ctgcn_amd import _lib
    lib = _lib.load()
    UNSUPPORTED = -4
    for operand, key in (("g01", "ldg01"), ("g2", "ldg2"), ("x", "ldx")):
        bound = T.dw_max_ld(rows, n_pairs, shift and operand == "x")
        rc, msg = _weight_grad(lib, rows=rows, shift=shift, n_pairs=n_pairs, **{key: bound + 1})
        assert rc == UNSUPPORTED, (operand, rc, msg)
        assert "gru_weight_grad: %s with ld=%d" % (operand, bound + 1) in msg and "is %d," % bound in msg and "n_pairs" in msg, msg
        rc, msg = _weight_grad(lib, rows=rows, shift=shift, n_pairs=n_pairs, **{key: 1 << 27})
        assert rc == UNSUPPORTED and ("%s with ld=%d" % (operand, 1 << 27)) in msg


def test_weight_gradient_bound_follows_the_kernels_arithmetic():
    # 64 rows on 8 pairs: two blocks of one 32-row chunk; row 31 must end (32-column tail) inside the 0x7fffffff-byte descriptor
    assert T.dw_max_ld(64, 8, False) == (0x7fffffff - 128) // 4 // 31 == 17318415
    assert T.dw_max_ld(64, 8, True) == 17318415              # the second block starts one row back and still reads 32 rows
    assert T.dw_max_ld(32, 8, True) == (0x7fffffff - 128) // 4 // 30          # one block from row 0: x[r - 1] for r = 1..31
    assert T.dw_max_ld(1000, 8, False) == (0x7fffffff - 128) // 4 // 127      # ceil(32 chunks / 8) = 4 chunks per block
    assert T.dw_max_ld(33, 8, False) == (0x7fffffff - 128) // 4 // 31         # the ragged last block's 31 padding rows: below 2^32
    assert T.dw_max_ld(1, 8, False) == (2 ** 32 - 128) // 4 // 31             # one data row at offset 0; rows 1..31 must not wrap
    # more pairs, shorter spans: the message's other way out
    assert T.dw_max_ld(20000, 128, False) > T.dw_max_ld(20000, 8, False)
