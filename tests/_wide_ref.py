"""Wide-stride operands: a tiny logical [N, d] matrix laid out as a view into one large device allocation, so that its rows lie more
than 2^31 elements and more than 2^32 bytes from the view's base while only N·d values are ever touched.  A kernel whose address
arithmetic drops bits (an int row index times a leading dimension, a 32-bit byte offset, a buffer descriptor's range) then reads or
writes the wrong place — and the layout guarantees that the wrong place is still inside the allocation: a regression shows as a wrong
number, never as a memory fault.

The layout arithmetic (plain integers, no torch) is checked by tests/test_wide_offsets_host.py; the arena needs a GPU."""

ITEM = 4                                   # bytes per element (fp32 / int32)
ALLOC_ELEMS = 6 * (1 << 30) + (1 << 24)    # 24 GiB + 64 MiB
MAX_ROWS = 33
MAX_ROWS_F64 = 32                          # 8-byte elements in the "aligned" layout: the same BYTE positions as rows 0..31 of the fp32 view
                                           # (element offsets stay below 2^31: a signed 32-bit element index of row 32 would leave the
                                           # allocation, which the layout must never allow; byte offsets still pass 2^32 from row 8 on)
MAX_WIDTH = 1024
GUARD = 256                                # sentinel floats checked before and after every written row
SENTINEL = -777.25

# name -> (first element of the view inside the allocation, leading dimension in elements)
LAYOUTS = {
    "aligned": ((1 << 31), (1 << 27) + 256),           # base and rows 16-byte aligned
    "odd": ((1 << 31) + 1, (1 << 27) + 257),           # base 4-byte but not 16-byte aligned, odd ld: rows of every alignment class
}


def row_offsets(layout, rows=MAX_ROWS):
    base, ld = LAYOUTS[layout]
    return [r * ld for r in range(rows)]


def _wrap(v, bits=32, signed=False):
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def truncated_byte_positions(elem_offset):
    """Where, in bytes from the view's base, an access to `elem_offset` lands when the element offset or the byte offset is cut to 32
    bits, signed or unsigned (the true position included)."""
    out = [elem_offset * ITEM]
    for signed in (False, True):
        out.append(_wrap(elem_offset, signed=signed) * ITEM)
        out.append(_wrap(elem_offset * ITEM, signed=signed))
    return out


def layout_problems(layout, rows=MAX_ROWS, width=MAX_WIDTH, alloc_elems=ALLOC_ELEMS):
    """The conditions of the layout alone, whatever a kernel does; returns a list of violations (empty = fine)."""
    base, ld = LAYOUTS[layout]
    bad = []
    offs = row_offsets(layout, rows)
    if not any((1 << 31) <= o < (1 << 32) for o in offs):
        bad.append("no row at an element offset in [2^31, 2^32)")
    if not any(o >= (1 << 32) and o * ITEM >= (1 << 34) for o in offs):
        bad.append("no row at an element offset >= 2^32 (>= 2^34 bytes)")
    lo, hi = GUARD * ITEM, alloc_elems * ITEM - (width + GUARD) * ITEM
    spans = []
    for r, o in enumerate(offs):
        for col in (0, width - 1):
            for k, pos in enumerate(truncated_byte_positions(o + col)):
                where = base * ITEM + pos
                if not lo <= where - col * ITEM <= hi:
                    bad.append("row %d col %d truncation %d lands at byte %d, outside the allocation" % (r, col, k, where))
        for k, pos in enumerate(truncated_byte_positions(o)):
            spans.append((base * ITEM + pos, r, k))
    # a truncated access must not land on another row's data or guard band either: it has to read or write something else
    true_rows = [(base * ITEM + o * ITEM, r) for r, o in enumerate(offs)]
    for where, r, k in spans:
        for start, r2 in true_rows:
            if r2 != r and abs(where - start) < (width + 2 * GUARD) * ITEM:
                bad.append("row %d truncation %d lands on row %d" % (r, k, r2))
            if r2 == r and k and where != start and abs(where - start) < (width + 2 * GUARD) * ITEM:
                bad.append("row %d truncation %d overlaps its own row" % (r, k))
    if layout == "aligned" and (base % 4 or ld % 4):
        bad.append("aligned layout is not 16-byte aligned")
    if layout == "odd" and (base % 4 == 0 or ld % 2 == 0):
        bad.append("odd layout must have an odd ld and a base that is not 16-byte aligned")
    return bad


class WideArena(object):
    """One allocation per test module; every operand view is carved out of it."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.buf = torch.empty(ALLOC_ELEMS, dtype=torch.float32, device=device)        # never touched as a whole

    def release(self):
        self.buf = None
        self.torch.cuda.empty_cache()

    def _rows(self, layout, n):
        base, ld = LAYOUTS[layout]
        assert n <= MAX_ROWS
        return [base + r * ld for r in range(n)]

    def _per(self, dtype):
        """fp32 slots per element: 1, or 2 for float64 (aligned layout, at most 32 rows)"""
        return 2 if dtype == self.torch.float64 else 1

    def view(self, layout, n, d, dtype=None):
        """[n, d] view with the layout's row stride (pass its data_ptr / stride(0) to a kernel; do not run torch ops on it)"""
        base, ld = LAYOUTS[layout]
        per = self._per(dtype)
        assert n <= (MAX_ROWS if per == 1 else MAX_ROWS_F64) and d * per <= MAX_WIDTH and (per == 1 or layout == "aligned")
        buf = self.buf if dtype is None else self.buf.view(dtype)
        return self.torch.as_strided(buf, (n, d), (ld // per, 1), base // per)

    def base(self, layout):
        """1-element-offset tensor whose data_ptr is the view's base (for kernels that take a base pointer and offsets)"""
        return self.buf[LAYOUTS[layout][0]:]

    def put(self, layout, small, guard=False):
        """copy the small [n, d] tensor into the rows of the layout and return the wide view"""
        n, d = small.shape
        src = small.contiguous().view(self.torch.float32) if small.dtype != self.torch.float32 else small
        w = src.shape[1]
        for r, s in enumerate(self._rows(layout, n)):
            if guard:
                self.buf[s - GUARD: s + w + GUARD].fill_(SENTINEL)
            self.buf[s: s + w].copy_(src[r])
        return self.view(layout, n, d, None if small.dtype == self.torch.float32 else small.dtype)

    def out(self, layout, n, d, dtype=None, fill=None):
        """an output view: rows and guard bands prefilled with the sentinel (or rows with `fill`, a small [n, d] tensor)"""
        w = d * self._per(dtype)
        for r, s in enumerate(self._rows(layout, n)):
            self.buf[s - GUARD: s + w + GUARD].fill_(SENTINEL)
            if fill is not None:
                self.buf[s: s + w].copy_(fill[r])
        return self.view(layout, n, d, dtype)

    def read(self, layout, n, d, dtype=None):
        """the rows as a dense [n, d] tensor"""
        w = d * self._per(dtype)
        rows = self.torch.stack([self.buf[s: s + w] for s in self._rows(layout, n)])
        return rows if dtype is None else rows.view(dtype)

    def guards_intact(self, layout, n, d, dtype=None):
        d = d * self._per(dtype)
        g = self.torch.stack([self.torch.cat([self.buf[s - GUARD: s], self.buf[s + d: s + d + GUARD]]) for s in self._rows(layout, n)])
        return bool((g == SENTINEL).all())


def dense_twin(small, layout):
    """The small tensor as a dense device tensor of the same alignment class as the layout: contiguous for "aligned"; ld = d + 1 (odd or
    even as the layout's) behind a 4-byte offset for "odd" — so that the dense and the wide call take the same kernel."""
    import torch
    if layout == "aligned":
        return small.contiguous()
    n, d = small.shape
    ld = d + 1 if d % 2 == 0 else d + 2
    store = torch.zeros(n * ld + 1, dtype=small.dtype, device=small.device)
    v = torch.as_strided(store, (n, d), (ld, 1), 1)
    v.copy_(small)
    return v
