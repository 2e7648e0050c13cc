"""The case table of test_gpu_agg_shapes.py: graphs with FORCED row lengths and slot layouts, and the two tiers of inputs (_agg_ref.py).
Importable without a GPU: test_agg_ref_host.py checks the exact tier's 2^24 condition for every case here.

A case's structure is a list of stored entries (row, col, slot, edge); the matrix list follows from it: nested A_j = entries tagged <= j
(what a k-core list is), general A_j = entries tagged j.  Columns are distinct within a row, so the stored row lengths are the forced ones
in either form.  `edge` names the value an entry takes (the two directions of a symmetric list share one)."""
import zlib

import numpy as np
import scipy.sparse as sp

from _gcn_graphs import havel_hakimi
import _agg_ref as R

HUB_SPLIT_ENTRIES = 8192           # the library's constant (ctgcn_hub_split_entries; the GPU file asserts it)
HUB_THREADS = 1024


def plan(d, vec4):
    """(VEC, LPR, passes) of plan_for (ctgcn_hip.hip)"""
    vec = 4 if vec4 else 1
    chunks = -(-d // vec)
    lpr = 8
    while lpr < 64 and lpr < chunks:
        lpr <<= 1
    return vec, lpr, -(-chunks // lpr)


def hub_groups(K, lpr, vec):
    """lane groups of a forward hub block (launch_agg_t): 1024 / LPR, fewer while the [G][K][LPR] partials exceed 144 KiB; 0 = K too large
    for one group, hub rows fall back to the row kernels (launch_agg)"""
    per = K * lpr * vec * 4
    if per > 144 * 1024:
        return 0
    g = HUB_THREADS // lpr
    while g > 1 and per * g > 144 * 1024:
        g -= 1
    return g


def row_lengths(L):
    return [0, 1, 3, 4, 5, L - 1, L, L + 1, L + 4, 2 * L, 2 * L + 5, 3 * L + 2]


def nodes_for(L):
    """67 rows (no multiple of the 4, 8, 16 or 32 rows of a block) unless the longest forced row, 3 L + 2 distinct columns, needs more"""
    return {8: 67, 16: 67, 32: 131, 64: 259}[L]


# ------------------------------------------------------------------------------------------------ slot layouts
def layout_slots(layout, length, K, L, variant):
    i = np.arange(length)
    last = K - 1
    if layout == "slot0":
        return np.zeros(length, np.int64)
    if layout == "last":                                   # K - 1 leading empty slots
        return np.full(length, last, np.int64)
    if layout == "s036":                                   # only the first, the middle and the last slot
        return np.array([0, K // 2, last])[(i * 3) // max(length, 1)]
    if layout == "each":                                   # a new slot at every entry: from the row's start (A) or up to its end (B)
        return np.minimum(i, last) if variant == 0 else np.maximum(0, last - (length - 1 - i))
    if layout == "at4L":                                   # a slot change exactly at entry 4 and at entry L; B: slot 0 stays empty
        s = np.array([0, min(2, last), min(5, last)] if variant == 0 else [min(1, last), min(3, last), last])
        return s[(i >= 4).astype(int) + (i >= L).astype(int)]
    if layout == "trail":                                  # trailing empty slots: nothing above slot 1
        return (i >= length // 2).astype(np.int64) * min(1, last) if variant == 0 else np.full(length, min(1, last), np.int64)
    if layout == "spread":                                 # evenly over all K slots
        return (i * K) // max(length, 1)
    raise KeyError(layout)


LAYOUTS = ("slot0", "last", "s036", "each", "at4L", "trail")
SYM_LAYOUTS = ("slot0", "last", "s036", "spread")


class Structure(object):
    def __init__(self, n, K, rows, cols, slots, edge=None):
        self.n, self.K = n, K
        self.rows, self.cols, self.slots = (np.asarray(a, np.int64) for a in (rows, cols, slots))
        self.edge = np.arange(len(self.rows)) if edge is None else np.asarray(edge, np.int64)

    def transposed(self):
        return Structure(self.n, self.K, self.cols, self.rows, self.slots, self.edge)

    def lengths(self, transposed=False):
        return np.bincount(self.cols if transposed else self.rows, minlength=self.n)

    def matrices(self, values, nested):
        """values: one per edge id.  float32-representable float64 CSR list."""
        v = np.asarray(values, np.float64)[self.edge]
        out = []
        for j in range(self.K):
            keep = (self.slots <= j) if nested else (self.slots == j)
            out.append(sp.csr_matrix((v[keep], (self.rows[keep], self.cols[keep])), shape=(self.n, self.n)))
        return out


_structs = {}


def _cached(key, make):
    if key not in _structs:
        _structs[key] = make()
    return _structs[key]


def forced_rows(L, K, layout, n=None, filler=13):
    """directed: rows 0-11 hold row_lengths(L) under variant A of the layout, rows 12-23 the same under variant B, the rest 0..filler entries"""
    n = nodes_for(L) if n is None else n

    def make():
        rng = np.random.default_rng(zlib.crc32(("forced %d %d %s %d" % (L, K, layout, n)).encode()))
        want = row_lengths(L)
        rows, cols, slots = [], [], []
        for r in range(n):
            length = want[r % 12] if r < 24 else int(rng.integers(0, filler + 1))
            c = np.sort(rng.choice(np.delete(np.arange(n), r), length, replace=False))
            rows.append(np.full(length, r))
            cols.append(c)
            slots.append(layout_slots(layout if r < 24 or layout in ("slot0", "last") else "spread", length, K, L, (r // 12) % 2))
        return Structure(n, K, np.concatenate(rows), np.concatenate(cols), np.concatenate(slots))
    return _cached(("forced", L, K, layout, n, filler), make)


def symmetric_rows(L, K, layout):
    """symmetric in structure, value and tag (the backward pass reuses the arrays): rows 0-11 hold row_lengths(L) neighbours (Havel-Hakimi,
    the idea of _gcn_graphs.symmetric_graph), an edge's slot is a symmetric function of its end points"""
    n = nodes_for(L)

    def make():
        want = row_lengths(L)
        for seed in range(200):
            rng = np.random.default_rng(1000 * L + seed)
            deg = np.array(want + list(rng.integers(2, 14, n - len(want))))
            if deg.sum() % 2:
                deg[-1] += 1
            edges = havel_hakimi(list(deg))
            if edges is not None:
                break
        else:
            raise AssertionError("no graph with the wanted row lengths")
        u, v = np.array(edges).T
        if layout == "slot0":
            s = np.zeros(len(u), np.int64)
        elif layout == "last":
            s = np.full(len(u), K - 1, np.int64)
        elif layout == "s036":
            s = np.array([0, K // 2, K - 1])[(u + v) % 3]
        else:
            s = (u + v) % K
        eid = np.arange(len(u))
        st = Structure(n, K, np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([s, s]), np.concatenate([eid, eid]))
        assert list(st.lengths()[:12]) == want
        return st
    return _cached(("sym", L, K, layout), make)


def hub_group_rows(K, L, G, threshold):
    """rows 0.. hold the hub lengths threshold + 1, G L - 1, G L, G L + 1 and one below G L (empty groups), slots spread over all K; the other
    rows stay at or below the threshold"""
    GL = max(G, 1) * L
    want = sorted(set([threshold + 1, GL - 1, GL, GL + 1, max(threshold + 2, GL // 2 - 3)]))
    n = max(259, (want[-1] + 4) | 1)

    def make():
        rng = np.random.default_rng(zlib.crc32(("hubgroup %d %d %d %d" % (K, L, G, threshold)).encode()))
        rows, cols, slots = [], [], []
        for r in range(n):
            length = want[r] if r < len(want) else int(rng.integers(0, threshold + 1))
            rows.append(np.full(length, r))
            cols.append(np.sort(rng.choice(np.delete(np.arange(n), r), length, replace=False)))
            slots.append(layout_slots("spread", length, K, L, 0))
        return Structure(n, K, np.concatenate(rows), np.concatenate(cols), np.concatenate(slots))
    return _cached(("hubgroup", K, L, G, threshold), make), want


def piece_rows(L, len_a, len_b):
    """n = 17 001, K = 3.  Hub ROWS 0 (len_a entries) and 1 (len_b, may be 0) with columns >= 4, hub COLUMNS 2 and 3 of the same lengths with
    rows >= 4 (the long rows of the transposed arrays), short rows elsewhere.  Slots of a hub row along its sorted entries: the first
    boundary falls exactly on the first piece boundary, the second in the middle of the second piece."""
    n, K = 17001, 3

    def make():
        rng = np.random.default_rng(zlib.crc32(("pieces %d %d %d" % (L, len_a, len_b)).encode()))
        split = max(1, -(-max(len_a, len_b) // HUB_SPLIT_ENTRIES))
        rows, cols, slots = [], [], []
        for hub, length in ((0, len_a), (1, len_b)):
            if not length:
                continue
            pieces = min(split, max(1, -(-length // HUB_SPLIT_ENTRIES)))
            plen = -(-(-(-length // pieces)) // L) * L if pieces > 1 else (length // 3) // L * L
            other = np.sort(rng.choice(np.arange(4, n), length, replace=False))
            i = np.arange(length)
            s = (i >= plen).astype(np.int64) + (i >= plen + plen // 2).astype(np.int64)
            rows += [np.full(length, hub), other]            # the hub row, and the hub column 2 + hub
            cols += [other, np.full(length, 2 + hub)]
            slots += [s, s]
        for r in range(4, n):
            length = int(rng.integers(0, 4))
            rows.append(np.full(length, r))
            cols.append(rng.choice(np.arange(4, n), length, replace=False))
            slots.append(np.sort(rng.integers(0, K, length)))
        st = Structure(n, K, np.concatenate(rows), np.concatenate(cols), np.concatenate(slots))
        key = st.rows * n + st.cols                           # a short row may repeat a column: keep the first
        _, first = np.unique(key, return_index=True)
        first.sort()
        return Structure(n, K, st.rows[first], st.cols[first], st.slots[first])
    return _cached(("pieces", L, len_a, len_b), make)


# ------------------------------------------------------------------------------------------------ cases
class Case(object):
    def __init__(self, id, struct, d, nested=True, self_loop=True, relu=True, long_row=None, symmetric=None, strided=False, expect=None):
        self.id, self.struct, self.d = id, struct, d
        self.nested, self.self_loop, self.relu = nested, self_loop, relu
        self.long_row = long_row                # CoreAdj.LONG_ROW for the case (None: the default, no hub rows at these sizes unless forced)
        self.symmetric = symmetric              # what CoreAdj must detect (None: not asserted)
        self.strided = strided                  # x is columns 1..d of an [n, d + 5] buffer: odd row stride, misaligned base -> scalar kernels
        self.expect = expect or {}              # what the API must expose: hubs / hubs_t (long-row counts), split / split_t (hub_split)

    @property
    def K(self):
        return self.struct.K

    @property
    def n(self):
        return self.struct.n

    def __repr__(self):
        return self.id

    def seed(self, what):
        return zlib.crc32((self.id + what).encode())


EXACT_LEVELS = (          # (x and dH as multiples of 1/4 up to ..., matrix values)
    (8, 8, (0.5, 1.0, 1.5)),
    (4, 4, (0.5, 1.0)),
    (2, 1, (0.5,)),
    (1, 1, (0.5,)),
)


def _inputs(case, level):
    n, d, K, st = case.n, case.d, case.K, case.struct
    rng = np.random.default_rng(case.seed("exact" if level is not None else "rounded"))
    n_edges = int(st.edge.max()) + 1 if len(st.edge) else 0
    if level is None:
        x = rng.standard_normal((n, d)).astype(np.float32).astype(np.float64)
        dH = rng.standard_normal((n, K, d)).astype(np.float32).astype(np.float64)
        vals = (rng.uniform(0.2, 1.0, n_edges) * rng.choice([-1.0, 1.0], n_edges)).astype(np.float32).astype(np.float64)
    else:
        xm, gm, vs = EXACT_LEVELS[level]
        x = rng.integers(-xm, xm + 1, (n, d)) * 0.25
        dH = rng.integers(-gm, gm + 1, (n, K, d)) * 0.25
        vals = rng.choice(vs, n_edges) * rng.choice([-1.0, 1.0], n_edges)
    return st.matrices(vals, case.nested), x, dH


def rounded_inputs(case):
    """(mats, x, dH, model): standard normal x and dH, uniform matrix values of both signs, all rounded to fp32 first"""
    mats, x, dH = _inputs(case, None)
    return mats, x, dH, R.model_all(mats, x, dH, case.self_loop, case.relu)


def exact_inputs(case):
    """(mats, x, dH, model, level): the widest value ranges of EXACT_LEVELS at which every term mass stays below 2^24 granules"""
    for level in range(len(EXACT_LEVELS)):
        mats, x, dH = _inputs(case, level)
        try:
            return mats, x, dH, R.exact_model(mats, x, dH, case.self_loop, case.relu), level
        except AssertionError:
            if level == len(EXACT_LEVELS) - 1:
                raise


F4_WIDTHS = (4, 32, 36, 64, 68, 128, 132, 256, 260, 516)      # LPR 8 | 16 | 32 | 64 | 64: second pass with one live lane | three passes
SCALAR_WIDTHS = (1, 7, 9, 15, 17, 31, 33, 63, 65, 129)        # LPR 8 | 16 | 32 | 64 | two passes | three passes
KS = (1, 2, 7, 33, 64, 65, 255)


def _flags(i):
    """rotate the flag combinations over a list of cases"""
    return dict(nested=bool(i & 1), self_loop=bool(i & 2), relu=not (i & 4))


def width_cases():
    out = []
    for i, d in enumerate(F4_WIDTHS + SCALAR_WIDTHS):
        vec, L, passes = plan(d, d in F4_WIDTHS)
        st = forced_rows(L, 7, "at4L")
        name = "row-%s-d%d-lpr%d-passes%d" % ("float4" if vec == 4 else "scalar", d, L, passes)
        out.append(Case(name + "-fwd", st, d, symmetric=False, **_flags(i)))                     # forced rows in the forward arrays
        out.append(Case(name + "-bwd", st.transposed(), d, symmetric=False, **_flags(i + 3)))    # ... in the arrays the backward reads
    out.append(Case("row-scalar-d128-strided-ldx133-lpr64-passes2", forced_rows(64, 7, "at4L"), 128, strided=True, symmetric=False))
    return out


def layout_cases():
    out = []
    for d, vec4 in ((36, True), (132, True), (7, False), (33, False)):
        L = plan(d, vec4)[1]
        for i, layout in enumerate(LAYOUTS):
            for t in (False, True):          # the forced rows in the forward arrays, and in the transposed arrays the backward reads
                st = forced_rows(L, 7, layout)
                out.append(Case("layout-%s-d%d-lpr%d-%s" % (layout, d, L, "bwd" if t else "fwd"), st.transposed() if t else st, d,
                                symmetric=False, **_flags(i + (4 if t else 0))))
    return out


def flag_cases():
    """every flag combination, over directed rows and over symmetric lists (arrays reused in backward); these also go through autograd"""
    out = []
    for i in range(8):
        f = _flags(i)
        name = "-".join(("nested" if f["nested"] else "general", "self" if f["self_loop"] else "noself", "relu" if f["relu"] else "linear"))
        out.append(Case("flags-%s-asymmetric-d36" % name, forced_rows(16, 7, "each"), 36, symmetric=False, **f))
        out.append(Case("flags-%s-symmetric-d7" % name, symmetric_rows(8, 7, "s036" if f["nested"] else "spread"), 7,
                        symmetric=f["nested"], **f))      # CoreAdj reuses the arrays for nested lists only
        out.append(Case("flags-%s-symmetric-d132" % name, symmetric_rows(64, 7, SYM_LAYOUTS[i % 4]), 132,
                        symmetric=f["nested"] or None, **f))
    return out


def k_cases():
    out = []
    for i, K in enumerate(KS):
        for d, vec4 in ((12, True), (5, False)):
            L = plan(d, vec4)[1]
            out.append(Case("slots-K%d-d%d-each" % (K, d), forced_rows(L, K, "each"), d, symmetric=False if K > 1 else None, **_flags(i)))
            out.append(Case("slots-K%d-d%d-spread-bwd" % (K, d), forced_rows(L, K, "spread").transposed(), d,
                            symmetric=False if K > 1 else None, **_flags(i + 1)))
    out.append(Case("slots-K255-d132-last", forced_rows(64, 255, "last"), 132, symmetric=False))
    return out


def hub_threshold_cases():
    out = []
    i = 0
    for threshold in (4, 12):
        for d, vec4 in ((32, True), (64, True), (128, True), (132, True), (7, False), (15, False), (31, False), (65, False)):
            vec, L, _ = plan(d, vec4)
            st = forced_rows(L, 7, "s036" if i % 2 else "each")
            lens, lens_t = st.lengths(), st.lengths(True)
            out.append(Case("hub-threshold%d-%s-d%d-lpr%d" % (threshold, "float4" if vec4 else "scalar", d, L), st, d, long_row=threshold,
                            symmetric=False, expect=dict(hubs=int((lens > threshold).sum()), hubs_t=int((lens_t > threshold).sum()), split=1),
                            **_flags(i)))
            i += 1
    st = symmetric_rows(16, 7, "spread")
    out.append(Case("hub-threshold4-symmetric-d36", st, 36, long_row=4, symmetric=True,
                    expect=dict(hubs=int((st.lengths() > 4).sum()), hubs_t=int((st.lengths() > 4).sum()))))
    return out


def hub_group_cases():
    """d = 132: float4, 64 lanes.  K = 9: G = 16 (all groups); 10: 14; 64: 2 with 128 KiB of LDS (the opt-in above 64 KiB); 144: 1; 145: the
    partials of one group exceed the budget, the rows stay with the row kernels"""
    out = []
    for i, K in enumerate((9, 10, 64, 144, 145)):
        G = hub_groups(K, 64, 4)
        assert G == {9: 16, 10: 14, 64: 2, 144: 1, 145: 0}[K]
        st, want = hub_group_rows(K, 64, G, 12)
        out.append(Case("hub-groups-K%d-G%d-d132" % (K, G) if G else "hub-fallback-K145-d132", st, 132, long_row=12, symmetric=False,
                        nested=i != 1, self_loop=i != 2, relu=i != 3,
                        expect=dict(hubs=len(want), hubs_t=int((st.lengths(True) > 12).sum()), split=1)))
    # the scalar kernels, 8 lanes: G = 128 groups of one row
    st, want = hub_group_rows(3, 8, 128, 12)
    out.append(Case("hub-groups-K3-G128-d5-scalar", st, 5, long_row=12, symmetric=False, expect=dict(hubs=len(want), split=1)))
    return out


def piece_cases():
    out = []
    for d in (12, 132):
        L = plan(d, True)[1]
        for i, (a, b, split) in enumerate(((8192, 0, 1), (8193, 0, 2), (16384, 0, 2), (16385, 8193, 3))):
            out.append(Case("hub-pieces-%d%s-split%d-d%d" % (a, "+%d" % b if b else "", split, d), piece_rows(L, a, b), d, symmetric=False,
                            nested=(i + d) % 2 == 0, self_loop=i != 1, relu=i != 2,
                            expect=dict(hubs=2 if b else 1, hubs_t=2 if b else 1, split=split, split_t=split)))
    return out


GROUPS = dict(widths=width_cases, layouts=layout_cases, flags=flag_cases, slots=k_cases, hub_threshold=hub_threshold_cases,
              hub_groups=hub_group_cases, hub_pieces=piece_cases)
_cases = {}


def cases(group):
    if group not in _cases:
        _cases[group] = GROUPS[group]()
        ids = [c.id for c in _cases[group]]
        assert len(set(ids)) == len(ids), ids
    return _cases[group]


def all_cases():
    return [c for g in GROUPS for c in cases(g)]


# ------------------------------------------------------------------------------------------------ agg_bwd_prep_kernel and spmm_csr
PREP_CASES = [(d, K) for d in (5, 8) for K in (1, 2, 64, 255)]


def prep_inputs(d, K, level, n=67):
    """H with exact +0.0 entries beside positive ones (and negative ones, which a relu output never holds but the mask must treat alike),
    dH; level None: the rounded tier"""
    rng = np.random.default_rng(zlib.crc32(("prep %d %d %s" % (d, K, level)).encode()))
    if level is None:
        H = np.maximum(rng.standard_normal((n, K, d)), 0.0).astype(np.float32).astype(np.float64)
        dH = rng.standard_normal((n, K, d)).astype(np.float32).astype(np.float64)
    else:
        gm = EXACT_LEVELS[level][1]
        H = np.maximum(rng.integers(-4, 9, (n, K, d)), 0) * 0.25
        dH = rng.integers(-gm, gm + 1, (n, K, d)) * 0.25
        dH[dH == 0] = 0.25                               # a masked entry always has a gradient to lose
    assert (H == 0).mean() > 0.2 and (H > 0).mean() > 0.2
    return H, dH


def prep_exact(d, K, nested, relu):
    for level in range(len(EXACT_LEVELS)):
        H, dH = prep_inputs(d, K, level)
        Z, S0 = R.backward_prep(H, dH, nested, relu)
        try:
            R.check_exact(Z, S0)
            return H, dH, Z, S0
        except AssertionError:
            if level == len(EXACT_LEVELS) - 1:
                raise


SPMM_CASES = [(4, True, False), (36, True, False), (132, True, False), (7, False, False), (65, False, False), (128, False, True)]


def spmm_case(d, vec4, strided):
    L = plan(d, vec4)[1]
    return Case("spmm-d%d-%s%s" % (d, "float4" if vec4 else "scalar", "-strided" if strided else ""), forced_rows(L, 1, "slot0"), d,
                self_loop=False, relu=False, strided=strided)
