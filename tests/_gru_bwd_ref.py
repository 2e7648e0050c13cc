"""Host model of the fused GRU backward (ctgcn_gru_bwd_rec_f32 / ctgcn_gru_bwd_in_f32, include/ctgcn_hip.h), in plain numpy, written
from the header's contract and the formulas at the top of gru_bwd_rec_kernel — no GPU, no torch.

Two uses (tests/test_gru_bwd_ref_host.py pins the model itself against float64 autograd of nn.GRU):

  * numeric: rec() / inp() in float64 (the reference) and in float32 (the yardstick "what plain fp32 arithmetic loses") on the very
    float32 operands the kernels read;
  * exact: exact_case() draws dyadic inputs and runs the model under an Audit that asserts, on the CPU, what makes the kernels'
    bf16 x 2 split arithmetic EXACT for them: every value a kernel publishes to an operand plane equals bf16(v) + bf16(v - bf16(v)),
    the dropped lo·lo term of every product is 0, every elementwise intermediate is a float32, and every sum an MFMA or a reduction
    forms in an order the model does not know is bounded by (sum of |terms|) < 2^24 granules — then EVERY order of EVERY partial sum is
    a float32, and the kernels must give the model's numbers bit for bit.  A routing error is a hard failure, not a tolerance question.
"""
import numpy as np

H = 128
G3 = 3 * H
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------- bf16 split
def bf16(v):
    """round to nearest even to bfloat16, returned as float32"""
    a = np.ascontiguousarray(v, dtype=np.float32)
    u = a.view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)      # finite inputs: no carry out of the exponent
    return r.view(np.float32).reshape(a.shape)


def split2(v):
    """the kernels' bf16_split2: hi = bf16(x), lo = bf16(x - hi) in float32"""
    a = np.ascontiguousarray(v, dtype=np.float32)
    hi = bf16(a)
    return hi, bf16(a - hi)


def _granule(*arrays):
    """largest power of two that divides every nonzero entry (1.0 for all-zero input)"""
    k = -60
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        a = np.abs(a[a != 0])
        if a.size == 0:
            continue
        m, e = np.frexp(a)                                  # a = m 2^e, m in [0.5, 1): m 2^53 is an integer
        mi = (m * (1 << 53)).astype(np.int64)
        tz = np.zeros(mi.shape, dtype=np.int64)
        low = mi & -mi
        tz = np.log2(low.astype(np.float64)).astype(np.int64)
        k = max(k, int((53 - tz - e).max()))                # a is a multiple of 2^-(53 - tz - e)
    return 2.0 ** (-k) if k > -60 else 1.0


class Audit(object):
    """collects the exactness conditions of one exact case; finish() asserts the order-free sum bounds"""

    def __init__(self):
        self.sums = {}
        self.count = 0

    def f32(self, tag, v):
        v = np.asarray(v, dtype=np.float64)
        assert np.isfinite(v).all(), tag
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "%s is no float32" % tag
        self.count += 1
        return v

    def plane(self, tag, v):
        v = self.f32(tag, v)
        hi, lo = split2(v)
        assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), v), "%s: hi + lo != value (more than 16 significant bits)" % tag
        return v

    def product(self, tag, a, b):
        """sum_k a[..., k] b[k, ...] by split MFMAs: both operands are planes (checked by the caller or here), no lo·lo term, and the
        terms enter the order-free bound of `tag`"""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        la, lb = np.abs(split2(a)[1]).astype(np.float64), np.abs(split2(b)[1]).astype(np.float64)
        assert not (la @ lb).any(), "%s: a lo·lo term is not 0" % tag
        self.terms(tag, np.abs(a) @ np.abs(b), _granule(a) * _granule(b))

    def terms(self, tag, abs_sum, granule):
        s, g = self.sums.get(tag, (0.0, 1.0))
        self.sums[tag] = (s + np.asarray(abs_sum, dtype=np.float64), min(g, granule))

    def finish(self):
        for tag, (s, g) in self.sums.items():
            assert float(np.max(s)) / g < 2.0 ** 24, "%s: sum of |terms| %g at granule %g: a partial sum may not be a float32" % (tag, np.max(s), g)
        return self


# ------------------------------------------------------------------------------------------------------------------ masks
PATTERNS = ("ones", "first-only", "top-and-zero", "nested-like", "alternating", "random", "first-then-ones",
            "low-word-only", "b0-32", "b0-31-32", "b0-63")


def make_masks(pattern, rows, steps, seed=0):
    """one Python int per 16-row tile, bit t set = step t is fresh; bit 0 always set, no bit at or above `steps`"""
    nt = (rows + 15) // 16
    S = steps
    full = (1 << S) - 1
    rng = np.random.default_rng(1000 + seed)
    out = []
    for i in range(nt):
        if pattern == "ones":
            m = full
        elif pattern == "first-only":
            m = 1
        elif pattern == "top-and-zero":
            m = 1 | (1 << (S - 1))
        elif pattern == "nested-like":                      # bit 0 | bits f .. S-1; f = S (nothing but bit 0) and f = 1 (everything) included
            f = (S, 1, 2, S - 1, (S + 1) // 2, 32, 33)[i % 7] if S > 34 else (S, 1, 2, S - 1, (S + 1) // 2)[i % 5]
            f = min(max(f, 1), S)
            m = 1 | (full & ~((1 << f) - 1))
        elif pattern == "alternating":
            m = sum(1 << t for t in range(0, S, 2)) if i % 2 == 0 else 1 | sum(1 << t for t in range(1, S, 2))
        elif pattern == "random":
            m = (int(rng.integers(0, 1 << 32)) | (int(rng.integers(0, 1 << 32)) << 32)) & full
        elif pattern == "first-then-ones":
            m = 1 if i % 2 == 0 else full
        elif pattern == "low-word-only":
            m = int(rng.integers(0, 1 << 32)) | (1 << 31)
        elif pattern == "b0-32":
            m = 1 | (1 << 32)
        elif pattern == "b0-31-32":
            m = 1 | (1 << 31) | (1 << 32)
        elif pattern == "b0-63":
            m = 1 | (1 << 63)
        else:
            raise ValueError(pattern)
        out.append((m | 1) & full)
    return out


def pack_masks(mask_bits, steps, garbage_seed=None):
    """the tile_mask operand: one uint32 per tile up to 32 steps, two (steps 0-31, 32-63) beyond.  garbage_seed: random bits at and
    above `steps` (the contract: ignored), bit `steps` itself and the word's top bit always among them"""
    if mask_bits is None:
        return None
    bits = 64 if steps > 32 else 32
    if garbage_seed is not None:
        assert steps < bits
        rng = np.random.default_rng(garbage_seed)
        junk = lambda: int(rng.integers(0, 1 << 32)) | (int(rng.integers(0, 1 << 32)) << 32) | (1 << (bits - 1)) | (1 << steps)
        mask_bits = [(m | (junk() & ~((1 << steps) - 1))) & ((1 << bits) - 1) for m in mask_bits]
    if steps > 32:
        return np.array([w for m in mask_bits for w in (m & 0xFFFFFFFF, m >> 32)], dtype=np.uint32)
    return np.array([m & 0xFFFFFFFF for m in mask_bits], dtype=np.uint32)


def fresh_matrix(mask_bits, rows, steps):
    """bool [rows, steps]"""
    f = np.ones((rows, steps), dtype=bool)
    if mask_bits is not None:
        for i, m in enumerate(mask_bits):
            assert m & 1, "bit 0 of every tile's mask is set"
            f[16 * i: 16 * i + 16] = [(m >> t) & 1 for t in range(steps)]
    return f


# ----------------------------------------------------------------------------------------------------------------- planes
def build_planes(x, plane_rows, first_row=0, exact=False, seed=0):
    """x [rows, steps, 128] -> (uint8 buffer in the layout ctgcn_core_aggregate_split_f32 writes at d = 128: fp16 plane 1 [plane_rows, 128],
    fp16 plane 2, fp32 row scales [plane_rows]; the sequences at [first_row, first_row + rows), every other row NaN), and the float32
    values the kernel decodes from it, ((float) p1 + (float) p2) * scale.  exact: plane 2 is 0 and the scales are powers of two."""
    rows, steps, d = x.shape
    assert d == H and (first_row + rows) * steps <= plane_rows
    x = np.asarray(x, dtype=np.float32).reshape(rows * steps, H)
    if exact:
        scale = (2.0 ** np.random.default_rng(seed).integers(-1, 3, rows * steps)).astype(np.float32)
    else:
        scale = np.abs(x).max(1).astype(np.float32)
        scale[scale == 0] = 1.0
    u = x / scale[:, None]
    p1 = u.astype(np.float16)
    p2 = np.zeros_like(p1) if exact else (u - p1.astype(np.float32)).astype(np.float16)
    dec = (p1.astype(np.float32) + p2.astype(np.float32)) * scale[:, None]
    if exact:
        assert np.array_equal(dec, x), "an exact case's x must survive the planes"
    P1 = np.full((plane_rows, H), NAN, dtype=np.float16)
    P2 = np.full((plane_rows, H), NAN, dtype=np.float16)
    SC = np.full(plane_rows, NAN, dtype=np.float32)
    lo = first_row * steps
    P1[lo: lo + rows * steps], P2[lo: lo + rows * steps], SC[lo: lo + rows * steps] = p1, p2, scale
    buf = np.concatenate([P1.view(np.uint8).ravel(), P2.view(np.uint8).ravel(), SC.view(np.uint8).ravel()])
    return buf, dec.reshape(rows, steps, H)


def poison_planes(buf, plane_rows, first_row, fresh):
    """NaN in the rows of the non-fresh row-steps (planes and scales)"""
    rows, steps = fresh.shape
    out = buf.copy()
    half = out[: 4 * plane_rows * H].view(np.float16).reshape(2, plane_rows, H)
    sc = out[4 * plane_rows * H:].view(np.float32)
    idx = first_row * steps + np.flatnonzero(~fresh.ravel())
    half[:, idx] = NAN
    sc[idx] = NAN
    return out


# ------------------------------------------------------------------------------------------------------------- the model
def forward(x, w_ih, w_hh, b_ih, b_hh, dtype=np.float64):
    """nn.GRU's forward from h = 0 in `dtype`: gates [rows, steps, 4, 128] = r, z, n, q (q = W_hn h_{t-1} + b_hn) and hseq"""
    x, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, dtype=dtype) for a in (x, w_ih, w_hh, b_ih, b_hh))
    R, S = x.shape[:2]
    gates, hseq = np.zeros((R, S, 4, H), dtype=dtype), np.zeros((R, S, H), dtype=dtype)
    h = np.zeros((R, H), dtype=dtype)
    sig = lambda a: dtype(1) / (dtype(1) + np.exp(-a))
    for t in range(S):
        gi, gh = x[:, t] @ w_ih.T + b_ih, h @ w_hh.T + b_hh
        r, z = sig(gi[:, :H] + gh[:, :H]), sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        n = np.tanh(gi[:, 2 * H:] + r * q)
        h = n + z * (h - n)
        gates[:, t], hseq[:, t] = np.stack([r, z, n, q], 1), h
    return gates, hseq


def rec(gates, gate_count, hseq, w_hh, mask_bits, steps, dh_sum=None, dh_seq=None, dtype=np.float64, audit=None):
    """ctgcn_gru_bwd_rec_f32.  gates [rows, steps, gate_count, 128] (4: r, z, n, q; 3: r, z, q), hseq [rows, steps, 128], exactly one of
    dh_sum [rows, 128] / dh_seq [rows, steps, 128], w_hh [384, 128].  Returns d_gi [rows, steps, 384] (NaN where the kernel does not
    write: the steps that are not fresh), dW_hh [384, 128], the n-gate column of db_hh [128]."""
    assert (dh_sum is None) != (dh_seq is None) and gate_count in (3, 4)
    gates, hseq, w = np.asarray(gates, dtype=dtype), np.asarray(hseq, dtype=dtype), np.asarray(w_hh, dtype=dtype)
    R, S = hseq.shape[0], steps
    fresh = fresh_matrix(mask_bits, R, S)
    A = audit
    c = (lambda tag, v: A.f32(tag, v)) if A else (lambda tag, v: v)
    p = (lambda tag, v: A.plane(tag, v)) if A else (lambda tag, v: v)
    if A:
        A.plane("W_hh", w)
    d_gi = np.full((R, S, G3), NAN, dtype=dtype)
    dW, dbn = np.zeros((G3, H), dtype=dtype), np.zeros(H, dtype=dtype)
    drec = np.zeros((R, H), dtype=dtype)
    gs = np.zeros((R, G3), dtype=dtype)
    one = dtype(1)
    for t in range(S - 1, -1, -1):
        dh = c("dh", drec + (np.asarray(dh_sum, dtype=dtype) if dh_sum is not None else np.asarray(dh_seq[:, t], dtype=dtype)))
        r, z, q = gates[:, t, 0], gates[:, t, 1], gates[:, t, gate_count - 1]
        hp = hseq[:, t - 1] if t > 0 else np.zeros((R, H), dtype=dtype)
        omz = c("1-z", one - z)
        if gate_count == 3:
            hcur = hseq[:, t]
            diff = c("h_t - h_{t-1}", hcur - hp)
            big = omz > np.float32(1e-6)
            n = np.where(big, hp + c("(h_t - h_{t-1}) / (1-z)", diff / np.where(big, omz, one)), hp)
            n = c("n rebuilt", n)
        else:
            n = gates[:, t, 2]
        dan = c("da_n", c("dh(1-z)", dh * omz) * c("1-n^2", one - c("n^2", n * n)))
        if gate_count == 3:
            daz = c("da_z", c("dh(h_{t-1}-h_t)", dh * c("h_{t-1}-h_t", hp - hcur)) * z)
        else:
            daz = c("da_z", c("dh(h_{t-1}-n)z", c("dh(h_{t-1}-n)", dh * c("h_{t-1}-n", hp - n)) * z) * omz)
        dar = c("da_r", c("da_n q r", c("da_n q", dan * q) * r) * c("1-r", one - r))
        dgn = c("dgh_n", dan * r)
        drec = c("dh z", dh * z)
        gs = c("d_gi running sum", gs + np.concatenate([dar, daz, dan], 1))
        if A:
            A.terms("db_hn", np.abs(dgn).sum(0), _granule(dgn))
        dbn = dbn + dgn.sum(0)
        if t > 0:
            g = np.concatenate([dar, daz, dgn], 1)
            if A:
                p("da_r | da_z | dgh_n", g)
                p("h_{t-1}", hp)
                A.product("dW_hh", g.T, hp)
                # the recurrent product, per row: |G| |W| bounds every order of its three accumulators
                la = np.abs(split2(g)[1]).astype(np.float64) @ np.abs(split2(w)[1]).astype(np.float64)
                assert not la.any(), "recurrent product: a lo·lo term is not 0"
                assert float((np.abs(g) @ np.abs(w)).max()) / (_granule(g) * _granule(w)) < 2.0 ** 24, "recurrent product"
            dW = dW + g.T @ hp
            drec = c("dh_{t-1}", drec + g @ w)
        wr = fresh[:, t]
        d_gi[wr, t] = gs[wr]
        gs = np.where(wr[:, None], 0, gs)
    if A:
        A.f32("dW_hh", dW)
        A.f32("db_hn", dbn)
        A.plane("d_gi", np.nan_to_num(d_gi))
    return d_gi, dW, dbn


def inp(d_gi, w_ih, mask_bits, x, steps, order=None, nested=0, self_loop=False, zout=False, n_out=None, dtype=np.float64, audit=None):
    """ctgcn_gru_bwd_in_f32 over the fresh (row, step) units only.  d_gi [rows, steps, 384] (read at fresh steps only), x [rows, steps, 128]
    (the values the kernel sees: fp32 rows, or the decoded planes).  Returns a dict: dW [384, 128], db [384] and either dx [rows, steps, 128]
    (NaN at steps that are not fresh) or, zout, Z [n_out, steps, 128] and S0 [n_out, 128] (None without self loop) with NaN where nothing
    is written:  G_t = sum_{fresh j >= t} dx_j [x_j > 0];  Z[order[p], t] = nested ? sum_{fresh i >= t} G_i : G_t;  S0[order[p]] = G_0."""
    R, S = x.shape[0], steps
    fresh = fresh_matrix(mask_bits, R, S)
    g = np.where(fresh[:, :, None], np.asarray(d_gi, dtype=dtype), 0).astype(dtype)
    xx = np.where(fresh[:, :, None], np.asarray(x, dtype=dtype), 0).astype(dtype)
    w = np.asarray(w_ih, dtype=dtype)
    A = audit
    if A:
        A.plane("W_ih", w)
        A.plane("d_gi read", g)
        A.plane("x", xx)
        A.product("dW_ih", g.reshape(R * S, G3).T, xx.reshape(R * S, H))
        A.terms("db_ih", np.abs(g).sum((0, 1)), _granule(g))
        assert not (np.abs(split2(g)[1]).astype(np.float64).reshape(R * S, G3) @ np.abs(split2(w)[1]).astype(np.float64)).any(), "dx: lo·lo"
        assert float((np.abs(g).reshape(R * S, G3) @ np.abs(w)).max()) / (_granule(g) * _granule(w)) < 2.0 ** 24, "dx product"
    dxv = (g.reshape(R * S, G3) @ w).reshape(R, S, H)
    out = {"dW": g.reshape(R * S, G3).T @ xx.reshape(R * S, H), "db": g.sum((0, 1))}
    if A:
        A.f32("dx", dxv), A.f32("dW_ih", out["dW"]), A.f32("db_ih", out["db"])
    if not zout:
        out["dx"] = np.where(fresh[:, :, None], dxv, NAN)
        return out
    n_out = R if n_out is None else n_out
    rowmap = np.arange(R) if order is None else np.asarray(order)[:R]
    Z = np.full((n_out, S, H), NAN, dtype=dtype)
    S0 = np.full((n_out, H), NAN, dtype=dtype) if self_loop else None
    Gr, Zr = np.zeros((R, H), dtype=dtype), np.zeros((R, H), dtype=dtype)
    for t in range(S - 1, -1, -1):
        wr = fresh[:, t]
        Gr = Gr + np.where((xx[:, t] > 0) & wr[:, None], dxv[:, t], 0)
        Zr = Zr + np.where(wr[:, None], Gr, 0)
        if A:
            A.f32("G_t", Gr), A.f32("Z_t", Zr)
        Z[rowmap[wr], t] = (Zr if nested else Gr)[wr]
    if self_loop:
        S0[rowmap] = Gr
    out["Z"], out["S0"] = Z, S0
    return out


# ----------------------------------------------------------------------------------------------------------- the exact tier
def _signed_perm(rng, halves):
    """[384, 128]: per gate block a signed permutation matrix (entries ±1, `halves` of them ±0.5)"""
    w = np.zeros((G3, H))
    for gblk in range(3):
        perm = rng.permutation(H)
        s = rng.choice([-1.0, 1.0], H)
        s[rng.permutation(H)[:halves[gblk]]] *= 0.5
        w[gblk * H + np.arange(H), perm] = s
    return w


def exact_inputs(rows, steps, seed, negatives=True):
    """dyadic operands of one exact case (float64 arrays holding float32 values): gates [rows, steps, 4, 128] (r, z, n, q), hseq,
    dh_sum, dh_seq, w_hh, w_ih, x.  z in {0, 1} and r in {0, 1} except 0.5 on half the units of one step per sequence each; n in
    {0, ±1} (|1 - n^2| <= 1: nothing amplifies along the steps, n = ±1 under z = 0 ends a gradient's chain); q, dh, x small integers;
    h_t = n + z (h_{t-1} - n), multiples of 1/2."""
    rng = np.random.default_rng(seed)
    R, S = rows, steps
    z = rng.integers(0, 2, (R, S, H)).astype(np.float64)
    r = rng.integers(0, 2, (R, S, H)).astype(np.float64)
    for a in (z, r):
        t = rng.integers(0, S, R)
        sel = rng.random((R, H)) < 0.5
        a[np.arange(R), t] = np.where(sel, 0.5, a[np.arange(R), t])
    n = rng.integers(-1, 2, (R, S, H)).astype(np.float64)
    q = rng.integers(-2, 3, (R, S, H)).astype(np.float64)
    hseq = np.zeros((R, S, H))
    hp = np.zeros((R, H))
    for t in range(S):
        hp = n[:, t] + z[:, t] * (hp - n[:, t])
        hseq[:, t] = hp
    n = np.where(z == 1, np.roll(hseq, 1, 1) * (np.arange(S)[None, :, None] > 0), n)      # where z = 1 the three-gate form rebuilds n = h_{t-1}
    dh_sum = rng.integers(-1, 2, (R, H)) * (rng.random((R, H)) < 0.4)
    dh_seq = rng.integers(-2, 3, (R, S, H)) * (rng.random((R, S, H)) < 0.3)
    x = rng.integers(-2, 4, (R, S, H)).astype(np.float64)
    if not negatives:
        x = np.maximum(x, 0)
    return {"gates": np.stack([r, z, n, q], 2), "hseq": hseq, "dh_sum": dh_sum.astype(np.float64), "dh_seq": dh_seq.astype(np.float64),
            "w_hh": _signed_perm(rng, (16, 16, 4)), "w_ih": _signed_perm(rng, (16, 16, 16)), "x": x}


def exact_case(rows, steps, mask_bits, gate_count=4, per_step=False, seed=0, negatives=True, order=None, nested=0, self_loop=False,
               zout=False, n_out=None, audit=True):
    """inputs + the model's outputs of one exact case, after the Audit has passed (AssertionError otherwise; audit=False skips it: the
    GPU tests, whose cases tests/test_gru_bwd_ref_host.py audits).  Returns (inputs, want)
    with want = {"d_gi", "dW_hh", "db_hn", "dW_ih", "db_ih", "dx" | ("Z", "S0")}, float64."""
    t = exact_inputs(rows, steps, seed, negatives)
    A = Audit() if audit else None
    for k, v in t.items():
        if A:
            (A.f32 if k in ("gates", "dh_sum", "dh_seq") else A.plane)(k, v)
    gates = t["gates"] if gate_count == 4 else t["gates"][:, :, [0, 1, 3]]
    d_gi, dW, dbn = rec(gates, gate_count, t["hseq"], t["w_hh"], mask_bits, steps, dh_sum=None if per_step else t["dh_sum"],
                        dh_seq=t["dh_seq"] if per_step else None, audit=A)
    want = inp(d_gi, t["w_ih"], mask_bits, t["x"], steps, order=order, nested=nested, self_loop=self_loop, zout=zout, n_out=n_out, audit=A)
    if A:
        A.finish()
    want = dict(want, dW_ih=want.pop("dW"), db_ih=want.pop("db"), d_gi=d_gi, dW_hh=dW, db_hn=dbn)
    t["gates_used"] = gates
    return t, want
