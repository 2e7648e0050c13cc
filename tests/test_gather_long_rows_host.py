"""The long-row refusals of every pull-form gather entry point (ctgcn_gcn.hip, ctgcn_gat.hip, ctgcn_pool.hip), pinned per entry point:
return code for each refusal, and the ctgcn_last_error text of the limit and workspace refusals.  Every call fails its argument checks
before any launch.  No GPU needed.

The accepted side of the workspace size (exactly one piece per row) needs a refusal after the long-row set-up to stop the call.  The gcn
and pool entry points have one (a null feature pointer).  ctgcn_gat_fwd_f32 has one only at a shape whose (row, head) pairs exceed one
launch, so that case alone leaves n = 4, d = 6, heads = 2.  ctgcn_gat_bwd_row_f32 and ctgcn_gat_bwd_col_f32 launch right after the
set-up: for them only the refusing side (one byte below) is pinned."""
import ctypes

import pytest

INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
N, D, HEADS = 4, 6, 2
p = ctypes.c_void_p(64)              # never dereferenced
ROW = (D + 3) // 4 * 4 * 4           # bytes of one partial vector: round_up(d, 4) floats

GCN_TEXT = "long rows need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes (one piece per row)"
GAT_TEXT = "long rows need a 16-byte aligned workspace of at least n_long * ctgcn_gat_piece_floats(d, heads) * 4 bytes (one piece per row)"
POOL_TEXT = ("long rows need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes (8 for pool_max_fwd), "
             "one piece per row")


def lib():
    from ctgcn_amd import _lib
    return _lib.load()


# each call is accepted but for its long-row arguments; feat is the feature pointer whose null check follows the long-row set-up
def gcn_layer_fwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=None):
    return lib().ctgcn_gcn_layer_fwd_f32(n, d, p, p, p, feat, d, p, d, 1, None, None, lr, nl, thr, ws, wsb, None)


def gcn_layer_bwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=None):
    return lib().ctgcn_gcn_layer_bwd_f32(n, d, p, p, p, feat, d, p, d, 1, p, d, lr, nl, thr, ws, wsb, None)


def gcn_conv_fwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=None):
    return lib().ctgcn_gcn_conv_fwd_f32(n, d, p, p, p, feat, d, p, p, d, 2, 0.0, 1, p, lr, nl, thr, ws, wsb, None)


def gat_fwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=HEADS):
    return lib().ctgcn_gat_fwd_f32(n, d, heads, p, p, feat, d, p, p, 0.2, 2, 0.0, 1, 0.0, 2, p, d, p, d, p, p, p, p, lr, nl, thr, ws, wsb, None)


def gat_bwd_row(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=HEADS):
    return lib().ctgcn_gat_bwd_row_f32(n, d, heads, p, p, feat, d, p, d, p, p, 0.2, 0.0, 1, p, d, p, p, lr, nl, thr, ws, wsb, None)


def gat_bwd_col(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=HEADS):
    return lib().ctgcn_gat_bwd_col_f32(n, d, heads, p, p, feat, d, p, d, p, p, p, p, 0.2, 0.0, 1, p, p, d, p, d, p, p, lr, nl, thr, ws, wsb, None)


def pool_conv_fwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=None):
    return lib().ctgcn_pool_conv_fwd_f32(n, d, p, p, p, p, d, p, d, 1.0, p, feat, d, 1, 0.0, 1, p, p, d, lr, nl, thr, ws, wsb, None)


def pool_max_fwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=None):
    return lib().ctgcn_pool_max_fwd_f32(n, d, p, p, feat, d, p, d, p, d, lr, nl, thr, ws, wsb, None)


def pool_max_bwd(lr, nl, thr, ws, wsb, n=N, feat=p, d=D, heads=None):
    return lib().ctgcn_pool_max_bwd_f32(n, d, p, p, feat, d, p, d, p, d, lr, nl, thr, ws, wsb, None)


def gat_piece_bytes(d=D, heads=HEADS):
    return lib().ctgcn_gat_piece_floats(d, heads) * 4


# name: (call, bytes of one piece of one row, the workspace refusal's text, whether a null feature pointer is refused after the set-up)
ENTRY_POINTS = {
    "gcn_layer_fwd": (gcn_layer_fwd, lambda: ROW, GCN_TEXT, True),
    "gcn_layer_bwd": (gcn_layer_bwd, lambda: ROW, GCN_TEXT, True),
    "gcn_conv_fwd": (gcn_conv_fwd, lambda: ROW, GCN_TEXT, True),
    "gat_fwd": (gat_fwd, gat_piece_bytes, GAT_TEXT, False),
    "gat_bwd_row": (gat_bwd_row, gat_piece_bytes, GAT_TEXT, False),
    "gat_bwd_col": (gat_bwd_col, gat_piece_bytes, GAT_TEXT, False),
    "pool_conv_fwd": (pool_conv_fwd, lambda: ROW, POOL_TEXT, True),
    "pool_max_fwd": (pool_max_fwd, lambda: 2 * ROW, POOL_TEXT, True),
    "pool_max_bwd": (pool_max_bwd, lambda: ROW, POOL_TEXT, True),
}


def last_error():
    return lib().ctgcn_last_error().decode()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_long_row_refusals(name):
    call, piece_bytes, text, stops_later = ENTRY_POINTS[name]
    big = 1 << 20
    assert call(p, -1, 8, p, big) == INVALID
    assert call(p, N + 1, 8, p, big) == INVALID
    assert last_error() == name + ": n_long outside [0, n]"
    assert call(None, 1, 8, p, big) == INVALID
    assert last_error() == name + ": n_long > 0 without long_rows"
    assert call(p, 1, 0, p, big) == INVALID
    assert call(p, 1, 2 ** 29, p, big) == INVALID
    assert last_error() == name + ": long_threshold outside [1, 2^29)"
    assert call(p, 1, 2 ** 29 - 1, None, 0) == WORKSPACE         # the largest threshold passes on to the workspace check
    assert call(p, 65536, 8, p, 1 << 40, n=65536) == UNSUPPORTED
    assert last_error() == name + ": more than 65535 long rows: raise long_threshold"
    assert call(p, 65535, 8, None, 0, n=65536) == WORKSPACE
    for nl in (1, 3):
        one = nl * piece_bytes()
        assert call(p, nl, 8, None, big) == WORKSPACE
        assert call(p, nl, 8, ctypes.c_void_p(72), big) == WORKSPACE     # 8 mod 16
        assert call(p, nl, 8, p, one - 1) == WORKSPACE
        assert last_error() == name + ": " + text
        if stops_later:
            assert call(p, nl, 8, p, one, feat=None) == INVALID
            assert last_error() == name + ": null pointer"


def test_gat_fwd_accepts_exactly_one_piece_per_row():
    """2^31 - 1 rows of 2^20 heads of width 1 are more (row, head) pairs than one launch takes: refused after the long-row set-up"""
    n, d = 2 ** 31 - 1, 2 ** 20
    one = 3 * gat_piece_bytes(d, d)
    assert one == 3 * (2 * d + d) * 4
    assert gat_fwd(p, 3, 8, p, one - 1, n=n, d=d, heads=d) == WORKSPACE
    assert gat_fwd(p, 3, 8, p, one, n=n, d=d, heads=d) == UNSUPPORTED
    assert last_error() == "gat: n * heads too large for one launch"
