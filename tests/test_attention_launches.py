"""GPU tier: which launches one forward and backward of each fused dot-product attention form makes -- the set of
(profile tag, kernel label, calls) -- and that they compute what the composed yardstick of functions.py computes.

Graph: 300 rows, about 3000 edges, chunks of at most 8 slots, so that at one chunk per lane group the rows of more than
8 edges and the hub row are shared between lane groups and leave the forwards as piece records.  The knobs turn every
fused form on at this size (attn_rows, attn_heads = 1; the walk of the one-head forward without a bias at 8 workgroups).
The tables were read from the profile of the commit before the host side of these ops was restated in one place; those
of the typed form (ETYPE_CASES: n_types = 5, inputs of attention_etype_reference.inputs) from the commit before its host
side became the edge form's.

Tolerances: the _compare of each op's own test file at factor 2 (two fp32 results compared with each other)."""
import pytest
import torch

import attention_dropout_reference as A
import attention_edge_reference as E
import attention_etype_reference as T
from custom_op_benchmark_amd import _lib, functions, graphop as ops
from test_attention_bias import _compare as compare_bias, _inputs as inputs_bias
from test_attention_dropout import _compare as compare_plain, _inputs as inputs_plain
from test_attention_edge import _compare as compare_edge
from test_attention_etype import _compare as compare_etype
from util import random_graph

pytestmark = pytest.mark.gpu

NONE, HALF = (0.0, 0, 0), (0.5, 1234567890123, 7)
N_TYPES = 5


def _table(zero_fills, fwd, pass_tag, pass_kernel, merge_kernel, pack, rows, rows_kernel, **more):
    """{tag: (kernel label, calls)}: the zero fills of both directions (stats, o, dQ, dK, dV and what the bindings
    clear), the three fills, the pass and the merge of a piece-record forward, then the pack and the two chunk-driver
    passes of the backward; more: the launches only this form makes"""
    return {"zero_fill": ("k_zero16", zero_fills), fwd + "_setup": ("k_fill", 1), pass_tag: (pass_kernel, 1),
            fwd + "_merge": (merge_kernel, 1), pack: ("k_" + pack, 1), rows + "_row": (rows_kernel, 1),
            rows + "_col": (rows_kernel, 1), **more}


def _etype_table(need_dR):
    """the typed form: the edge form's launches and, where dR is wanted, the zero fill of its replicas and their sum"""
    more = {"attn_etype_dr_reduce": ("k_attn_etype_dr_reduce", 1)} if need_dR else {}
    return _table(5 if need_dR else 4, "attn_etype_fwd", "attn_etype_fwd_rows", "k_attn_etype_fwd_rows_f32",
                  "k_attn_etype_piece_add", "attn_etype_pack", "attn_etype_rows", "k_attn_etype_bwd_rows_f32", **more)


# name -> (op, h, d, (p, seed, offset), wants the edge-sized gradient, expected launches)
CASES = {
    "plain": ("plain", 1, 64, NONE, True,
              _table(6, "attn_fwd", "attn_fwd", "k_attn_fwd_walk_f32", "k_attn_piece_add", "attn_pack", "attn_rows",
                     "k_attn_bwd_rows_f32")),
    "dropout": ("plain", 1, 64, HALF, True,
                _table(6, "attn_fwd", "attn_fwd", "k_attn_fwd_walk_f32<DROP>", "k_attn_piece_add", "attn_pack", "attn_rows",
                       "k_attn_bwd_rows_f32<DROP>")),
    "bias_db": ("bias", 1, 32, NONE, True,
                _table(5, "attn_bias_fwd", "attn_bias_fwd_rows", "k_attn_bias_fwd_rows_f32", "k_attn_bias_piece_add",
                       "attn_pack", "attn_bias_rows", "k_attn_bias_bwd_rows_f32")),
    "bias_no_db": ("bias", 1, 32, NONE, False,
                   _table(5, "attn_bias_fwd", "attn_bias_fwd_rows", "k_attn_bias_fwd_rows_f32", "k_attn_bias_piece_add",
                          "attn_pack", "attn_bias_rows", "k_attn_bias_bwd_rows_f32")),
    "bias_heads_dropout": ("bias", 4, 16, HALF, True,
                           _table(5, "attn_heads_fwd", "attn_heads_fwd_rows", "k_attn_heads_fwd_rows_f32",
                                  "k_attn_heads_piece_add", "attn_heads_pack", "attn_heads_rows",
                                  "k_attn_heads_bwd_rows_f32")),
    "edge": ("edge", 1, 64, NONE, True,
             _table(4, "attn_edge_fwd", "attn_edge_fwd_rows", "k_attn_edge_fwd_rows_f32", "k_attn_edge_piece_add",
                    "attn_edge_pack", "attn_edge_rows", "k_attn_edge_bwd_rows_f32")),
    "edge_heads": ("edge", 8, 32, NONE, True,
                   _table(4, "attn_edge_fwd", "attn_edge_fwd_rows", "k_attn_edge_fwd_rows_f32", "k_attn_edge_piece_add",
                          "attn_edge_pack", "attn_edge_rows", "k_attn_edge_bwd_rows_f32")),
}
# the typed form, n_types = N_TYPES: tables read from the profile of the commit before its host side was shared with
# the edge form's
ETYPE_CASES = {
    "etype": ("etype", 1, 64, NONE, True, _etype_table(True)),
    "etype_heads_dropout": ("etype", 4, 16, HALF, True, _etype_table(True)),
    "etype_heads_no_dr": ("etype", 8, 32, NONE, False, _etype_table(False)),
}


def _graph():
    g = random_graph(300, 300, 2700, seed=3, chunk_size=8, zero_rows=0.2, hub=150)          # (square: the composed SpMM
    deg = torch.bincount(g.src, minlength=g.n_src)                                           # returns zeros_like(V))
    assert (deg == 0).any() and deg.max() >= 150 and (deg > 8).sum() > 100 and (g.ptr_r[1:] - g.ptr_r[:-1]).max() <= 8
    return g


def _fused(op, a8, Q, K, V, x, dO, drop, need_dx):
    """one forward and backward through the entry points -> dict(o, stats, dQ, dK, dV[, dx])"""
    if op == "plain":
        o, stats = ops.attention_dropout_forward(*a8[:4], Q, K, V, *drop, 0) if drop[0] > 0 else \
            ops.attention_forward(*a8[:4], Q, K, V)
        grads = ops.attention_dropout_backward(*a8, Q, K, V, o, stats, dO, *drop, 0) if drop[0] > 0 else \
            ops.attention_backward(*a8, Q, K, V, o, stats, dO)
    elif op == "bias":
        o, stats = ops.attention_bias_forward(*a8[:4], Q, K, V, x, *drop, 0)
        grads = ops.attention_bias_backward(*a8, Q, K, V, x, o, stats, dO, *drop, 0, need_dx)
    elif op == "etype":
        o, stats = ops.attention_etype_forward(*a8[:4], Q, K, V, *x, *drop, 0)
        grads = ops.attention_etype_backward(*a8, Q, K, V, *x, o, stats, dO, *drop, 0, need_dx)
    else:
        o, stats = ops.attention_edge_forward(*a8[:4], Q, K, V, x, *drop, 0)
        grads = ops.attention_edge_backward(*a8, Q, K, V, x, o, stats, dO, *drop, 0, need_dx)
    torch.cuda.synchronize()
    return dict(zip(("o", "stats", "dQ", "dK", "dV", "dx"), (o, stats) + tuple(grads)))


def _composed(op, g, Q, K, V, x, dO, drop):
    """the composed yardstick of functions.py -> the same dict, stats = (m, 1 / l) of its scores"""
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    xg = None if x is None else (x[0] if op == "etype" else x).clone().requires_grad_(True)      # etype: x = (R, etype)
    if op == "plain":
        s, _, o = functions.attention_dropout_step(g, q, k, v, dO, *drop) if drop[0] > 0 else \
            functions.attention_step(g, q, k, v, dO)
    elif op == "bias":
        s, _, o = functions.attention_bias_step(g, q, k, v, xg, dO, *drop)
    elif op == "etype":
        s, _, o = functions.attention_etype_step(g, q, k, v, xg, x[1], dO, *drop)
    else:
        s, _, o = functions.attention_edge_step(g, q, k, v, xg, dO, *drop)
    torch.cuda.synchronize()
    s = s.detach().cpu().double()
    m, l = A.softmax_stats(g.src.cpu(), g.n_src, s.reshape(s.size(0), -1))
    stats = torch.stack([m, torch.where(l > 0, 1 / l, torch.zeros_like(l))], -1)
    return dict(o=o.detach(), stats=stats, dQ=q.grad, dK=k.grad, dV=v.grad, dx=None if xg is None else xg.grad)


@pytest.mark.parametrize("name", list(CASES) + list(ETYPE_CASES))
def test_launches_and_results(dev, name):
    op, h, d, drop, need_dx, table = {**CASES, **ETYPE_CASES}[name]
    g = _graph()
    if op == "edge":
        Q, K, V, x, dO = (t.to(dev) for t in E.graph_inputs(g, h, d, torch.float32, seed=h * 100 + d))
    elif op == "etype":
        Q, K, V, R, etype, dO = (t.to(dev) for t in T.inputs(g, h, d, torch.float32, h * 100 + d, N_TYPES))
        x = (R, etype)
    elif op == "bias":
        Q, K, V, x, dO = (t.to(dev) for t in inputs_bias(g, h, d, torch.float32, seed=h * 100 + d))
    else:
        (Q, K, V, dO), x = (t.to(dev) for t in inputs_plain(g, h, d, torch.float32, seed=h * 100 + d)), None
    gd = g.to(dev)
    want = _composed(op, gd, Q, K, V, x, dO, drop)
    for knob, v in dict(attn_rows=1, attn_heads=1, sweep_min_kb=0, sweep_min_granule=0, walk_min_bin=0, walk_blocks=8).items():
        _lib.tune(knob, v)
    _lib.clear_plan_cache()
    try:
        a8 = gd.csr_args()
        _fused(op, a8, Q, K, V, x, dO, drop, need_dx)          # the plans and their layouts are built here
        _lib.profile_enable(True)
        try:
            got = _fused(op, a8, Q, K, V, x, dO, drop, need_dx)
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()
    seen = {tag: (r["kernel"], r["calls"]) for tag, r in prof.items()}
    print(name, sorted(seen.items()))
    assert seen == table
    compare = {"plain": compare_plain, "bias": compare_bias, "edge": compare_edge, "etype": compare_etype}[op]
    compare(got, want, torch.float32, drop[0], name + " ", factor=2, keys=("o", "dQ", "dK", "dV"))
    if op == "plain":
        assert "dx" not in got
    elif need_dx and op == "etype":
        compare(dict(dR=got["dx"]), dict(dR=want["dx"]), torch.float32, drop[0], name + " ", factor=2, keys=("dR",),
                n_max=T.n_max(x[1].cpu(), N_TYPES))
    elif need_dx:
        compare(got, want, torch.float32, drop[0], name + " ", factor=2, keys=("dx",))
    else:
        assert got["dx"].numel() == 0
    has = (torch.bincount(g.src, minlength=g.n_src) > 0)
    st = got["stats"].cpu().reshape(g.n_src, h, 2)
    compare(dict(stats=st[has]), dict(stats=want["stats"][has].float()), torch.float32, 0.0, name + " ", factor=2,
            keys=("stats",))
