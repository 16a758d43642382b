"""CPU tier of the fused GATv2 layer on bfloat16 tables (kernels_gatv2_attn_bf16.h): the float64 reference
against the family's, the three new symbols under ABI 8 and the routing predicate, how much of each bound of the GPU tier
an fp32 evaluation with one bf16 rounding uses by itself, a named refusal, and a gfx950 code object without scratch."""
import ctypes
import os
import re
import sys

import pytest
import torch

import fused_gatv2_reference as G
import gatv2_bf16_reference as R
from dropout_reference import multipliers
from test_attention_bf16_host import _plan, lib          # noqa: F401 (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, dict(rtol=1e-4, atol=1e-5)          # (TOL[torch.float32] of test_fused_attention.py)


def _r3(g, h, inp):
    xl, xr, att, dO = inp
    return (xl.reshape(g.n_src, h, -1), xr.reshape(g.n_dst, h, -1), att.reshape(h, -1), dO.reshape(g.n_src, h, -1))


def test_reference_is_the_familys_without_dropout():
    g, h, d = G.irregular_graph(8), 4, 16
    inp = G.inputs(g, h, d, seed=3, dtype=torch.float64)
    xl, xr, att, dO = _r3(g, h, inp)
    o0, stats0, dxl0, dxr0, datt0, S0, _ = G.reference(g, *inp, 0.2)
    o, m, linv = R.forward(g.src, g.dst, g.n_src, xl, xr, att, 0.2)
    tol = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(o, o0, **tol)
    torch.testing.assert_close(torch.stack([m, linv], -1), stats0, **tol)
    for x, x0 in zip(R.backward(g.src, g.dst, xl, xr, att, o, dO, 0.2), (dxl0, dxr0, datt0, S0)):
        torch.testing.assert_close(x, x0, **tol)


def test_abi_symbols_and_routing(lib):          # noqa: F811
    from custom_op_benchmark_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.graphop_abi_version() == 8
    gat = {n: _lib._SIGNATURES["graphop_gat_attention_bf16_" + n] for n in ("workspace_bytes", "forward", "backward")}
    for name, sig in gat.items():          # shaped like the GAT trio
        assert hasattr(lib, "graphop_gatv2_attention_bf16_" + name)
        assert _lib._SIGNATURES["graphop_gatv2_attention_bf16_" + name] == sig
    x = torch.zeros(2, dtype=BF)
    assert all(_lib.gatv2_attn_is_bf16("gatv2_attention" + f, x) for f in ("_forward", "_backward", "_dropout_forward",
                                                                           "_dropout_backward"))
    assert not _lib.gatv2_attn_is_bf16("gatv2_attention_dropout_forward", x, xe=x)
    assert not _lib.gatv2_attn_is_bf16("gatv2_attention_weights", x) and not _lib.gatv2_attn_is_bf16("gatv2_attention_forward", x.float())
    plan = _plan(4, 10, 4, 4)
    plan.seg_chunk = 256          # (never read on the host)
    plan.row = plan.indptr = plan.eid = plan.indices = 4096
    some = ctypes.c_void_p(4096)
    assert lib.graphop_gatv2_attention_bf16_forward(*([some] * 10), 0, 4, 10, 5, 5, 3, 8, 0.2, 0.5, 1, 0,
                                                    ctypes.byref(plan), ctypes.c_void_p(0)) == 1
    assert b"gatv2_attention_bf16_forward: bfloat16 unsupported: (h, d) = (3, 8) is not in the bfloat16 set" in lib.graphop_last_error()


@pytest.mark.parametrize("graph,kind,slope,p", [("irregular", "normal", 0.2, 0.0), ("irregular", "normal", 0.2, 0.5),
                                                ("rows", "normal", 0.2, 0.5), ("slopes", "ties", -0.3, 0.5),
                                                ("slopes", "ties", 1.0, 0.5), ("slopes", "large", 0.2, 0.5)])
def test_fp32_evaluation_uses_at_most_half_of_each_bound(graph, kind, slope, p):
    """the reference's lines in fp32 on the widened inputs, outputs rounded once to bf16, against the float64 reference on
    the GPU tier's graphs and input kinds.  Every bf16 bound is one rounding, 2**-8 |want| (which a single rounding can use
    up by itself, so no evaluation leaves half of it), plus an fp32 part: what the error exceeds the rounding's share by
    must stay within half of that fp32 part; m and 1 / l within half of the fp32 bound"""
    g = {"irregular": lambda: G.irregular_graph(8), "rows": G.edge_rows_graph, "slopes": G.slopes_graph}[graph]()
    h, d = 4, 32
    xl, xr, att, dO = _r3(g, h, tuple(x.to(BF) for x in G.inputs(g, h, d, seed=h + d, kind=kind, slope=slope)))
    mult = multipliers(g.src.numpy(), g.dst.numpy(), h, p, 1234567, 3) if p else None
    o, m, linv = R.forward(g.src, g.dst, g.n_src, xl, xr, att, slope, mult, dt=torch.float32)
    o = o.to(BF)
    dxl, dxr, datt, _ = (x.to(BF) for x in R.backward(g.src, g.dst, xl, xr, att, o, dO, slope, mult, dt=torch.float32))
    o0, m0, linv0 = R.forward(g.src, g.dst, g.n_src, xl, xr, att, slope, mult)
    dxl0, dxr0, datt0, S = R.backward(g.src, g.dst, xl, xr, att, o, dO, slope, mult)
    f32p = dict(rtol=F32["rtol"], atol=F32["atol"] / (1 - p))
    beyond = lambda x, x0, part: float(((x.double() - x0).abs() - 2 ** -8 * x0.abs()).clamp_min(0).div(part(x0)).max())
    rel = lambda x0: f32p["atol"] + f32p["rtol"] * x0.abs()
    used = {"o": beyond(o, o0, rel), "dxl": beyond(dxl, dxl0, rel), "dxr": beyond(dxr, dxr0, rel),
            "m": G.ratio(m, m0, F32), "1/l": G.ratio(linv, linv0, F32),
            "datt": beyond(datt, datt0, lambda x0: (G.K32 * S).clamp_min(1e-300))}
    assert all(v <= 0.5 for v in used.values()), used


def test_gatv2_bf16_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    fam = {}
    for name, r in kernel_resources().items():
        m = re.search(r"graphop::(k_gv2bf16_\w+)<(.*)>\(", name)
        if m:
            assert not r["spill_vgpr"] and not r["scratch"] and r["vgpr"] <= 256, (name, r)
            fam.setdefault(m.group(1), set()).add(m.group(2))
    hd = {"%d, %d" % x for x in G.FAST}
    both = {a + ", " + b for a in hd for b in ("false", "true")}
    assert fam == {"k_gv2bf16_fwd": both, "k_gv2bf16_pack": hd, "k_gv2bf16_bwd_row": both,
                   "k_gv2bf16_bwd_col": both, "k_gv2bf16_bwd_merge": hd}
