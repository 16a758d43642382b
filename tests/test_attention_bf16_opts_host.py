"""CPU tier of the bfloat16 fused attention step with dropout and a score bias (kernels_attn_bf16_opts.h, DESIGN.md
4.5w): the workspace query answers the plain bf16 step's sums, empty problems touch nothing, every refusal is named, the
new kernels stay out of scratch, and the GPU tier's bounds leave an fp32 evaluation room."""
import ctypes
import os
import re
import sys

import pytest
import torch

import attention_bf16_opts_reference as R
from gat_edge_reference import permute_edge_ids
from test_attention_bf16_host import BF16, HD, QUERY, _plan, lib          # noqa: F401 (fixture)
from test_attention_heads_host import _query
from util import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, dict(rtol=1e-4, atol=1e-5)          # (TOL[torch.float32] of test_fused_attention.py)
NULL, SOME = ctypes.c_void_p(0), ctypes.c_void_p(4096)


def _fwd(lib, h, d, plan=NULL, p=0.5, head0=0, ptr=SOME, sizes=(4, 10, 5, 5)):          # noqa: F811
    return lib.graphop_attention_bf16_opts_forward(*([ptr] * 10), *sizes, h, d, NULL, 0, plan, NULL, p, 1, 0, head0)


def test_workspace_query_answers_the_plain_sums(lib):          # noqa: F811
    E, C, n_q, n_k = 1000, 100, 50, 40
    pr, pc = _plan(C, E, n_q - 1, n_k - 1), _plan(C + 7, E, n_k - 1, n_q - 1)
    for h, d in ((4, 16), (8, 64), (3, 8)):
        for backward in (0, 1):
            want = _query(lib, QUERY, backward, E, n_q, n_k, h, d, pr, pc, dtype=BF16)
            assert (want > 0) == ((h, d) != (3, 8))
            for with_db in (0, 1):
                out = ctypes.c_int64(-1)
                assert lib.graphop_attention_bf16_opts_workspace_bytes(backward, E, n_q, n_k, h, d, ctypes.byref(pr),
                                                                       ctypes.byref(pc), NULL, with_db, ctypes.byref(out)) == 0
                assert out.value == want, (h, d, backward, with_db)


def test_empty_problems_touch_nothing_and_refusals_are_named(lib):          # noqa: F811
    for h, d in ((4, 16), (8, 64)):
        assert _fwd(lib, h, d, ptr=NULL, sizes=(0, 0, 0, 7)) == 0
        assert lib.graphop_attention_bf16_opts_backward(*([NULL] * 19), 0, 0, 0, 0, 0, h, d, NULL, 0, NULL, NULL, NULL, 0.5, 1,
                                                        0, 0) == 0
    for kw, message in ((dict(p=1.0), b"dropout probability p must be in [0, 1)"),
                        (dict(head0=2 ** 31 - 4), b"head0 + h < 2^31"),
                        (dict(), b"attention_bf16_opts_forward: bfloat16 unsupported: plan is NULL"),
                        (dict(h=3, d=8), b"(h, d) = (3, 8) is not in the bfloat16 set")):
        assert _fwd(lib, kw.pop("h", 4), kw.pop("d", 16), **kw) == 1
        assert message in lib.graphop_last_error(), lib.graphop_last_error()
    ptrs = [SOME] * 19
    ptrs[11] = NULL          # b, with db given
    assert lib.graphop_attention_bf16_opts_backward(*ptrs, 4, 4, 10, 5, 5, 4, 16, NULL, 0, NULL, NULL, NULL, 0.0, 1, 0, 0) == 1
    assert b"attention_bf16_opts_backward: db given without b" in lib.graphop_last_error()


def test_new_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    fam = {}
    for name, r in kernel_resources().items():
        m = re.search(r"graphop::(k_attnopt_bf16_\w+)<(.*)>\(", name)
        if m:
            assert not r["spill_vgpr"] and not r["scratch"] and r["vgpr"] <= 256, (name, r)
            fam.setdefault(m.group(1), set()).add(m.group(2))
    hd = ["%d, %d" % x for x in HD]
    opts = ("true, false", "false, true", "true, true")          # (DROP, BIAS): neither is the plain kernel
    fwd = {a + ", " + o for a in hd for o in opts}
    bwd = {"%s, %s, %s, false" % (a, col, o) for a in hd for col in ("false", "true") for o in opts}
    bwd |= {a + ", false, " + o + ", true" for a in hd for o in opts[1:]}          # db: the row pass with a bias
    assert fam == {"k_attnopt_bf16_fwd_rows": fwd, "k_attnopt_bf16_bwd_rows": bwd}


@pytest.mark.parametrize("mode", ["dropout", "bias", "both"])
@pytest.mark.parametrize("h,d", [(4, 16), (8, 32), (8, 64)])          # NV = 1, 2, 4
def test_fp32_evaluation_uses_at_most_half_of_each_bound(h, d, mode):
    """The rule of test_gatv2_attention_bf16_host.py on the inputs of the GPU tier's first test: the reference's lines in
    fp32 on the widened inputs, outputs rounded once to bf16, against the float64 reference.  Every bf16 bound is one
    rounding, 2**-8 |want|, plus the fp32 TOL: what the error exceeds the rounding's share by must stay within half of the
    fp32 part, for o, dQ, dK, dV and db; m and 1 / l within half of the fp32 bound.  The inputs are the GPU tier's
    unchanged: nothing had to be rescaled."""
    p, biased = {"dropout": (0.5, False), "bias": (0.0, True), "both": (0.5, True)}[mode]
    g, src, dst = permute_edge_ids(random_graph(300, 337, 2700, seed=3, chunk_size=8, zero_rows=0.2, hub=150), seed=5)
    gen = torch.Generator().manual_seed(h * 100 + d)
    Q, K, V, dO = ((torch.randn(n, h, d, generator=gen) / d ** 0.5).to(BF) for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))
    b = torch.randn(g.n_edges, h, generator=torch.Generator().manual_seed(h + d)).to(BF) if biased else None
    mult = R.multipliers(src, dst, h, p, 2 ** 40 + 12345, 7)
    f32 = torch.float32
    o, m, linv, _ = R.forward(src, dst, g.n_src, Q, K, V, b, mult, dtype=f32)
    o = o.to(BF)
    got = [x.to(BF) for x in R.backward(src, dst, Q, K, V, o, dO, b, mult, dtype=f32)]
    o0, m0, linv0, _ = R.forward(src, dst, g.n_src, Q, K, V, b, mult)
    want = R.backward(src, dst, Q, K, V, o, dO, b, mult)
    beyond = lambda x, x0: float(((x.double() - x0).abs() - 2 ** -8 * x0.abs()).clamp_min(0)
                                 .div(F32["atol"] + F32["rtol"] * x0.abs()).max())
    ratio = lambda x, x0: float(((x.double() - x0).abs() / (F32["atol"] + F32["rtol"] * x0.abs())).max())
    live = torch.bincount(src, minlength=g.n_src) > 0
    used = {"o": beyond(o, o0), "m": ratio(m[live], m0[live]), "1/l": ratio(linv, linv0)}
    used.update({n: beyond(x, x0) for n, x, x0 in zip(("dQ", "dK", "dV", "db")[:4 if biased else 3], got, want)})
    print(used)
    assert all(v <= 0.5 for v in used.values()), used
