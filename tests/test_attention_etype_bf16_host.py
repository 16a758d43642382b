"""CPU tier of the bfloat16 fused attention step with edge-type embeddings (kernels_attn_etype_bf16.h):
empty problems touch nothing, every refusal is named in the stated order, the workspace is the plain bf16 step's plus the
bounded partial tables, the ops are bound and not registered, the set of k_etype_bf16_* instantiations is exact, out of
scratch and within 256 VGPRs, and the GPU tier's bounds leave an fp32 evaluation room."""
import ctypes
import os
import re
import sys

import pytest
import torch

import attention_edge_bf16_reference as R
from gat_edge_reference import permute_edge_ids
from test_attention_bf16_host import HD, _plan, lib          # noqa: F401 (fixture)
from util import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, dict(rtol=1e-4, atol=1e-5)          # (TOL[torch.float32] of test_fused_attention.py)
NULL, SOME = ctypes.c_void_p(0), ctypes.c_void_p(4096)


def _fwd(lib, h, d, T=5, plan=NULL, ptr=SOME, sizes=(4, 10, 5, 5), p=0.5, head0=0):          # noqa: F811
    return lib.graphop_attention_etype_bf16_forward(*([ptr] * 11), *sizes, h, d, T, NULL, 0, plan, NULL, p, 1, 0, head0)


def test_empty_problems_touch_nothing_and_refusals_are_named(lib):          # noqa: F811
    from custom_op_benchmark_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.graphop_abi_version() == 8
    for h, d in ((4, 16), (8, 64)):
        assert _fwd(lib, h, d, T=0, ptr=NULL, sizes=(0, 0, 0, 7)) == 0
        assert lib.graphop_attention_etype_bf16_backward(*([NULL] * 20), 0, 0, 0, 0, 0, h, d, 0, NULL, 0, NULL, NULL, NULL,
                                                         0.5, 1, 0, 0) == 0
    # each call breaks its own condition and every later one: the earliest is the one named
    for kw, message in ((dict(p=1.0, head0=-1, T=0), b"dropout probability p must be in [0, 1)"),
                        (dict(head0=-1, T=0), b"head0 >= 0 and head0 + h < 2^31 wanted"),
                        (dict(T=0, h=3, d=8), b"n_types must be >= 1 with n_edges > 0"),
                        (dict(T=171, h=3, d=8), b"bfloat16 unsupported: n_types * h * d = 4104 is above 4096"),
                        (dict(h=3, d=8), b"(h, d) = (3, 8) is not in the bfloat16 set"),
                        (dict(), b"attention_etype_bf16_forward: bfloat16 unsupported: plan is NULL")):
        assert _fwd(lib, kw.pop("h", 4), kw.pop("d", 16), **kw) == 1
        assert message in lib.graphop_last_error(), lib.graphop_last_error()
    assert _fwd(lib, 8, 8, T=65) == 1 and b"attention_edge_bf16_* on the gathered rows" in lib.graphop_last_error()
    assert lib.graphop_attention_etype_bf16_backward(*([SOME] * 20), 4, 4, 10, 5, 5, 8, 32, 17, NULL, 0, NULL, NULL, NULL,
                                                     0.0, 1, 0, 0) == 1
    assert b"attention_etype_bf16_backward: bfloat16 unsupported: n_types * h * d = 4352" in lib.graphop_last_error()
    # the query: the plain step's bytes in the forward, plus the partial tables in the backward, 0 where a call would refuse
    E, C, n_q, n_k = 1000, 100, 50, 40
    pr, pc = _plan(C, E, n_q - 1, n_k - 1), _plan(C + 7, E, n_k - 1, n_q - 1)
    out, plain = ctypes.c_int64(-1), ctypes.c_int64(-1)
    query = lambda backward, h, d, T, a, b: lib.graphop_attention_etype_bf16_workspace_bytes(
        backward, E, n_q, n_k, h, d, T, a, b, NULL, ctypes.byref(out))
    for backward in (0, 1):          # 100 chunks of 8-lane groups, one chunk each: ceil(100 / 32) = 4 workgroups, T F = 320 words
        assert lib.graphop_attention_bf16_opts_workspace_bytes(backward, E, n_q, n_k, 4, 16, ctypes.byref(pr), ctypes.byref(pc),
                                                               NULL, 0, ctypes.byref(plain)) == 0
        assert query(backward, 4, 16, 5, ctypes.byref(pr), ctypes.byref(pc)) == 0
        assert out.value == plain.value + backward * 4 * 1280 and plain.value > 0
        assert query(backward, 4, 16, 65, ctypes.byref(pr), ctypes.byref(pc)) == 0 and out.value == 0
        assert query(backward, 3, 8, 5, ctypes.byref(pr), ctypes.byref(pc)) == 0 and out.value == 0
        assert query(backward, 4, 16, 5, NULL, NULL) == 0 and out.value == 0
    unowned = _plan(C, E, n_q - 1, n_k - 1, row_owned=0)
    assert query(0, 4, 16, 5, ctypes.byref(unowned), NULL) == 0 and out.value == 0
    # a plan whose row pass would have more workgroups than kEtypeBf16Parts: 1024 partial tables and no more
    many = _plan(2 ** 22, 2 ** 23, n_q - 1, n_k - 1)
    assert lib.graphop_attention_bf16_opts_workspace_bytes(1, 2 ** 23, n_q, n_k, 4, 16, ctypes.byref(many), ctypes.byref(pc),
                                                           NULL, 0, ctypes.byref(plain)) == 0
    assert lib.graphop_attention_etype_bf16_workspace_bytes(1, 2 ** 23, n_q, n_k, 4, 16, 5, ctypes.byref(many), ctypes.byref(pc),
                                                            NULL, ctypes.byref(out)) == 0
    assert out.value == plain.value + 1024 * 1280


def test_ops_are_bound_and_not_registered():
    from custom_op_benchmark_amd import graphop
    for name in ("attention_etype_bf16_forward", "attention_etype_bf16_backward"):
        assert name in graphop.EXTRA_OPS and name not in graphop._SCHEMAS and name not in graphop.__all__
        assert callable(getattr(graphop, name)) and not hasattr(torch.ops.graphop, name)
        assert graphop.cpp_ext is None or hasattr(graphop.cpp_ext, name)


def test_instantiation_set_is_exact_and_out_of_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    fam = {}
    for name, r in kernel_resources().items():
        m = re.search(r"graphop::(k_etype_bf16_\w+)(?:<(.*)>)?\(", name)
        if m:
            assert not r["spill_vgpr"] and not r["scratch"] and r["vgpr"] <= 256, (name, r)
            fam.setdefault(m.group(1), set()).add(m.group(2))
    hd = ["%d, %d" % x for x in HD]
    tf = ("false", "true")
    fwd = {"%s, %s" % (a, drop) for a in hd for drop in tf}
    bwd = {"%s, %s, %s, false" % (a, col, drop) for a in hd for col in tf for drop in tf}
    bwd |= {"%s, false, %s, true" % (a, drop) for a in hd for drop in tf}          # dR: the row pass alone
    assert fam == {"k_etype_bf16_fwd_rows": fwd, "k_etype_bf16_bwd_rows": bwd, "k_etype_bf16_dr_reduce": {None}}


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,d", [(4, 16), (8, 32), (8, 64)])          # NV = 1, 2, 4
def test_fp32_evaluation_uses_at_most_half_of_each_bound(h, d, p):
    """The rule of test_attention_tbias_bf16_host.py's last test on the inputs of the GPU tier's first test: the
    reference's lines in fp32 on the widened inputs, outputs rounded once to bf16 (dR: index_add in fp32, then one
    rounding), against the float64 reference.  What the error exceeds the one rounding's share 2**-8 |want| by must stay
    within half of the fp32 part of the bound -- for dR that part is atol sqrt(n_max) + rtol |want|."""
    T = 5
    g, src, dst = permute_edge_ids(random_graph(300, 337, 2700, seed=3, chunk_size=8, zero_rows=0.2, hub=150), seed=5)
    gen = torch.Generator().manual_seed(h * 100 + d)
    Q, K, V, dO = ((torch.randn(n, h, d, generator=gen) / d ** 0.5).to(BF) for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))
    gen = torch.Generator().manual_seed(h + d)
    Rt = torch.randn(T, h, d, generator=gen).to(BF)
    et = torch.randint(0, T, (g.n_edges,), generator=gen, dtype=torch.int32).long()
    mult = R.multipliers(src, dst, h, p, 2 ** 40 + 12345, 7)
    f32 = torch.float32
    o, m, linv = R.forward(src, dst, g.n_src, Q, K, V, Rt.float()[et], mult, dtype=f32)
    o = o.to(BF)
    got = list(R.backward(src, dst, Q, K, V, Rt.float()[et], o, dO, mult, dtype=f32))
    got[3] = torch.zeros(T, h, d).index_add_(0, et, got[3])
    o0, m0, linv0 = R.forward(src, dst, g.n_src, Q, K, V, Rt.double()[et], mult)
    want = list(R.backward(src, dst, Q, K, V, Rt.double()[et], o, dO, mult))
    want[3] = torch.zeros(T, h, d, dtype=torch.float64).index_add_(0, et, want[3])
    n_max = float(torch.bincount(et).max())

    def beyond(x, x0, atol=F32["atol"]):
        return float(((x.to(BF).double() - x0).abs() - 2 ** -8 * x0.abs()).clamp_min(0).div(atol + F32["rtol"] * x0.abs()).max())
    ratio = lambda x, x0: float(((x.double() - x0).abs() / (F32["atol"] + F32["rtol"] * x0.abs())).max())
    live = torch.bincount(src, minlength=g.n_src) > 0
    used = {"o": beyond(o, o0), "m": ratio(m[live], m0[live]), "1/l": ratio(linv, linv0)}
    used.update({n: beyond(x, x0) for n, x, x0 in zip(("dQ", "dK", "dV"), got, want)})
    used["dR"] = beyond(got[3], want[3], F32["atol"] * n_max ** 0.5)
    print(used)
    assert all(v <= 0.5 for v in used.values()), used
