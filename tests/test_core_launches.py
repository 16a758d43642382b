"""GPU tier: which launches one forward and backward of each of the four function classes makes (MaskedMMCSR,
SparseSoftmax, VectorSPMM, NodeMulEdge) -- the set of (profile tag, kernel label, calls), zero fills included -- and
that they compute what the CPU oracle computes, at the bounds of tests/test_hip_parity.py.

Graph: the family's small tier, 300 x 337, 2700 edges, chunks of at most 8 slots, rows without edges, one hub row.
Each case changes what the host side decides from the arrays and their plans: the self-zeroing chunk driver (fewer
fills), the generic kernels, several heads, permuted edge ids (the plans do not cover the edge-sized outputs: more
fills), shuffled chunk lists (no row owned), forced windows, block-dense covers.  The tables were read from the profile
of the commit before a chunked CSR orientation and its plan became one value on the host side.

Also here, because they need real buffers: the NULL-array checks that stand behind an entry point's first zero fill
(tests/test_core_checks_host.py has those in front of it)."""
import dataclasses

import pytest
import torch

import oracle
from custom_op_benchmark_amd import _lib, functions, graphs
from gat_edge_reference import permute_edge_ids
from test_core_checks_host import SIGNATURES, call, csr_arrays
from test_fused_attention import force_sweep, shuffled_chunk_arrays          # noqa: F401 (force_sweep: a fixture)
from test_hip_parity import TOL, hip_step
from util import oracle_step, rand_inputs, random_graph

pytestmark = pytest.mark.gpu

SELFZERO = dict(sweep=0, walk=0, spmm_selfzero_min_mb=0)
DENSE = dict(dense_detect_min_fill=1, dense_min_fill=1)

# name -> (dtype, h, d, graph, knobs)
CASES = {
    "default": (torch.float32, 1, 64, "tier", {}),
    "selfzero": (torch.float32, 1, 64, "tier", SELFZERO),
    "fp64": (torch.float64, 1, 64, "tier", {}),
    "heads_2x32": (torch.float32, 2, 32, "tier", {}),
    "permuted_eids": (torch.float32, 1, 64, "permuted", {}),
    "shuffled_chunks": (torch.float32, 1, 64, "shuffled", {}),
    "windows": (torch.float32, 1, 64, "tier", "force_sweep"),
    "dense_blocks": (torch.float32, 1, 32, "dense", DENSE),
}

GATHER = ("sddmm_fwd", "spmm_bwd_dedata"), ("spmm_fwd", "spmm_bwd_dx", "sddmm_bwd_dA", "sddmm_bwd_dB")


def _table(zero_fills, sddmm="k_sddmm_f32", spmm="k_spmm_f32", softmax=True, nme=True):
    """{tag: (kernel label, calls)}: the zero fills of both directions, the two SDDMM-type and the four SpMM-type gather
    passes, the two softmax passes (plan-less: no tag), node_mul_edge on its own kernels or on the generic ones"""
    t = {"zero_fill": ("k_zero16", zero_fills), **{tag: (sddmm, 1) for tag in GATHER[0]},
         **{tag: (spmm, 1) for tag in GATHER[1]}}
    if softmax:
        t.update(softmax_fwd=("k_softmax_fwd_seg", 1), softmax_bwd=("k_softmax_bwd_seg", 1))
    if nme:
        t.update(node_mul_edge_fwd=("k_nme_fwd_f32", 1), node_mul_edge_bwd=("k_nme_bwd_f32", 1))
    else:
        t.update(node_mul_edge_fwd=("k_sddmm_generic", 1), node_mul_edge_bwd_dA=("k_spmm_generic", 1))
    return t


# name -> {tag: (kernel label, calls)}
TABLES = {
    "default": _table(5),
    "selfzero": _table(2),
    "fp64": _table(5, "k_sddmm_generic", "k_spmm_generic", nme=False),
    "heads_2x32": _table(5),
    "permuted_eids": _table(11),
    "shuffled_chunks": _table(13, softmax=False),
    "windows": _table(11, "k_sddmm_wown_staged_f32", "k_spmm_wown_staged_f32"),
    "dense_blocks": _table(1, "k_sddmm_block_f32", "k_spmm_block_f32"),
}


def _graph(kind):
    if kind == "dense":
        return graphs.block_diagonal_graph(7, 30, chunk_size=32)
    g = random_graph(300, 337, 2700, seed=3, chunk_size=8, zero_rows=0.2, hub=150)
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert (deg == 0).any() and deg.max() >= 150 and (g.ptr_r[1:] - g.ptr_r[:-1]).max() <= 8
    if kind == "permuted":
        g = permute_edge_ids(g, 5)[0]
        assert not torch.equal(g.eid_r, torch.arange(g.n_edges))
    elif kind == "shuffled":
        names = ("row", "ptr_r", "eid_r", "indices_r", "col", "ptr_c", "eid_c", "indices_c")
        g = dataclasses.replace(g, **dict(zip(names, shuffled_chunk_arrays(g, 1))))
        assert (g.row[1:] < g.row[:-1]).any()
    return g


def _inputs(g, h, d, dtype):
    inp = rand_inputs(g, h, d, seed=3, dtype=dtype, normal=True)
    gen = torch.Generator().manual_seed(4)
    inp["Be"] = torch.randn(g.n_edges, d, generator=gen, dtype=dtype) / d ** 0.5
    return inp


def _oracle(g, inp):
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"])
    a3 = (g.row, g.ptr_r, g.eid_r)
    want["ne_y"] = oracle.node_mul_edge_forward(*a3, inp["Q"], inp["Be"])
    want["ne_dA"], want["ne_dB"] = oracle.node_mul_edge_backward(*a3, inp["Q"], inp["Be"], inp["ge"])
    return want


def _step(g, inp):
    """one forward and backward of the four function classes"""
    got = hip_step(g, inp["Q"], inp["K"], inp["V"], inp["dO"])
    A, Be = inp["Q"].clone().requires_grad_(True), inp["Be"].clone().requires_grad_(True)
    y = functions.NodeMulEdge.apply(g.row, g.ptr_r, g.eid_r, A, Be)
    y.backward(inp["ge"])
    torch.cuda.synchronize()
    got.update(ne_y=y.detach(), ne_dA=A.grad, ne_dB=Be.grad)
    return got


def _run(dev, name):
    """-> (the launches of one profiled step, its results, the oracle's); the case's knobs are set and reset here"""
    dtype, h, d, kind, knobs = CASES[name]
    g = _graph(kind)
    inp = _inputs(g, h, d, dtype)
    want = _oracle(g, inp)
    gd, inpd = g.to(dev), {k: v.to(dev) for k, v in inp.items()}
    for knob, v in (knobs if isinstance(knobs, dict) else {}).items():
        _lib.tune(knob, v)
    _lib.clear_plan_cache()
    try:
        _step(gd, inpd)                                  # the plans and their layouts are built here
        _lib.profile_enable(True)
        try:
            got = _step(gd, inpd)
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()
    return {tag: (r["kernel"], r["calls"]) for tag, r in prof.items()}, got, want


@pytest.mark.parametrize("name", list(CASES))
def test_launches_and_results(dev, request, name):
    if CASES[name][4] == "force_sweep":
        request.getfixturevalue("force_sweep")
    seen, got, want = _run(dev, name)
    print(name, sorted(seen.items()))
    for k in ("s", "a", "o", "dQ", "dK", "dV", "ne_y", "ne_dA", "ne_dB"):
        torch.testing.assert_close(got[k].cpu(), want[k], **TOL[CASES[name][0]],
                                   msg=lambda m, k=k: "%s %s: %s" % (name, k, m))
    assert seen == TABLES[name]


# ---- the NULL-array checks behind a zero fill ---------------------------------------------------------------------
SIZES = dict(n_chunks=4, n_row_chunks=4, n_col_chunks=4, n_edges=10, n_a=5, n_b=5, n_x=5, n_y=5, n_dy=5, n_l=5, n_r=5,
             n_q=5, n_k=5, h=1, d=8, workspace_rows=5)
BEHIND_A_FILL = ("maskedmm_csr_forward", "vector_spmm_forward", "vector_spmm_backward", "node_mul_edge_forward",
                 "gat_scores_forward", "gat_scores_backward", "gatv2_scores_forward", "gatv2_scores_backward",
                 "attention_forward", "attention_backward")
# the composed attention ops (no plan) report the array under the name the entry point they call gives it
NESTED = {"attention_forward": {a: "maskedmm_csr_forward: %s is NULL" % a for a in ("row", "indptr", "eid", "indices")},
          "attention_backward": {**{a + s: "maskedmm_csr_forward: %s is NULL" % a
                                    for a, s in (("row", ""), ("indptr", "_r"), ("eid", "_r"), ("indices", "_r"))},
                                 **{a + s: "vector_spmm_backward: %s is NULL" % (a + t)
                                    for a, s, t in (("col", "", ""), ("indptr", "_c", "_t"), ("eid", "_c", "_t"),
                                                    ("indices", "_c", "_t"))}}}


def _sizes(name):
    return {n: SIZES[n] for n, kind in SIGNATURES[name] if kind == "i" and n != "workspace_bytes"}


@pytest.mark.parametrize("name", BEHIND_A_FILL)
def test_a_null_csr_array_behind_a_zero_fill_is_named(dev, name):
    """the CSR arrays are one zeroed buffer (empty chunks of row 0) that nothing writes, the operands and outputs a
    second, the workspace a third; one CSR array is NULL"""
    l = _lib.lib()
    arrays, data, ws = (torch.zeros(1 << 14, dtype=torch.int64, device=dev) for _ in range(3))
    ptr = {None: data.data_ptr(), "workspace": ws.data_ptr(), **{a: arrays.data_ptr() for a in csr_arrays(name)}}
    for dtype in (0, 1):
        for a in csr_arrays(name):
            rc, msg = call(l, name, dtype=dtype, null=(a,), ptr=ptr, ws_bytes=ws.numel() * 8, **_sizes(name))
            want = NESTED.get(name, {}).get(a, "%s: %s is NULL" % (name, a))
            assert rc == 1 and msg == want.encode(), (name, a, rc, msg)
    torch.cuda.synchronize()
    assert not arrays.any()


@pytest.mark.parametrize("name,out_items", [("maskedmm_csr_forward", 10), ("sparse_softmax_forward", 10),
                                            ("vector_spmm_forward", 40), ("node_mul_edge_forward", 10)])
def test_no_chunks_accepts_null_arrays_and_zero_fills(dev, name, out_items):
    """n_chunks == 0 with n_edges > 0: the arrays may be NULL, the output is zero-filled, nothing else is written"""
    l = _lib.lib()
    buf = torch.ones(1024, dtype=torch.float32, device=dev)
    sizes = {**_sizes(name), "n_chunks": 0}
    assert call(l, name, null=csr_arrays(name), ptr=buf.data_ptr(), **sizes) == (0, b"")
    torch.cuda.synchronize()
    assert not buf[:out_items].any() and bool((buf[out_items:] == 1).all())
