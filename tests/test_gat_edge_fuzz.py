"""GPU tier of the edge-term battery (tests/gat_edge_fuzz.py), and what test_gat_edge.py does not run: the two edge step
helpers replayed from a captured HIP graph, the raw ops on a side stream without a host synchronisation, and the
backward with the plan of one orientation NULL (a fast pack feeding one fast and one generic edge pass).

Every expected value is the float64 reference of gat_edge_fuzz.reference; the bounds are gat_edge_fuzz.bounds, none
widened.  Every used fraction of a bound is printed."""
import dataclasses

import pytest
import torch

import fused_gatv2_reference as R
import gat_edge_fuzz as G
import gat_edge_reference as E
import test_gat_edge as TE
from custom_op_benchmark_amd import _lib, functions, graphop as ops
from test_gat_fuzz import DROP, GRAD_SCALE, TOL      # (0.5, 2^40 + 3, 7); dO / 8 and rtol 1e-4 / atol 1e-5 of two fp32 runs
from test_gat_launch_geometry import _profiled
from util import random_graph

pytestmark = pytest.mark.gpu


def _check(case, got, want, what):
    """shapes and dtypes, then every output inside gat_edge_fuzz.bounds(case) of the float64 reference"""
    for name in G.OUTPUTS:
        if name == "dee" and not case.need_dee:
            continue
        x = got[name]
        assert x.dtype == case.torch_dtype and x.shape == want[name].shape, (what, name, x.dtype, x.shape)
    used = G.ratios(case, got, want)
    assert set(used) == set(G.OUTPUTS) - (set() if case.need_dee else {"dee"}), (what, sorted(used))
    print("%s: %s" % (what, "  ".join("%s %.3f" % (n, r) for n, r in used.items())))
    for name, r in used.items():
        assert r <= 1.0, "%s %s: %.3f of the bound" % (what, name, r)
    return used


# ---- 1. the battery ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(G.N_SUITE))
def test_gat_edge_fuzz(dev, seed):
    """One drawn case: shape, dtype, graph (rectangular, empty rows, hub, shuffled chunk lists, the large stratum at cpg 2
    or 3), slope, ee kind, edge numbering (permuted, row-major identity, column-major identity), dropout triple,
    need_dee, cpg knobs, force_generic, a misaligned table, binding or autograd entry with a non-contiguous output
    gradient.  The kernels are the expected ones, then the results are."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    case, built, want = G.case_data(seed, n_cu)
    what = "seed %d %s" % (seed, case)
    try:
        G.set_knobs(case)
        _lib.clear_plan_cache()
        got, names = _profiled(lambda: G.run(case, built, dev))
        names = {t: k for t, k in names.items() if t.startswith(G.TAG_PREFIX)}
        assert names == G.expected_kernels(case) and len(names) == 5, "%s\nlaunched %s" % (what, names)
        if case.large:
            knobs = _lib.tune_snapshot()
            G.assert_cpg(case, built, n_cu, knobs["sddmm_cpg"], knobs["spmm_cpg"])
        empty = torch.bincount(built.src, minlength=built.g.n_src) == 0
        assert got["o"].shape[0] == built.g.n_src and not got["o"].cpu()[empty].any(), what
        if "stats" in got:
            stats = got["stats"].cpu()
            assert stats.shape == (built.g.n_src, case.h, 2) and stats.dtype == case.torch_dtype, what
            assert bool((stats[empty][..., 0] == -1e9).all()) and not stats[empty][..., 1].any(), what
        _check(case, got, want, what)
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()


# ---- 2. HIP-graph replay of the two edge step helpers -----------------------------------------------------------------
def _fixed_case(h, d, p=0.0, seed=0, offset=0):
    """a hand-set fp32 case, so that gat_edge_fuzz.reference and gat_edge_fuzz.bounds serve the fixed tests below too"""
    return dataclasses.replace(G.draw(0), h=h, d=d, dtype="float32", slope=0.2, kind="unit", p=p,
                               philox_seed=seed if p else 0, offset=offset if p else 0, need_dee=True, large=False,
                               shuffled=False, force_generic=False, misaligned=-1, entry="ctypes",
                               grad_view="contiguous")


@pytest.mark.parametrize("p", [0.0, DROP[0]], ids=["p0", "dropout"])
@pytest.mark.parametrize("hd", [(4, 16), (3, 5)], ids=["fast", "generic"])
@pytest.mark.parametrize("step", ["fused_gat_edge_attention_step", "gat_edge_attention_step"])
def test_gat_edge_steps_replay_from_a_captured_hip_graph(dev, step, hd, p):
    """The pattern of test_gat_steps_replay_from_a_captured_hip_graph with ee a fourth leaf that requires grad: two
    warm-up steps on a side stream (they build the plans), one step captured, two replays on new values copied into the
    leaves, ee among them, and dO, each equal (up to the order of atomic adds) to an eager run of the same step, dee
    included; the first also inside the bounds of the float64 reference.  The zero fill of dee, the workspace and the
    plan look-ups are replayed, none synchronises.  Edge ids are permuted.  The composed step ends in VectorSPMM, so
    it runs on the same draw at 900 x 900."""
    h, d = hd
    composed = step == "gat_edge_attention_step"
    drop = DROP if p else (0.0, 0, 0)
    fn = getattr(functions, step)
    g0, src, dst = E.permute_edge_ids(
        random_graph(900, 900 if composed else 700, 9000, seed=4, chunk_size=32, zero_rows=0.1, hub=1100), 41)
    g = g0.to(dev)
    case = _fixed_case(h, d, *drop)
    _lib.clear_plan_cache()
    try:
        gen = torch.Generator(device=dev).manual_seed(0)
        shapes = [(g.n_src, h), (g.n_dst, h), (g.n_edges, h), (g.n_dst, h, d), (g.n_src, h, d)]
        scale = [1.0, 1.0, 1.0, 1.0, GRAD_SCALE]
        tables = [torch.randn(s, device=dev, generator=gen) * c for s, c in zip(shapes, scale)]
        leaves, dO = [t.requires_grad_(True) for t in tables[:4]], tables[4]
        run = lambda ls, grad: fn(g, *ls, grad, 0.2, *drop)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                     # warm-up: builds the plans
            for _ in range(2):
                run(leaves, dO)
        torch.cuda.current_stream().wait_stream(side)
        for t in leaves:
            t.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run(leaves, dO)
        out = tuple(out) if composed else (out,)
        outs = out + tuple(t.grad for t in leaves)
        names = (("s", "a", "o") if composed else ("o",)) + G.OUTPUTS[1:]
        for trial in range(2):
            with torch.no_grad():
                for t, c in zip(leaves + [dO], scale):
                    t.copy_(torch.randn(t.shape, device=dev, generator=gen) * c)
            graph.replay()
            torch.cuda.synchronize()
            got = [x.clone() for x in outs]
            fresh = [t.detach().clone().requires_grad_(True) for t in leaves]
            ref = run(fresh, dO.clone())
            ref = (tuple(ref) if composed else (ref,)) + tuple(t.grad for t in fresh)
            torch.cuda.synchronize()
            assert len(got) == len(ref) == len(names)
            for name, x, y in zip(names, got, ref):
                torch.testing.assert_close(x, y, **TOL, msg=lambda m: "%s trial %d %s: %s" % (step, trial, name, m))
            if trial == 0:
                built = G.EdgeBuilt(g0, g0.csr_args(), tuple(t.detach().cpu() for t in leaves), dO.cpu(), src, dst)
                want = G.reference(case, built)
                _check(case, {n: x for n, x in zip(names, got) if n in want}, want, "%s %s p=%g replay" % (step, hd, p))
    finally:
        _lib.clear_plan_cache()


# ---- 3. a side stream, no host synchronisation between the ops --------------------------------------------------------
def _edge_pairs(a8, t):
    """the edge forward + backward pair without and with dropout on the current stream -> flat list of their outputs"""
    el, er, ee, V, dO = t
    out = []
    for drop in ((), DROP):
        o, stats = ops.gat_edge_attention_forward(*a8[:4], el, er, ee, V, 0.2, *drop)
        out += [o, stats] + ops.gat_edge_attention_backward(*a8, el, er, ee, V, o, stats, dO, 0.2, *drop)
    return out


@pytest.mark.parametrize("hd", [(4, 16), (3, 5)], ids=["fast", "generic"])
def test_gat_edge_ops_on_a_side_stream_without_a_sync(dev, hd):
    """Inputs generated on a side stream and the edge pairs run there back to back, one synchronize at the end: an op
    that launched a kernel or the fill of dee on another stream would read inputs that are not written yet, or race its
    own fill.  Compared with the same calls on the default stream (the two runs differ in the order of atomic adds)."""
    h, d = hd
    g0, _, _ = E.permute_edge_ids(random_graph(600, 723, 7200, seed=91, chunk_size=32, zero_rows=0.1, hub=1100), 43)
    g = g0.to(dev)
    a8 = g.csr_args()
    for plan in (_lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst),       # (building a plan synchronises)
                 _lib.get_plan(g.col, g.ptr_c, g.eid_c, g.indices_c, g.n_src)):
        assert plan.info.row_owned and not plan.info.eid_identity
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gen = torch.Generator(device=dev).manual_seed(5)
        rn = lambda *s: torch.randn(s, device=dev, generator=gen)
        t = [rn(g.n_src, h), rn(g.n_dst, h), rn(g.n_edges, h), rn(g.n_dst, h, d), rn(g.n_src, h, d) * GRAD_SCALE]
        got = _edge_pairs(a8, t)
    side.synchronize()
    want = _edge_pairs(a8, t)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2 * 6
    for i, (x, y) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(x).all()), i
        torch.testing.assert_close(x, y, **TOL, msg=lambda m: "output %d: %s" % (i, m))


# ---- 4. the plan of one orientation NULL -------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [(4, 16), (8, 32)])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("which", ["row_only", "col_only"])
def test_gat_edge_with_one_plan_null(dev, which, p, hd):
    """The C ABI with the plan of one orientation and NULL for the other, permuted edge ids.  The rule of
    host_gat_attn_ops.h: the pack kernel is fast with either plan; stats, forward and the row pass (which writes dee)
    with the row-major one; the column pass with the column-major one.  Kernel names from the launch profile, results
    inside the bounds of the float64 reference, dee included."""
    h, d = hd
    g0, src, dst = E.permute_edge_ids(R.irregular_graph(32), 47)
    g = g0.to(dev)
    drop = (p, DROP[1], DROP[2]) if p else (0.0, 0, 0)
    case = _fixed_case(h, d, *drop)
    inp = E.inputs(src, dst, g0.n_src, g0.n_dst, h, d, torch.float32, seed=h * 100 + d)
    built = G.EdgeBuilt(g0, g0.csr_args(), tuple(inp[:4]), inp[4], src, dst)
    want = G.reference(case, built)
    row = which == "row_only"
    got, names = TE._c_abi(_lib.lib(), g, dev, h, d, [x.to(dev) for x in inp], (row, not row), drop)
    fast = G.expected_kernels(case)
    pre = G.TAG_PREFIX + ("drop_" if p else "")
    slow = [pre + "bwd_col"] if row else [G.TAG_PREFIX + "stats", pre + "fwd", pre + "bwd_row"]
    expect = {t: (k.replace("_f32", "_generic") if t in slow else k) for t, k in fast.items()}
    assert names == expect and names[G.TAG_PREFIX + "pack"] == "k_gat_attn_pack_f32", names
    _check(case, dict(zip(G.OUTPUTS, got)), want, "%s p=%g %s" % (which, p, hd))
