"""GPU tier of the guard (tests/guarded.py): every op of the ctypes binding run into poisoned, guard-banded
outputs and workspaces, on float operands between NaN bands, with its plans built in guard-banded, poisoned plan memory.

Every test: (1) makes the call unguarded for its launch profile, (2) builds the plans again inside guarded_plan_memory() and
runs the same call inside guarded_ops(), (3) asserts no band byte changed, no NaN is left in a returned output and the
inputs are bitwise what they were, (4) asserts the guarded launch profile {tag: kernel} is the unguarded one, (5) holds the
results to the bound the case has in its own module, unchanged, and (6) puts knobs, plan cache and allocator back.

The batteries' cases run through the ctypes entry (the C++ bindings allocate in C++).  The core step is the six raw calls
the autograd classes of hip_step make (functions.MaskedMMCSR / SparseSoftmax / VectorSPMM are thin wrappers), so that the
operands keep their bands -- hip_step clones them -- and da and ds are returned outputs under the NaN rule too."""
import dataclasses
import functools

import pytest
import torch

import attention_edge_reference as AE
import attention_fuzz as AF
import attention_tbias_reference as T
import dropout_reference as DR
import gat_edge_fuzz as GEF
import gat_edge_reference as GE
import gat_fuzz as GF
import gat_weights_reference as W
import gatv2_edge_reference as G2
import guarded as G
import oracle
import test_attention_fuzz as TAF
import test_gat_edge_fuzz as TGE
import test_gat_fuzz as TGF
import test_hip_parity as HP
from custom_op_benchmark_amd import _lib, graphs, graphop as ops
from test_gat_launch_geometry import _profiled
from util import rand_inputs

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TOTALS = {"calls": 0, "allocations": 0, "bytes": 0}


def _under_guard(call, inputs, what):
    """steps 1 to 4 of the module docstring -> (what call() returned under the guard, its launch profile)"""
    _lib.clear_plan_cache()
    _, before = _profiled(call)
    snap = G.snapshot(inputs)
    with G.guarded_plan_memory() as damage:
        with G.guarded_ops() as guard:
            got, during = _profiled(call)
            bad = guard.violations(got)
        changed = G.unchanged(snap)
    assert ops.torch is torch
    TOTALS["calls"] += 1
    TOTALS["allocations"] += len(guard.records)
    TOTALS["bytes"] += guard.guarded_bytes()
    print("%s: %d allocations, %d bytes under guard" % (what, len(guard.records), guard.guarded_bytes()))
    assert not bad, "%s\n%s" % (what, "\n".join(bad))
    assert not damage, "%s\n%s" % (what, "\n".join(damage))
    assert not changed, "%s\n%s" % (what, "\n".join(changed))
    assert guard.records, what
    assert during == before, "%s: the guard moved the call to other kernels\nunguarded %s\nguarded   %s" % (what, before, during)
    return got, during


def _reset():
    _lib.profile_enable(False)
    _lib.tune_reset()
    _lib.clear_plan_cache()


# ---- 1. the three batteries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(GF.N_SUITE))
def test_gat_family_under_guard(dev, seed):
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    case, built, want = GF.case_data(seed, n_cu)
    case = G.ctypes_entry(case)
    what = "gat seed %d %s" % (seed, case)
    on_dev = dataclasses.replace(built, csr=tuple(x.to(dev) for x in built.csr),
                                 inputs=tuple(G.banded(t, dev) for t in built.inputs), grad=G.banded(built.grad, dev))
    try:
        GF.set_knobs(case)
        got, names = _under_guard(lambda: GF.run(case, on_dev, dev), [on_dev.csr, on_dev.inputs, on_dev.grad], what)
        names = {t: k for t, k in names.items() if t.startswith(GF.TAG_PREFIX[case.family])}
        assert names == GF.expected_kernels(case), "%s\nlaunched %s" % (what, names)
        TGF._check(case, got, want, what)
    finally:
        _reset()


@pytest.mark.parametrize("seed", range(GEF.N_SUITE))
def test_gat_edge_family_under_guard(dev, seed):
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    case, built, want = GEF.case_data(seed, n_cu)
    case = G.ctypes_entry(case)
    what = "gat_edge seed %d %s" % (seed, case)
    on_dev = dataclasses.replace(built, csr=tuple(x.to(dev) for x in built.csr),
                                 inputs=tuple(G.banded(t, dev) for t in built.inputs), grad=G.banded(built.grad, dev))
    try:
        GEF.set_knobs(case)
        got, names = _under_guard(lambda: GEF.run(case, on_dev, dev), [on_dev.csr, on_dev.inputs, on_dev.grad], what)
        names = {t: k for t, k in names.items() if t.startswith(GEF.TAG_PREFIX)}
        assert names == GEF.expected_kernels(case), "%s\nlaunched %s" % (what, names)
        TGE._check(case, got, want, what)
    finally:
        _reset()


@functools.lru_cache(maxsize=None)
def _attention_case(seed, n_cu):
    """(case through the ctypes entry, built, float64 reference).  The raw ops take no gradient of `a`: a weights case
    drawn with ga (behind the autograd entry, its loss <o, dO> + <a, ga> or <a, ga> alone) runs here with the loss
    <o, dO>, and its reference is attention_fuzz.reference of that case on the same graph and operands."""
    case, built, want = AF.case_data(seed, n_cu)
    case = G.ctypes_entry(case)
    if case.ga:
        case = dataclasses.replace(case, ga=False, dO=True)
        built = dataclasses.replace(built, t={k: v for k, v in built.t.items() if k != "ga"})
        want = AF.reference(case, built)
    return case, built, want


@pytest.mark.parametrize("seed", range(AF.N_SUITE))
def test_attention_family_under_guard(dev, seed):
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    case, built, want = _attention_case(seed, n_cu)
    what = "attention seed %d %s" % (seed, case)
    on_dev = dataclasses.replace(built, csr=tuple(x.to(dev) for x in built.csr),
                                 t={k: G.banded(v, dev) for k, v in built.t.items()})
    try:
        AF.set_knobs(case)
        got, profile = _under_guard(lambda: AF.run(case, on_dev, dev), [on_dev.csr, on_dev.t], what)
        seen, forms = AF.seen_forms(profile), AF.expected_forms(case, built)
        assert len([f for f in forms if f.tags == seen]) == 1, "%s\nlaunched %s" % (what, seen)
        TAF._check(case, got, want, built, what)
    finally:
        _reset()


# ---- 2. the core step ------------------------------------------------------------------------------------------------------------
STEP_KEYS = ("s", "a", "o", "da", "dV", "ds", "dQ", "dK")


def _raw_step(a8, Q, K, V, dO):
    """the six calls of hip_step's autograd classes, in its order"""
    s = ops.maskedmm_csr_forward(*a8[:4], Q, K)
    a = ops.sparse_softmax_forward(*a8[:3], s)
    o = ops.vector_spmm_forward(*a8[:4], a, V)
    da, dV = ops.vector_spmm_backward(*a8, a, dO, V)
    ds = ops.sparse_softmax_backward(*a8[:3], a, da)
    dQ, dK = ops.maskedmm_csr_backward(*a8, Q, K, ds)
    return dict(s=s, a=a, o=o, da=da, dV=dV, ds=ds, dQ=dQ, dK=dK)


def _oracle_step(a8, Q, K, V, dO):
    """util.oracle_step on eight index arrays"""
    s = oracle.maskedmm_csr_forward(*a8[:4], Q, K)
    a = oracle.sparse_softmax_forward(*a8[:3], s)
    o = oracle.vector_spmm_forward(*a8[:4], a, V)
    da, dV = oracle.vector_spmm_backward(*a8, a, dO, V)
    ds = oracle.sparse_softmax_backward(*a8[:3], a, da)
    dQ, dK = oracle.maskedmm_csr_backward(*a8, Q, K, ds)
    return dict(s=s, a=a, o=o, da=da, dV=dV, ds=ds, dQ=dQ, dK=dK)


def _guarded_step(dev, a8, inp, what, dtype=F32, **tol):
    """the step on banded operands under the guard, every one of its eight results against the oracle at close()'s
    bound for `dtype` (or the case's own, in tol) -> the launch profile"""
    args = tuple(inp[k] for k in ("Q", "K", "V", "dO"))
    want = _oracle_step(a8, *args)
    a8d = tuple(x.to(dev) for x in a8)
    on_dev = tuple(G.banded(x, dev) for x in args)
    got, profile = _under_guard(lambda: _raw_step(a8d, *on_dev), [a8d, on_dev], what)
    for k in STEP_KEYS:
        HP.close(got[k], want[k], dtype, **tol)
    return profile


@pytest.mark.parametrize("seed", range(48))
def test_core_fuzz_under_guard(dev, seed):
    """test_hip_parity.fuzz_case(seed): 40 to 700 rows, every forced driver, the tile seeds 40 to 47; at the battery's bound"""
    shape, knobs, tile = HP.fuzz_case(seed)
    g = G.core_fuzz_graph(seed)
    try:
        for key, value in knobs.items():
            _lib.tune(key, value)
        inp = rand_inputs(g, shape["h"], shape["d"], seed=seed + 50, normal=True)
        kern = _guarded_step(dev, g.csr_args(), inp, "core seed %d %s %s" % (seed, shape, knobs), rtol=2e-4, atol=2e-5)
        if tile:
            assert kern.get("sddmm_fwd") == "k_sddmm_tile_f32" and kern.get("spmm_bwd_dedata") == "k_sddmm_tile_f32", kern
    finally:
        _reset()


@pytest.mark.parametrize("h,d", [(1, 64), (4, 16), (3, 5)])
def test_core_fp64_under_guard(dev, h, d):
    """the shapes of test_step_vs_oracle_fp64"""
    g = G.fp64_graph(d)
    try:
        inp = rand_inputs(g, h, d, seed=4, dtype=F64, normal=True)
        _guarded_step(dev, g.csr_args(), inp, "fp64 %d x %d" % (h, d), F64)
    finally:
        _reset()


def test_core_fp64_walk_and_staged_strip_under_guard(dev):
    """test_fp64_on_the_walk_and_window_drivers_vs_oracle at d = 32, walk_blocks = 8: 1,500 rows"""
    try:
        for key, value in (("sweep_min_kb", 0), ("walk_window_kb", 8), ("walk_window_kb_col", 8), ("walk_min_bin", 0),
                           ("sweep_min_granule", 0), ("max_windows", 512), ("walk", 6), ("walk_blocks", 8),
                           ("window_kb", 8), ("vrow_t", 64)):
            _lib.tune(key, value)
        g = G.walk_graph()
        inp = rand_inputs(g, 1, 32, seed=8, dtype=F64, normal=True)
        kern = _guarded_step(dev, g.csr_args(), inp, "fp64 walk", F64)
        assert kern["sddmm_fwd"] == kern["spmm_bwd_dedata"] == "k_sddmm_wown_staged_f64", kern
        assert all(kern[t] == "k_spmm_walk_f64" for t in ("spmm_fwd", "spmm_bwd_dx", "sddmm_bwd_dA", "sddmm_bwd_dB")), kern
    finally:
        _reset()


@pytest.mark.parametrize("l,h,d", [(30, 8, 64), (5, 1, 8)])
def test_core_block_dense_under_guard(dev, l, h, d):
    """block_diagonal_graph(7, l) under the knobs of test_block_dense_drivers_vs_oracle: the MFMA drivers"""
    g = graphs.block_diagonal_graph(7, l, chunk_size=32)
    try:
        _lib.tune("dense_detect_min_fill", 1); _lib.tune("dense_min_fill", 1)
        inp = rand_inputs(g, h, d, seed=l + d, normal=True)
        _guarded_step(dev, g.csr_args(), inp, "block dense l=%d %d x %d" % (l, h, d))
        gd = g.to(dev)
        for p in HP._plans(gd):
            assert p.info.n_dense_blocks == 7
        del p, gd
    finally:
        _reset()


def test_core_shuffled_chunks_under_guard(dev):
    """the general path of test_unordered_chunks_take_the_general_path at (8, 16): no row is owned, every pass adds by atomics
    into rows it has to clear first, and the softmax takes a workspace"""
    g, a8 = G.shuffled_graph()
    try:
        inp = rand_inputs(g, 8, 16, seed=6, normal=True)
        _guarded_step(dev, a8, inp, "shuffled chunks 8 x 16")
        a4 = tuple(x.to(dev) for x in a8[:4])
        info = _lib.get_plan(*a4, n_index_bound=g.n_dst).info
        assert info.row_owned == 0 and info.rows_sorted == 0
        del a4
    finally:
        _reset()


# ---- 3. softmax alone ------------------------------------------------------------------------------------------------------------
def _softmax_case(dev, g, h, gen, what):
    es = (g.n_edges,) if h == 1 else (g.n_edges, h)
    x = torch.randn(es, generator=gen) * 3
    ge = torch.randn(es, generator=gen)
    for side, a3 in (("rows", (g.row, g.ptr_r, g.eid_r)), ("columns", (g.col, g.ptr_c, g.eid_c))):
        yo = oracle.sparse_softmax_forward(*a3, x)
        dxo = oracle.sparse_softmax_backward(*a3, yo, ge)
        a3d = tuple(v.to(dev) for v in a3)
        xd, ged = G.banded(x, dev), G.banded(ge, dev)

        def call():
            y = ops.sparse_softmax_forward(*a3d, xd)
            return dict(y=y, dx=ops.sparse_softmax_backward(*a3d, y, ged))
        got, kern = _under_guard(call, [a3d, xd, ged], "%s %s h=%d" % (what, side, h))
        HP.close(got["y"], yo)
        HP.close(got["dx"], dxo, rtol=1e-3, atol=1e-6)          # (the bound of the two softmax tests of test_hip_parity.py)
        yield side, kern


@pytest.mark.parametrize("h", [1, 4])
def test_softmax_long_rows_under_guard(dev, h):
    """the graph of test_softmax_long_rows_and_cached_rows: 400 rows, one hub above 8,192 slots"""
    try:
        g = G.softmax_hub_graph(h)
        assert int(torch.bincount(g.src).max()) > 8192
        list(_softmax_case(dev, g, h, torch.Generator().manual_seed(3), "softmax hub"))
    finally:
        _reset()


@pytest.mark.parametrize("h", [4, 8])
def test_softmax_float4_items_under_guard(dev, h):
    """the length list of test_softmax_several_heads_float4_items: the float4 kernels row-major, the scalar ones column-major"""
    try:
        g, gen = G.softmax_lengths_graph(h)
        for side, kern in _softmax_case(dev, g, h, gen, "softmax float4"):
            ran = {k for k in kern.values() if "softmax" in k}
            want = "vec4" if side == "rows" else "seg"
            assert ran == {"k_softmax_fwd_" + want, "k_softmax_bwd_" + want}, (side, ran)
    finally:
        _reset()


# ---- 4. ops outside the batteries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,d", [(1, 64), (8, 64), (2, 5), (3, 64)])
def test_node_mul_edge_under_guard(dev, h, d):
    g = G.outside_graph()
    try:
        gen = torch.Generator().manual_seed(1)
        A = torch.rand((g.n_src, d) if h == 1 else (g.n_src, h, d), generator=gen)
        Be = torch.rand(g.n_edges, d, generator=gen)
        ge = torch.rand((g.n_edges,) if h == 1 else (g.n_edges, h), generator=gen)
        a3 = (g.row, g.ptr_r, g.eid_r)
        yo = oracle.node_mul_edge_forward(*a3, A, Be)
        dAo, dBo = oracle.node_mul_edge_backward(*a3, A, Be, ge)
        a3d = tuple(v.to(dev) for v in a3)
        Ad, Bd, ged = (G.banded(x, dev) for x in (A, Be, ge))

        def call():
            dA, dB = ops.node_mul_edge_backward(*a3d, Ad, Bd, ged)
            return dict(y=ops.node_mul_edge_forward(*a3d, Ad, Bd), dA=dA, dB=dB)
        got, _ = _under_guard(call, [a3d, Ad, Bd, ged], "node_mul_edge %d x %d" % (h, d))
        HP.close(got["y"], yo); HP.close(got["dA"], dAo); HP.close(got["dB"], dBo)
    finally:
        _reset()


@pytest.mark.parametrize("types", ["one", "past_table"])
@pytest.mark.parametrize("h,d", [(1, 64), (4, 32), (8, 32), (3, 5)])
def test_attention_tbias_under_guard(dev, h, d, types):
    """one type, and n_types * h one type past the 16 KiB LDS table of the fast row pass; need_dB on and off; against
    attention_tbias_reference at its bounds"""
    g = G.outside_graph()
    n_types = 1 if types == "one" else T.max_types(h) + 1
    inp = T.inputs(g, h, d, F32, 7 + h, n_types)
    want = T.reference_step(g.src, g.dst, g.n_src, *inp)
    n_max = T.n_max(inp[4], n_types)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    Q, K, V, B, etype, dO = (G.banded(x, dev) for x in inp)
    has = torch.bincount(g.src, minlength=g.n_src) > 0
    try:
        for need_dB in (True, False):
            def call():
                o, stats = ops.attention_tbias_forward(*a8[:4], Q, K, V, B, etype)
                dQ, dK, dV, dB = ops.attention_tbias_backward(*a8, Q, K, V, B, etype, o, stats, dO, 0.0, 0, 0, 0, need_dB)
                return dict(o=o, stats=stats, dQ=dQ, dK=dK, dV=dV, dB=dB)
            what = "tbias %d x %d, %d types, need_dB=%d" % (h, d, n_types, need_dB)
            got, _ = _under_guard(call, [a8, Q, K, V, B, etype, dO], what)
            for k in T.KEYS if need_dB else T.PLAIN:
                tol = T.tol(F32, 0.0, key=k, n_max=n_max)
                r = T.error_ratio(got[k].cpu(), want[k], **tol)
                print("%s %s: %.3f of the bound" % (what, k, r))
                assert got[k].dtype == F32 and r <= 1.0, (what, k, r)
            if not need_dB:
                assert got["dB"].shape == (0,) and got["dB"].dtype == F32
            st = got["stats"].cpu().reshape(g.n_src, h, 2)
            assert T.error_ratio(st[has], want["stats"][has], **T.tol(F32)) <= 1.0, what
            assert (st[~has][..., 0] == -1e9).all() and not st[~has][..., 1].any() and not got["o"].cpu()[~has].any(), what
    finally:
        _reset()


def test_attention_edge_odd_sized_dxe_under_guard(dev):
    """the hand case of the coverage condition (tests/test_guarded_host.py): dxe (E, 3, 5) whose byte size is no multiple
    of 16 -- every drawn edge case has d % 4 == 0 --, generic kernels, against attention_edge_reference at its bound"""
    g = G.outside_graph()
    h, d = 3, 5
    assert (g.n_edges * h * d * 4) % 16 != 0
    inp = AE.inputs(g.n_src, g.n_dst, g.n_edges, h, d, F32, 5)
    want = AE.reference_step(g.src, g.dst, g.n_src, *inp)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    Q, K, V, xe, dO = (G.banded(x, dev) for x in inp)
    try:
        def call():
            o, stats = ops.attention_edge_forward(*a8[:4], Q, K, V, xe)
            return dict(zip(AE.KEYS, [o] + list(ops.attention_edge_backward(*a8, Q, K, V, xe, o, stats, dO))), stats=stats)
        got, _ = _under_guard(call, [a8, Q, K, V, xe, dO], "attention_edge 3 x 5")
        for k in AE.KEYS:
            r = AE.error_ratio(got[k].cpu(), want[k], **AE.tol(F32))
            print("attention_edge 3 x 5 %s: %.3f of the bound" % (k, r))
            assert r <= 1.0, (k, r)
    finally:
        _reset()


def _weights_case(dev, kind, h, d, what):
    """a of the weights op, with and without the edge operand, from the statistics of the matching fused forward (made
    under the guard too), against gat_weights_reference.step at TOL_A"""
    g = G.outside_graph()
    mod = GE if kind == W.GAT else G2
    first, second, edge, last, _ = mod.inputs(g.src, g.dst, g.n_src, g.n_dst, h, d, F32, 40 + h + d, "unit")
    if kind == W.GATV2:
        last = last * 0.5          # (as gat_weights_reference.input_set: keeps |s| < 9, where TOL_A was set)
    a4 = tuple(x.to(dev) for x in g.csr_args()[:4])
    for with_edge in (False, True):
        o = W.with_edge((first, second, edge, last), with_edge)
        want = W.step(kind, g.src, g.dst, g.n_src, o, None, None, 0.2)["a"]
        f, s, e, l = (None if t is None else G.banded(t, dev) for t in o)

        def call():
            if kind == W.GAT:
                stats = (ops.gat_edge_attention_forward(*a4, f, s, e, l, 0.2) if with_edge else
                         ops.gat_attention_forward(*a4, f, s, l, 0.2))[1]
                return dict(stats=stats, a=ops.gat_attention_weights(*a4, f, s, stats, e, 0.2))
            stats = ops.gatv2_attention_dropout_forward(*a4, f, s, l, 0.2, xe=e)[1]
            return dict(stats=stats, a=ops.gatv2_attention_weights(*a4, f, s, l, stats, e, 0.2))
        w = "%s edge=%d" % (what, with_edge)
        got, _ = _under_guard(call, [a4] + [t for t in (f, s, e, l) if t is not None], w)
        a = got["a"].cpu()
        assert a.dtype == F32 and a.shape == want.shape, (w, a.shape, want.shape)
        r = W.error_ratio(a, want, **W.TOL_A)
        print("%s a: %.4f of the bound" % (w, r))
        assert r <= 1.0, (w, r)


@pytest.mark.parametrize("h", [1, 4, 8, 3])
def test_gat_attention_weights_under_guard(dev, h):
    try:
        _weights_case(dev, W.GAT, h, 8, "gat weights h=%d" % h)
    finally:
        _reset()


@pytest.mark.parametrize("h,d", [(1, 64), (4, 16), (8, 32), (3, 5)])
def test_gatv2_attention_weights_under_guard(dev, h, d):
    try:
        _weights_case(dev, W.GATV2, h, d, "gatv2 weights %d x %d" % (h, d))
    finally:
        _reset()


def test_edge_dropout_mask_under_guard(dev):
    """bit equal to dropout_reference.multipliers, fp32 and fp64, h = 1, 3, 8"""
    g = G.outside_graph()
    a4 = tuple(x.to(dev) for x in g.csr_args()[:4])
    try:
        for dtype in (F32, F64):
            for h in (1, 3, 8):
                got, _ = _under_guard(lambda: dict(m=ops.edge_dropout_mask(*a4, h, 0.6, 1234567890123, 7, dtype)), [a4],
                                      "edge_dropout_mask h=%d %s" % (h, dtype))
                want = DR.multipliers(g.src.numpy(), g.dst.numpy(), h, 0.6, 1234567890123, 7, dtype)
                assert got["m"].dtype == dtype and torch.equal(got["m"].cpu().reshape(g.n_edges, h), want), (dtype, h)
    finally:
        _reset()


def test_zz_guard_totals(dev):
    """what the tests above put under guard in this process (DESIGN.md 4.5r records the numbers of a full run)"""
    blocks, nbytes = G.plan_memory_counts()
    print("guarded calls %d, output / workspace allocations %d (%d bytes), plan blocks %d (%d bytes)"
          % (TOTALS["calls"], TOTALS["allocations"], TOTALS["bytes"], blocks, nbytes))
    assert ops.torch is torch
