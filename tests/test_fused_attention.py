"""GPU tier: the fused attention op (extra op) against the oracle's composition
of the three primitives (wrapper.py:20-30, 8-18, 44-55) on the same seeded inputs.

Two paths are covered: the fused window-owner passes (kernels_attn.h; fp32, one head, sweepable
plans -- forced on small graphs through the tuning knobs) and the composed path everything else
takes (several heads, fp64, odd d, plan-less chunk layouts).  Tolerance rtol 1e-4 / atol 1e-5
(north_star allows 1e-3)."""
import pytest
import torch

import oracle
from custom_op_benchmark_amd import _lib, functions, graphs
from custom_op_benchmark_amd import graphop as ops

from util import oracle_step, rand_inputs, random_graph

pytestmark = pytest.mark.gpu

TOL = {torch.float32: dict(rtol=1e-4, atol=1e-5), torch.float64: dict(rtol=1e-10, atol=1e-12)}


def close(got, want, dtype=torch.float32, **kw):
    tol = dict(TOL[dtype]); tol.update(kw)
    torch.testing.assert_close(got.cpu(), want, **tol)


def fused_step(g, Q, K, V, dO):
    Q = Q.clone().requires_grad_(True); K = K.clone().requires_grad_(True); V = V.clone().requires_grad_(True)
    o = functions.FusedAttention.apply(*g.csr_args(), Q, K, V)
    o.backward(dO)
    torch.cuda.synchronize()
    return dict(o=o.detach(), dQ=Q.grad, dK=K.grad, dV=V.grad)


def prof_tags(fn):
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return set(_lib.profile_read())
    finally:
        _lib.profile_enable(False)


def shuffled_chunk_arrays(g, seed):
    """The graph's eight arrays with both chunk lists in random order (chunks of a row not adjacent)."""
    gen = torch.Generator().manual_seed(seed)

    def shuffled(row, ptr):
        perm = torch.randperm(row.numel(), generator=gen)
        lens = (ptr[1:] - ptr[:-1])[perm]
        new_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
        slot = torch.cat([torch.arange(int(ptr[c]), int(ptr[c + 1])) for c in perm.tolist()])
        return row[perm].contiguous(), new_ptr, slot

    row, ptr_r, sr = shuffled(g.row, g.ptr_r)
    col, ptr_c, sc = shuffled(g.col, g.ptr_c)
    return (row, ptr_r, g.eid_r[sr].contiguous(), g.indices_r[sr].contiguous(),
            col, ptr_c, g.eid_c[sc].contiguous(), g.indices_c[sc].contiguous())


@pytest.fixture
def force_sweep():
    _lib.tune("sweep_min_kb", 0); _lib.tune("window_kb", 4); _lib.tune("vrow_t", 64)
    _lib.tune("max_windows", 512); _lib.tune("sweep_min_granule", 0)
    _lib.tune("attn_max_d", 1024)          # by default the fused window passes are only chosen up to d = 64
    _lib.clear_plan_cache()
    yield
    _lib.tune_reset(); _lib.clear_plan_cache()


@pytest.mark.parametrize("h,d", [(1, 64), (1, 16), (8, 16), (2, 32), (3, 5), (1, 128)])
def test_fused_step_vs_oracle_irregular(dev, h, d):
    """Small irregular graph (empty rows, a hub row, non-square): default knobs -> composed path."""
    g = random_graph(90, 131, 1500, seed=5, chunk_size=8, zero_rows=0.2, hub=200)
    inp = rand_inputs(g, h, d, seed=6, normal=True)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"][:g.n_src])
    got = fused_step(g.to(dev), *(inp[k].to(dev) for k in ("Q", "K", "V")), inp["dO"][:g.n_src].to(dev))
    want["o"] = want["o"][:g.n_src]        # the oracle's y = zeros_like(x) has n_dst rows (graphop_kernel.cu:527)
    for k in ("o", "dQ", "dK", "dV"):
        close(got[k], want[k])


@pytest.mark.parametrize("d", [64, 16, 4])
def test_fused_step_fp64(dev, d):
    g = random_graph(60, 60, 900, seed=9, chunk_size=8, zero_rows=0.1, hub=100)
    inp = rand_inputs(g, 1, d, seed=10, dtype=torch.float64, normal=True)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"])
    got = fused_step(g.to(dev), *(inp[k].to(dev) for k in ("Q", "K", "V", "dO")))
    for k in ("o", "dQ", "dK", "dV"):
        close(got[k], want[k], dtype=torch.float64)


@pytest.mark.parametrize("d,scale,k,bpc", [(64, 2, 0, 0), (64, 1, 2, 1), (16, 2, 0, 1), (32, 1, 0, 0),
                                           (128, 2, 0, 0), (256, 1, 0, 0), (512, 2, 0, 0), (1024, 1, 0, 0)])
@pytest.mark.parametrize("staged", [0, 7])
def test_fused_window_passes_vs_oracle(dev, force_sweep, d, scale, k, bpc, staged):
    """The fused window-owner passes (forced by tiny windows): rows longer than vrow_t are cut into
    pieces merged by atomics, empty rows / windows occur, non-square graph, several tasks per wave."""
    _lib.tune("attn_window_scale", scale); _lib.tune("attn_k", k); _lib.tune("attn_bpc", bpc)
    _lib.tune("staged_ids", staged)                  # ids per batch / staged through LDS (d <= 64 in the fused passes)
    _lib.tune("window_kb", 4 * max(1, d // 64))      # a few packed rows per window at every width
    n = 120 if d >= 512 else 1500
    g = random_graph(n, n + 41, 10 * n, seed=77 + d, chunk_size=32, zero_rows=0.15, hub=900)
    inp = rand_inputs(g, 1, d, seed=8, normal=True)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"][:g.n_src])
    gd = g.to(dev)
    args = [inp[x].to(dev) for x in ("Q", "K", "V")] + [inp["dO"][:g.n_src].to(dev)]
    got = fused_step(gd, *args)
    want["o"] = want["o"][:g.n_src]
    for key in ("o", "dQ", "dK", "dV"):
        close(got[key], want[key])
    tags = prof_tags(lambda: fused_step(gd, *args))
    assert {"attn_bwd_row", "attn_bwd_col"} <= tags, tags          # the fused kernels did run


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256, 1024])
@pytest.mark.parametrize("chunk_size,rows_sorted", [(8, True), (32, True), (8, False)])
def test_fused_chunk_driver_passes_vs_oracle(dev, d, chunk_size, rows_sorted):
    """The chunk-driver form of the fused passes (graphs with no window structure): forced on at every
    width; empty rows, a hub row cut into many chunks (the atomic merge), non-square; with the chunk
    list shuffled the kernels cannot own rows and every row is merged by atomics."""
    n = 64 if d >= 256 else 300
    g = random_graph(n, n + 37, 9 * n, seed=3 + d, chunk_size=chunk_size, zero_rows=0.2, hub=n // 2)
    inp = rand_inputs(g, 1, d, seed=4, normal=True)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"][:g.n_src])
    want["o"] = want["o"][:g.n_src]
    a8 = g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=11)
    a8 = tuple(v.to(dev) for v in a8)
    Q, K, V = (inp[x].to(dev) for x in ("Q", "K", "V"))
    dO = inp["dO"][:g.n_src].to(dev)

    def step():
        o, stats = ops.attention_forward(*a8[:4], Q, K, V)
        return (o,) + tuple(ops.attention_backward(*a8, Q, K, V, o, stats, dO))

    _lib.tune("attn_rows", 1); _lib.clear_plan_cache()
    try:
        assert ops.attention_backward_is_fused(*a8, Q, K)
        got = dict(zip(("o", "dQ", "dK", "dV"), step()))
        assert {"attn_rows_row", "attn_rows_col"} <= prof_tags(step)
        for key in ("o", "dQ", "dK", "dV"):
            close(got[key], want[key])
        _lib.tune("attn_rows", 0); _lib.clear_plan_cache()
        assert not ({"attn_rows_row", "attn_rows_col"} & prof_tags(step))
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


def test_fused_selection_follows_the_measured_rules(dev):
    """Which form attention_backward takes at the default knobs: the fused window passes up to d = 64
    (beyond, the two-row gathers dominate and they measure slower than the unfused passes); the
    chunk-driver form only where the unfused passes would not run on the window drivers either."""
    g = graphs.chung_lu_graph(30000, 3000000, alpha=0.5, seed=1, device=dev)      # 7.7 MB tables at d = 64: windows
    for d, want in ((64, True), (128, False), (256, False)):
        Q = torch.zeros(30000, d, device=dev)
        assert ops.attention_backward_is_fused(*g.csr_args(), Q, Q) == want, d
    q, k, v = (torch.rand(30000, 128, device=dev).requires_grad_(True) for _ in range(3))
    o = functions.fused_attention_step(g, q, k, v, torch.rand(30000, 128, device=dev))     # keeps a, unfused backward
    q2, k2, v2 = (x.detach().clone().requires_grad_(True) for x in (q, k, v))
    assert o.shape == (30000, 128) and q.grad is not None


def test_fused_chunk_driver_cost_rule(dev):
    """Default knobs: the chunk-driver passes run where the avoided E-sized streams outweigh packing
    (narrow rows, E/N large) and the composition runs where they do not (wide rows, E/N small)."""
    g = random_graph(400, 400, 8000, seed=2, chunk_size=32).to(dev)
    for d, want in ((16, True), (128, False)):
        Q = torch.zeros(400, d, device=dev)
        assert ops.attention_backward_is_fused(*g.csr_args(), Q, Q) == want, d


def test_fused_matches_unfused_medium_powerlaw(dev):
    """~1M edges, power-law degrees, d = 64, windows of 64 KB so the fused passes run at a realistic
    tile count; compared with the oracle AND with this library's own unfused composition."""
    _lib.tune("sweep_min_kb", 0); _lib.tune("window_kb", 64); _lib.tune("sweep_min_granule", 0); _lib.clear_plan_cache()
    try:
        g = graphs.chung_lu_graph(20000, 1000000, alpha=0.6, seed=0)
        inp = rand_inputs(g, 1, 64, seed=7, normal=True)
        want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"])
        gd = g.to(dev)
        args = [inp[x].to(dev) for x in ("Q", "K", "V", "dO")]
        got = fused_step(gd, *args)
        tags = prof_tags(lambda: fused_step(gd, *args))
        assert {"attn_bwd_row", "attn_bwd_col"} <= tags, tags
        for key in ("o", "dQ", "dK", "dV"):
            close(got[key], want[key], rtol=2e-4, atol=2e-5)
        q, k, v = (x.clone().requires_grad_(True) for x in args[:3])
        functions.attention_step(gd, q, k, v, args[3])
        for key, ref in (("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
            torch.testing.assert_close(got[key], ref, rtol=2e-4, atol=2e-5)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


def test_fused_uniform_inputs_and_large_scores(dev, force_sweep):
    """U[0,1) features (scores ~ d/4, the harness' input distribution, wrapper.py:151-153) and
    scores of magnitude 1e3: exp(s - m) must not overflow and stats must reproduce a."""
    g = random_graph(800, 800, 12000, seed=31, chunk_size=32, hub=700)
    # |s| ~ 16 and ~ 260: fp32 tolerance.  |s| ~ 1.4e4: one ulp of s is 1e-3, and a = exp(s - m)
    # carries that as a RELATIVE error whatever the implementation (the oracle's serial sums included),
    # so only a loose bound is meaningful there; what must hold is that nothing overflows (a <= 1:
    # the backward recomputes s bitwise as the forward stored it) and no NaN / inf appears.
    for scale, tol in ((1.0, dict(rtol=2e-4, atol=2e-5)), (4.0, dict(rtol=2e-4, atol=1e-4)),
                       (30.0, dict(rtol=2e-2, atol=1e-2))):
        inp = rand_inputs(g, 1, 64, seed=12)
        Q, K = inp["Q"] * scale, inp["K"] * scale
        want = oracle_step(oracle, g, Q, K, inp["V"], inp["dO"])
        got = fused_step(g.to(dev), Q.to(dev), K.to(dev), inp["V"].to(dev), inp["dO"].to(dev))
        for key in ("o", "dQ", "dK", "dV"):
            assert torch.isfinite(got[key]).all(), key
            close(got[key], want[key], **tol)


def test_fused_forward_stats(dev):
    """stats = (row max, 1 / sum exp) reproduce the softmax; rows without edges read (0, 0)."""
    g = random_graph(70, 70, 1200, seed=41, chunk_size=4, zero_rows=0.1)
    inp = rand_inputs(g, 2, 8, seed=42, normal=True)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"])
    gd = g.to(dev)
    Q, K, V, dO = (inp[x].to(dev) for x in ("Q", "K", "V", "dO"))
    o, stats = ops.attention_forward(gd.row, gd.ptr_r, gd.eid_r, gd.indices_r, Q, K, V)
    close(o, want["o"])
    m = torch.full((g.n_src, 2), -1e9).scatter_reduce(0, g.src[:, None].expand(-1, 2), want["s"], "amax")
    has = (g.indptr_r[1:] - g.indptr_r[:-1]) > 0
    close(stats[:, :, 0][has.to(dev)], m[has])
    ssum = torch.zeros(g.n_src, 2).index_add_(0, g.src, torch.exp(want["s"] - m[g.src]))
    close(stats[:, :, 1][has.to(dev)], 1.0 / ssum[has])
    assert float(stats[~has.to(dev)].abs().sum()) == 0.0
    dQ, dK, dV = ops.attention_backward(*gd.csr_args(), Q, K, V, o, stats, dO)
    close(dQ, want["dQ"]); close(dK, want["dK"]); close(dV, want["dV"])


@pytest.mark.parametrize("h,d", [(1, 64), (2, 8)])
def test_fused_unordered_chunks_take_the_general_path(dev, h, d):
    """Chunks of a row need not be adjacent (row[] unsorted): no row ownership, the softmax runs its
    atomics path with scratch from the workspace, and the fused op must still match."""
    g = random_graph(150, 150, 5000, seed=11, chunk_size=8, hub=300)
    inp = rand_inputs(g, h, d, seed=6, normal=True)
    a8 = shuffled_chunk_arrays(g, seed=0)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"])
    a8d = tuple(v.to(dev) for v in a8)
    assert _lib.get_plan(*a8d[:4], n_index_bound=g.n_dst).info.row_owned == 0
    Q, K, V, dO = (inp[x].to(dev) for x in ("Q", "K", "V", "dO"))
    o, stats = ops.attention_forward(*a8d[:4], Q, K, V)
    close(o, want["o"])
    dQ, dK, dV = ops.attention_backward(*a8d, Q, K, V, o, stats, dO)
    close(dQ, want["dQ"]); close(dK, want["dK"]); close(dV, want["dV"])


def test_fused_torch_ops_and_errors(dev):
    g = random_graph(40, 40, 300, seed=2, chunk_size=8).to(dev)
    Q, K, V = (torch.rand(40, 16, device=dev) for _ in range(3))
    o, stats = torch.ops.graphop.attention_forward(g.row, g.ptr_r, g.eid_r, g.indices_r, Q, K, V)
    o2, _ = ops.attention_forward(g.row, g.ptr_r, g.eid_r, g.indices_r, Q, K, V)
    assert torch.equal(o, o2)
    dQ, dK, dV = torch.ops.graphop.attention_backward(*g.csr_args(), Q, K, V, o, stats, torch.ones_like(o))
    assert dQ.shape == Q.shape and dK.shape == K.shape and dV.shape == V.shape
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.attention_forward(g.row, g.ptr_r, g.eid_r, g.indices_r, Q.cpu(), K, V)
    with pytest.raises(RuntimeError):
        ops.attention_forward(g.row, g.ptr_r, g.eid_r, g.indices_r, Q, K[:10].contiguous(), V[:10].contiguous())
    with pytest.raises(RuntimeError, match="row id"):
        ops.attention_forward(g.row, g.ptr_r, g.eid_r, g.indices_r, Q[:10].contiguous(), K, V)


def test_fused_step_replays_from_a_hip_graph(dev, force_sweep):
    """No op of the fused step synchronises or allocates outside torch's pool once the plans and
    window structures exist: the step captures into a HIP graph and replays bit-for-bit... up to
    the order of the float atomics."""
    g = random_graph(1500, 1500, 15000, seed=3, chunk_size=32, hub=900).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    Q, K, V, dO = (torch.randn(1500, 64, device=dev, generator=gen) / 8 for _ in range(4))
    eager = fused_step(g, Q, K, V, dO)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        functions.fused_attention_step(g, q, k, v, dO)
    torch.cuda.current_stream().wait_stream(side)
    q.grad = k.grad = v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = functions.fused_attention_step(g, q, k, v, dO)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(o.detach(), eager["o"], rtol=1e-5, atol=1e-6)
    for key, got in (("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
        torch.testing.assert_close(got, eager[key], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("seed", range(30))
def test_fused_fuzz_shapes_and_paths(dev, seed):
    """Randomised battery for the fused op: width, heads, chunk size, degree profile, square /
    non-square, windows forced on (random window size, piece length, K, resident grid, touch knob) or
    off.  Fused passes or composed path, whichever applies -- always vs the oracle."""
    import numpy as np
    rng = np.random.RandomState(4000 + seed)
    h = int(rng.choice([1, 1, 1, 2, 8]))
    d = int(rng.choice([4, 16, 64])) if h > 1 else int(rng.choice([16, 32, 64, 128, 256]))
    n_src = int(rng.randint(40, 900))
    n_dst = n_src if rng.rand() < 0.5 else int(rng.randint(40, 900))
    n_edges = int(rng.randint(1, 40) * n_src)
    cs = int(rng.choice([1, 7, 32, 64]))
    hub = int(rng.choice([0, 0, 300, 1500]))
    forced = bool(rng.rand() < 0.7)
    knobs = {}
    if forced:
        knobs = dict(sweep_min_kb=0, sweep_min_granule=0, max_windows=512, window_kb=int(rng.choice([1, 4, 16])),
                     vrow_t=int(rng.choice([0, 64, 256])), attn_window_scale=int(rng.choice([1, 2, 4])),
                     attn_k=int(rng.choice([0, 1, 2, 4])), attn_bpc=int(rng.choice([0, 1, 2])),
                     touch_sddmm=int(rng.choice([0, 1, 3])), attn_max_d=int(rng.choice([64, 1024, 1024])),
                     staged_ids=int(rng.choice([0, 7, 7])))
    for k, v in knobs.items():
        _lib.tune(k, v)
    _lib.clear_plan_cache()
    try:
        g = random_graph(n_src, n_dst, n_edges, seed=seed, chunk_size=cs, zero_rows=float(rng.choice([0, 0.2])),
                         hub=hub or None)
        # the oracle's SpMM output is zeros_like(x) (graphop_kernel.cu:527): x (n_dst rows) must cover the row ids
        if g.n_dst < g.n_src:
            g = random_graph(n_src, n_src, n_edges, seed=seed, chunk_size=cs, hub=hub or None)
        inp = rand_inputs(g, h, d, seed=seed + 50, normal=True)
        dO = inp["dO"][:g.n_src]
        want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], dO)
        want["o"] = want["o"][:g.n_src]
        got = fused_step(g.to(dev), *(inp[k].to(dev) for k in ("Q", "K", "V")), dO.to(dev))
        for key in ("o", "dQ", "dK", "dV"):
            close(got[key], want[key], rtol=2e-4, atol=2e-5)
    finally:
        for k, v in dict(sweep_min_kb=4608, sweep_min_granule=4, max_windows=128, window_kb=4096, vrow_t=0,
                         attn_window_scale=2, attn_k=0, attn_bpc=0, touch_sddmm=1, attn_max_d=64, staged_ids=7).items():
            _lib.tune(k, v)
        _lib.clear_plan_cache()


@pytest.mark.parametrize("h,d,dtype", [(3, 5, torch.float64), (2, 6, torch.float32), (1, 20, torch.float32), (8, 64, torch.float32)])
def test_fused_step_with_fewer_key_rows_than_query_rows(dev, h, d, dtype):
    """n_k < n_q where no fused form applies (seed 30 of tests/attention_fuzz.py: 3 x 5 in fp64 on 685+ rows and 545
    keys): FusedAttention used to take the unfused SpMM there, whose result has the row count of V, and raised.  One
    call and head groups, against the float64 statement of the definition."""
    import attention_dropout_reference as A
    g = random_graph(700, 545, 7000, seed=30, chunk_size=7, zero_rows=0.2, hub=300)
    assert int(g.src.max()) >= g.n_dst
    gen = torch.Generator().manual_seed(5)
    shape = (lambda n: (n, d) if h == 1 else (n, h, d))
    Q, dO = (torch.randn(*shape(g.n_src), generator=gen, dtype=torch.float64).to(dtype) / d ** 0.5 for _ in range(2))
    K, V = (torch.randn(*shape(g.n_dst), generator=gen, dtype=torch.float64).to(dtype) for _ in range(2))
    want = A.reference_step(g.src, g.dst, g.n_src, Q, K, V, dO, 0.0, 0)
    got = fused_step(g.to(dev), Q.to(dev), K.to(dev), V.to(dev), dO.to(dev))
    for key in ("o", "dQ", "dK", "dV"):
        assert got[key].shape == want[key].shape and got[key].dtype == dtype
        torch.testing.assert_close(got[key].cpu().double(), want[key], **TOL[dtype], msg=lambda m: "%s: %s" % (key, m))


@pytest.fixture
def force_fwd_walk():
    _lib.tune_reset()
    _lib.tune("sweep_min_kb", 0); _lib.tune("walk_window_kb", 8); _lib.tune("walk_window_kb_col", 8); _lib.tune("walk_min_bin", 0)
    _lib.tune("sweep_min_granule", 0); _lib.tune("max_windows", 512); _lib.tune("window_kb", 4); _lib.tune("vrow_t", 64)
    _lib.clear_plan_cache()
    yield
    _lib.tune_reset(); _lib.clear_plan_cache()


@pytest.mark.parametrize("blocks", [8, 24, 0])
@pytest.mark.parametrize("normal", [True, False])
def test_fused_forward_is_one_walk_pass_vs_oracle(dev, force_fwd_walk, blocks, normal):
    """attention_forward as ONE walk-style kernel (kernels_attn_walk.h: online softmax per (row, window) granule,
    running output rows and (max, sum) in LDS, no s / a in the workspace) at a forced small geometry: rows cut by
    bin boundaries (their pieces are merged by the three piece kernels), a hub row spanning many bins, empty rows,
    empty windows, several rounds, padded last chunks; against the oracle's composition of the three primitives
    (wrapper.py:20-30, 8-18, 44-55), and the backward (which recomputes from the statistics the forward left)."""
    _lib.tune("walk_blocks", blocks)
    g = random_graph(1500, 1541, 15000, seed=91 + blocks, chunk_size=32, zero_rows=0.15, hub=900)
    inp = rand_inputs(g, 1, 64, seed=12, normal=normal)
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], inp["dO"][:g.n_src])
    gd = g.to(dev)
    args = [inp[k].to(dev) for k in ("Q", "K", "V")] + [inp["dO"][:g.n_src].to(dev)]
    _lib.profile_enable(True)
    got = fused_step(gd, *args)
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    kern = {tag: r.get("kernel") for tag, r in prof.items()}
    assert kern.get("attn_fwd") == "k_attn_fwd_walk_f32", kern
    assert not ({"sddmm_fwd", "softmax_fwd", "spmm_fwd"} & set(kern)), kern          # nothing of the composed forward ran
    close(got["o"], want["o"][:g.n_src])
    for k in ("dQ", "dK", "dV"):
        close(got[k], want[k])
    # the statistics the forward leaves: (row maximum, 1 / sum) of the oracle's scores; rows without slots (0, 0)
    a4 = (gd.row, gd.ptr_r, gd.eid_r, gd.indices_r)
    o2, stats = ops.attention_forward(*a4, args[0], args[1], args[2])
    s = want["s"]
    deg = g.indptr_r[1:] - g.indptr_r[:-1]
    rows = torch.repeat_interleave(torch.arange(g.n_src), deg)
    m_ref = torch.full((g.n_src,), float("-inf")).scatter_reduce(0, rows, s, "amax", include_self=True)
    l_ref = torch.zeros(g.n_src).index_add_(0, rows, torch.exp(s - m_ref[rows]))
    has = deg > 0
    st = stats.cpu().reshape(-1, 2)
    torch.testing.assert_close(st[has, 0], m_ref[has], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(st[has, 1], 1.0 / l_ref[has], rtol=1e-4, atol=1e-7)
    assert (not (~has).any()) or float(st[~has].abs().max()) == 0.0
    close(o2, want["o"][:g.n_src])


def test_fused_forward_walk_matches_composed_forward_medium(dev, force_fwd_walk):
    """Same inputs through the one-pass forward and through the composed forward (knob attn_fwd_walk = 0)."""
    _lib.tune("walk_window_kb", 256); _lib.tune("window_kb", 256)
    g = graphs.chung_lu_graph(20000, 1000000, alpha=0.6, seed=3).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    Q, K, V = (torch.randn(20000, 64, device=dev, generator=gen) / 4 for _ in range(3))
    a4 = (g.row, g.ptr_r, g.eid_r, g.indices_r)
    tags = prof_tags(lambda: ops.attention_forward(*a4, Q, K, V))
    assert "attn_fwd" in tags, tags
    o1, st1 = ops.attention_forward(*a4, Q, K, V)
    _lib.tune("attn_fwd_walk", 0)
    tags = prof_tags(lambda: ops.attention_forward(*a4, Q, K, V))
    assert "attn_fwd" not in tags and "sddmm_fwd" in tags, tags
    o0, st0 = ops.attention_forward(*a4, Q, K, V)
    torch.testing.assert_close(o1, o0, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(st1, st0, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("mode", ["keep", "recompute"])
@pytest.mark.parametrize("h,d", [(8, 32), (8, 16), (4, 64), (2, 128), (6, 16), (8, 64)])
def test_fused_head_groups_vs_oracle(dev, force_sweep, h, d, mode, monkeypatch):
    """Round 5: FusedAttention over several heads runs in head groups of 256-B rows (one head per group from d = 64 on,
    where the one-head fused kernels apply to every head): no (E, h) tensor exists, the E-sized temporaries are (E, hg).
    Both modes -- a_g kept per group / recomputed in the backward -- against the oracle, on a non-square graph, with the
    window drivers forced so that the groups take the fused kernels where they apply (d <= 64, one head per group)."""
    monkeypatch.setattr(functions, "FUSED_HEADS_MODE", mode)
    rule = functions._head_group
    monkeypatch.setattr(functions, "_head_group", lambda h_, d_, *sizes: rule(h_, d_))   # (the small test graph is below the memory rule's bar)
    hg = functions._head_group(h, d)
    assert hg * d * 4 <= 256 or hg == 1
    g = random_graph(700, 941, 14000, seed=3 + h + d, chunk_size=32, zero_rows=0.1, hub=900)
    inp = rand_inputs(g, h, d, seed=5, normal=True)
    dO = inp["dO"][:g.n_src]
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], torch.cat([dO, torch.zeros(g.n_dst - g.n_src, h, d)]))
    gd = g.to(dev)
    tags = prof_tags(lambda: fused_step(gd, inp["Q"].to(dev), inp["K"].to(dev), inp["V"].to(dev), dO.to(dev)))
    if d == 64:
        assert {"attn_bwd_row", "attn_bwd_col"} <= tags, tags        # every head through the fused one-head passes
    got = fused_step(gd, inp["Q"].to(dev), inp["K"].to(dev), inp["V"].to(dev), dO.to(dev))
    close(got["o"], want["o"][:g.n_src])
    for k in ("dQ", "dK", "dV"):
        close(got[k], want[k])


def test_fused_head_groups_hold_no_e_by_h_tensor(dev):
    """The memory deliverable of the head groups, at a size where it shows (E x h = 16 M floats = 64 MB per edge tensor):
    the peak the fused step adds to what is allocated before it is well below the 8-function step's, in both modes."""
    _lib.tune_reset(); _lib.clear_plan_cache()
    N, E, h, d = 20000, 8_000_000, 8, 32
    assert functions._head_group(8, 16, 61_859_140, 2_449_029) == 8       # products-shape: node tensors dominate, no blocking
    assert functions._head_group(h, d, E, N) == 2
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    Q, K, V, dO = (torch.randn(N, h, d, device=dev, generator=gen) / 8 for _ in range(4))

    def peak(step):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def unfused():
        q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
        a8 = g.csr_args()
        o = functions.VectorSPMM.apply(*a8, functions.SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r,
                                                                         functions.MaskedMMCSR.apply(*a8, q, k)), v)
        o.backward(dO)
        return q.grad, k.grad, v.grad

    def fused():
        q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
        functions.FusedAttention.apply(*g.csr_args(), q, k, v).backward(dO)
        return q.grad, k.grad, v.grad

    edge_tensor = E * h * 4
    p_unfused = peak(unfused)
    ref = unfused()
    results = {}
    for mode in ("keep", "recompute"):
        functions.FUSED_HEADS_MODE = mode
        try:
            results[mode] = peak(fused)
            for a, b in zip(fused(), ref):
                torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5)
        finally:
            functions.FUSED_HEADS_MODE = "keep"
    assert p_unfused >= 2.9 * edge_tensor                       # a, da, ds (and s while the softmax runs)
    assert results["keep"] <= 0.70 * p_unfused, (results, p_unfused)        # a in groups + one group's da, ds (Reddit shape: 0.59)
    assert results["recompute"] <= 0.50 * p_unfused, (results, p_unfused)   # one group's s / a / da / ds (Reddit shape: 0.35)
