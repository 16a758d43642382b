"""CPU tier of the bfloat16 attention battery (tests/attention_bf16_fuzz.py): the draw is stable and pinned, seeds 0..47 cover
what the battery is there to cover (conditions, not measurements: BASE was chosen so that all of them hold), the graphs and
float64 scores have the structure the recipes are there to produce, and the bounds are reachable -- torch's own fp32
evaluation of the reference stays inside half the fp32 TOL before it is rounded and inside BF_TOL after one rounding to
bfloat16, for every suite seed.

Measured by test_fp32_torch_rounded_once_is_inside_the_bounds (the worst used fraction over the 48 seeds, large stratum at
256 CUs; fp32 before rounding against TOL, where at most 0.5 is allowed | after rounding against BF_TOL):
    o 0.39 | 0.97   dQ 0.30 | 0.96   dK 0.12 | 0.96   dV 0.02 | 0.96   m 0.07   1 / l 0.03"""
import hashlib

import torch

import attention_bf16_fuzz as F
import attention_bf16_reference as R

N_CU = 256
SEEDS = range(F.N_SUITE)
MARGIN = 0.5


def test_draw_is_deterministic_and_depends_on_the_seed_alone():
    first = [F.draw(s) for s in SEEDS]
    torch.manual_seed(123)      # (no global generator takes part)
    assert [F.draw(s) for s in SEEDS] == first
    assert len(set(first)) == len(first)
    for c in first:
        assert c.large == (c.seed % 4 == 3) and (c.h, c.d) in F.HD and c.recipe in F.RECIPES and c.entry in F.ENTRIES
        assert c.grad_view in F.GRAD_VIEWS and (c.entry == "autograd" or c.grad_view == "contiguous"), c
        if c.large:
            assert c.target_cpg in (2, 3) and c.chunk_size == 1 and c.hub == 0 and c.zero_rows == 0.0, c
        else:
            assert c.target_cpg == 0 and 40 <= c.n_src < 700 and 40 <= c.n_dst < 700 and c.n_src <= c.n_edges <= 39 * c.n_src, c
    a, b = F.build(first[0], N_CU), F.build(first[0], N_CU)
    assert all(torch.equal(u, v) for u, v in zip(a.csr + tuple(a.t.values()), b.csr + tuple(b.t.values())))
    assert all(v.dtype == torch.bfloat16 for v in a.t.values())


def test_the_48_suite_draws_are_pinned():
    """Whatever is refactored later, draw(seed) returns what it returned when the battery was written, field for field"""
    digest = hashlib.sha256(repr([F.draw(s) for s in range(48)]).encode()).hexdigest()
    assert digest == "65e578d51f2b97988d19d63c48f1a4b518b60cc3b99e9382ed2c52010d279f41"
    assert F.N_SUITE == 48 and F.RECIPES == ("flat", "unit", "wide8", "wide24", "ramp", "equal")


def test_layout_is_the_kernels():
    """(L, NV, SB) of AttnBf16Cfg, and the four classes the coverage conditions name"""
    assert [F.layout(h, d) for h, d in ((4, 16), (4, 32), (4, 64), (8, 64), (8, 8), (1, 128))] == \
        [(8, 1, 8), (16, 1, 8), (16, 2, 4), (16, 4, 2), (8, 1, 8), (16, 1, 8)]
    assert {F.nv_class(h, d) for h, d in F.HD} == set(F.NV_CLASSES) and len(F.HD) == 11
    assert [hd for hd in F.HD if F.nv_class(*hd) == "NV4"] == [(8, 64)]


def coverage_failures(cases):
    """the coverage conditions over the suite's seeds that do NOT hold -> list of strings"""
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    small, large = [c for c in cases if not c.large], [c for c in cases if c.large]
    need(4 * len(large) == len(cases), "one seed in four is large")
    for hd in F.HD:
        need(sum((c.h, c.d) == hd for c in small) >= 2, "%s in two small seeds" % (hd,))
    for r in F.RECIPES:
        need(sum(c.recipe == r for c in cases) >= 4, "recipe %s in four seeds" % r)
    for r in ("wide24", "ramp"):
        for k in F.NV_CLASSES:
            need(any(c.recipe == r and c.nv_class == k for c in cases), "%s at %s" % (r, k))
    for e in F.ENTRIES:
        need(any(c.entry == e for c in cases), "entry %s" % e)
    for v in F.GRAD_VIEWS:
        need(any(c.grad_view == v and c.entry == "autograd" for c in cases), "grad_view %s" % v)
    for k in F.NV_CLASSES:
        need(any(c.nv_class == k for c in large), "a large seed at %s" % k)
    for cpg in (2, 3):
        need(any(c.target_cpg == cpg for c in large), "a large seed at cpg %d" % cpg)
    need(any(c.hub and c.chunk_size == 1 for c in small), "a small seed with a hub and chunk_size = 1")
    need(any(c.hub and c.chunk_size >= 32 for c in small), "a small seed with a hub and chunk_size >= 32")
    return bad


def test_coverage_of_the_suite_seeds():
    assert coverage_failures([F.draw(s) for s in SEEDS]) == []


def _scores(built, head=0):
    """float64 scores of one head in CSR slot order"""
    g = built.g
    return (built.t["Q"][:, head].double()[g.src] * built.t["K"][:, head].double()[g.dst]).sum(-1)


def rising_batches(case, built, r, s):
    """(batches of row r after its first in which the running maximum rises, batches after its first): the batches are
    those of k_attn_bf16_fwd_rows, SB slots at a time inside each chunk of the row, in chunk order"""
    g = built.g
    chunks = (g.row == r).nonzero().flatten().tolist()
    assert chunks == list(range(chunks[0], chunks[-1] + 1))
    m, rises, n = float("-inf"), 0, 0
    for c in chunks:
        j0, j1 = int(g.ptr_r[c]), int(g.ptr_r[c + 1])
        for jb in range(j0, j1, case.sb):
            top = float(s[jb:min(jb + case.sb, j1)].max())
            if m > float("-inf"):
                n += 1
                rises += top > m
            m = max(m, top)
    return rises, n


def test_the_recipes_produce_the_structure_they_are_there_for():
    """ramp with a hub: in some even (ascending) row of at least five batches the running maximum, in the order the kernel
    meets the slots, rises in at least half of the batches after the first.  wide24: some row holds two scores more than 87
    apart.  Large stratum: lane groups that share both their first and their last row with their neighbours, and groups
    wholly inside one row, as test_several_chunks_per_lane_group counts them."""
    seen = {"ramp": 0, "wide24": 0, "large": 0}
    for seed in SEEDS:
        case, built, _ = F.case_data(seed, N_CU)
        g = built.g
        if case.recipe == "ramp" and case.hub:
            s = _scores(built)
            deg = torch.bincount(g.src, minlength=g.n_src)
            even = [r for r in torch.argsort(deg, descending=True).tolist() if r % 2 == 0][:8]
            best = max(((rises / n, n) for rises, n in (rising_batches(case, built, r, s) for r in even) if n >= 4), default=(0, 0))
            print("seed %d ramp: the maximum rises in %.2f of %d batches" % (seed, best[0], best[1]))
            assert best[0] >= 0.5, (case, best)
            seen["ramp"] += 1
        if case.recipe == "wide24":
            s = _scores(built)
            idx = g.src
            hi = torch.full((g.n_src,), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amax")
            lo = torch.full((g.n_src,), float("inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amin")
            spread = float((hi - lo)[F.live_rows(built)].max())
            print("seed %d wide24: the widest row spans %.1f" % (seed, spread))
            assert spread > F.UNDERFLOW, (case, spread)
            seen["wide24"] += 1
        if case.large:
            cpg = F.assert_cpg(case, built, N_CU)
            for row in (g.row.tolist(), g.col.tolist()):
                both = inside = 0
                for c0 in range(cpg, len(row) - cpg, cpg):
                    first, last = row[c0], row[c0 + cpg - 1]
                    both += first != last and first == row[c0 - 1] and last == row[c0 + cpg]
                    inside += first == last and first == row[c0 - 1] and last == row[c0 + cpg]
                assert both > 0 and inside > 0, (case, both, inside)
            seen["large"] += 1
    assert seen["ramp"] >= 1 and seen["wide24"] >= 4 and seen["large"] == 12, seen


def test_fp32_torch_rounded_once_is_inside_the_bounds():
    """The reference's lines in plain fp32 torch on the CPU (one thread, so that the figures repeat).  Before rounding: at
    most MARGIN = 0.5 of the fp32 TOL against the float64 reference, so a correct kernel that sums in another order has the
    other half.  After ONE round-to-nearest to bfloat16: inside BF_TOL.  The backward gets the rounded o, as the op does,
    and its float64 reference gets that same o."""
    worst = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for seed in SEEDS:
            case, built, want = F.case_data(seed, N_CU)
            f32 = F.reference_forward(case, built, torch.float32)
            o_bf = f32["o"].to(F.BF)
            b32 = F.reference_backward(case, built, o_bf, torch.float32)
            b64 = F.reference_backward(case, built, o_bf)
            live = F.live_rows(built)
            used = {"o": (F.error_ratio(f32["o"], want["o"], **F.F32), F.error_ratio(o_bf, want["o"], **F.BF_TOL))}
            for name in ("dQ", "dK", "dV"):
                assert b32[name].dtype == torch.float32
                used[name] = (F.error_ratio(b32[name], b64[name], **F.F32),
                              F.error_ratio(b32[name].to(F.BF), b64[name], **F.BF_TOL))
            used["m"] = (F.error_ratio(f32["m"][live], want["m"][live], **F.F32), 0.0)
            used["1 / l"] = (F.error_ratio(f32["linv"], want["linv"], **F.F32), 0.0)
            for name, (before, after) in used.items():
                w = worst.setdefault(name, [0.0, 0.0])
                w[0], w[1] = max(w[0], before), max(w[1], after)
                assert before <= MARGIN, "seed %d %s: fp32 torch uses %.3f of the fp32 bound\n%s" % (seed, name, before, case)
                assert after <= 1.0, "seed %d %s: fp32 torch rounded once uses %.3f of BF_TOL\n%s" % (seed, name, after, case)
    finally:
        torch.set_num_threads(threads)
    print("    " + "   ".join("%s %.2f | %.2f" % (n, a, b) for n, (a, b) in worst.items()))


def test_the_equal_recipe_is_what_the_gpu_tier_assumes():
    """Q = 0: the float64 reference has m = 0, 1 / l = 1 / deg, o the mean of V, and dQ = 0 on the rows of degree 0 and 1"""
    seeds = [s for s in SEEDS if F.draw(s).recipe == "equal" and not F.draw(s).large]
    single = 0
    for seed in seeds:
        case, built, want = F.case_data(seed, N_CU)
        g = built.g
        deg = torch.bincount(g.src, minlength=g.n_src)
        live = deg > 0
        assert not want["m"][live].any()
        assert torch.allclose(want["linv"][live], (1.0 / deg[live].double())[:, None].expand(-1, case.h), rtol=1e-14, atol=0)
        mean = torch.zeros(g.n_src, case.h, case.d, dtype=torch.float64).index_add_(0, g.src, built.t["V"].double()[g.dst])
        assert torch.allclose(want["o"][live], mean[live] / deg[live, None, None], rtol=1e-12, atol=1e-14)
        dQ = R.backward(g.src, g.dst, built.t["Q"], built.t["K"], built.t["V"], want["o"].to(F.BF), built.t["dO"])[0]
        assert not dQ[deg <= 1].any()
        single += int((deg == 1).sum())
    assert len(seeds) >= 2 and single > 0
