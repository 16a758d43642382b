"""CPU tier of the edge-term battery (tests/gat_edge_fuzz.py): the draw is stable, seeds 0..23 cover what the battery is
there to cover (conditions, not measurements: gat_edge_fuzz.BASE was chosen so that all of them hold), torch's own fp32
evaluation of every case's reference uses at most half of every bound, and expected_kernels agrees with the kernel tables
of test_gat_edge.py.

Measured by test_fp32_references_use_at_most_half_of_every_bound (the worst used fraction of a bound over the 24 seeds,
large stratum at 256 CUs):
    o 0.13  del 0.32  der 0.09  dee 0.43  dV 0.09
The largest, dee at 0.43, is seed 9: (1, 128) with a hub row of 1500 slots, where D = <dO, o> is a sum of 128 products
and dee = a (da - D) is small against both."""
import dataclasses

import torch

import gat_edge_fuzz as G
import gat_edge_reference as E

N_CU = 256
SEEDS = range(G.N_SUITE)
MARGIN = 0.5


def test_draw_is_deterministic_and_depends_on_the_seed_alone():
    first = [G.draw(s) for s in SEEDS]
    torch.manual_seed(123)      # (no global generator takes part)
    assert [G.draw(s) for s in SEEDS] == first
    assert len(set(first)) == len(first)
    for c in first:
        assert c.large == (c.seed % 4 == 3)
        assert c.dtype in ("float32", "float64") and c.entry in G.ENTRIES and c.kind in G.KINDS, c
        assert c.numbering in G.NUMBERINGS and -1 <= c.misaligned < len(G.TABLES), c
        assert c.grad_view == "contiguous" or c.entry == "autograd", c
        if c.large:
            assert c.dtype == "float32" and G.fast_shape(c) and not c.force_generic and c.misaligned < 0, c
            assert c.spmm_cpg in (0, 16) and c.chunk_size == 1 and c.target_cpg in (2, 3) and c.h * c.d <= 128, c
    a, b = G.build(first[0], N_CU), G.build(first[0], N_CU)
    assert all(torch.equal(u, v) for u, v in zip(a.csr + a.inputs + (a.grad, a.src, a.dst),
                                                 b.csr + b.inputs + (b.grad, b.src, b.dst)))


def coverage_failures(cases):
    """the coverage conditions over the suite's seeds that do NOT hold -> list of strings"""
    bad = []
    count = lambda f: sum(1 for c in cases if f(c))

    def need(cond, what):
        if not cond:
            bad.append(what)
    would_be_fast = lambda c: c.dtype == "float32" and not c.force_generic and G.fast_shape(c)
    generic = lambda c: all(k.endswith("_generic") for k in G.expected_kernels(c).values())
    need(count(lambda c: c.large) >= 5, "5 large seeds")
    need(count(lambda c: c.dtype == "float64") >= 1, "an fp64 seed")
    need(count(lambda c: c.shuffled) >= 1, "a shuffled seed")
    need(count(lambda c: not c.large and c.n_src != c.n_dst) >= 1, "a rectangular seed")
    need(count(lambda c: c.hub == 1500) >= 1, "a seed with hub == 1500")
    need(count(lambda c: not G.fast_shape(c)) >= 1, "a seed that is generic by shape")
    for numbering in G.NUMBERINGS:
        need(count(lambda c: c.numbering == numbering) >= 3, "numbering %s 3 times" % numbering)
    need(count(lambda c: c.numbering == "col_identity" and G.all_fast(c) and c.p > 0) >= 1,
         "col_identity on all-fast kernels with p > 0")
    for kind in G.KINDS:
        need(count(lambda c: c.kind == kind) >= 1, "ee kind %s" % kind)
    need(count(lambda c: not c.need_dee and c.p > 0) >= 1, "need_dee = False with p > 0")
    need(count(lambda c: not c.need_dee and c.p == 0) >= 1, "need_dee = False with p = 0")
    need(count(lambda c: c.p == 0.9) >= 1, "p = 0.9")
    need(count(lambda c: c.p == 0.0) >= 1, "p = 0")
    need(count(lambda c: c.philox_seed >= 2 ** 32) >= 1, "a Philox seed >= 2^32")
    need(count(lambda c: c.offset == 2 ** 32 - 1) >= 1, "offset = 2^32 - 1")
    ee_off = lambda c: c.misaligned >= 0 and G.TABLES[c.misaligned] == "ee" and would_be_fast(c)
    need(count(lambda c: ee_off(c) and c.h == 1 and G.all_fast(c)) >= 1, "ee misaligned at h = 1, kernels fast")
    need(count(lambda c: ee_off(c) and c.h >= 2 and generic(c)) >= 1, "ee misaligned at h >= 2, kernels generic")
    need(count(lambda c: c.force_generic) >= 1, "force_generic")
    for entry in G.ENTRIES:
        need(count(lambda c: c.entry == entry) >= 2, "entry %s twice" % entry)
    need(count(G.all_fast) >= 8, "8 seeds whose five kernels are all fast")
    return bad


def test_coverage_of_the_suite_seeds():
    cases = [G.draw(s) for s in SEEDS]
    assert coverage_failures(cases) == []
    assert all(0 <= c.philox_seed < 2 ** 63 and 0 <= c.offset < 2 ** 32 and 0 <= c.p < 1 for c in cases)
    for c in cases:
        assert len(G.expected_kernels(c)) == 5


def test_fp32_references_use_at_most_half_of_every_bound():
    """Every seed's formula in plain torch fp32 on the CPU (gat_edge_fuzz.reference in its dtype=torch.float32 mode)
    against the float64 reference: at most MARGIN = 0.5 of every bound, so a correct fp32 kernel that sums in another
    order has the other half.  The fp32 evaluation runs on one thread, so that the figures repeat.  fp64 cases are
    measured on their inputs rounded to fp32, against the fp32 bounds; dee is measured whether or not the case asks
    for it."""
    worst = {}
    for seed in SEEDS:
        case, built, want = G.case_data(seed, N_CU)
        case = dataclasses.replace(case, need_dee=True)
        if case.dtype == "float64":
            case = dataclasses.replace(case, dtype="float32")
            built = G.EdgeBuilt(built.g, built.csr, tuple(t.float() for t in built.inputs), built.grad.float(),
                                built.src, built.dst)
            want = G.reference(case, built)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)      # (as in test_gat_fuzz_host.py: the order of torch's scatter adds)
        try:
            got = G.reference(case, built, dtype=torch.float32)
        finally:
            torch.set_num_threads(threads)
        used = G.ratios(case, got, want)
        assert set(used) == set(G.OUTPUTS)
        for name, r in used.items():
            assert got[name].dtype == torch.float32
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= MARGIN, "seed %d %s: fp32 torch uses %.3f of the bound\n%s" % (seed, name, r, case)
    print("  ".join("%s %.2f" % (n, worst[n]) for n in G.OUTPUTS))


def _case(**kw):
    base = dict(h=4, d=16, dtype="float32", large=False, shuffled=False, force_generic=False, misaligned=-1, p=0.0)
    return dataclasses.replace(G.draw(0), **dict(base, **kw))


def test_expected_kernels_against_the_tables_of_test_gat_edge():
    import test_gat_edge as T
    fast, generic, drop_fast = (dict(zip(T.TAGS, T.FAST)), dict(zip(T.TAGS, T.GENERIC)), dict(zip(T.DROP_TAGS, T.DROP_FAST)))
    drop_generic = {t: k.replace("_f32", "_generic") for t, k in drop_fast.items()}
    ee, el = G.TABLES.index("ee"), G.TABLES.index("el")
    assert G.expected_kernels(_case()) == fast
    assert G.expected_kernels(_case(p=0.5)) == drop_fast
    assert G.expected_kernels(_case(h=3, d=5)) == generic
    assert G.expected_kernels(_case(dtype="float64", p=0.1)) == drop_generic
    assert G.expected_kernels(_case(force_generic=True)) == generic
    assert G.expected_kernels(_case(shuffled=True)) == dict(fast, gat_edge_attn_stats="k_gat_edge_attn_stats_generic")
    assert G.expected_kernels(_case(shuffled=True, p=0.9)) == \
        dict(drop_fast, gat_edge_attn_stats="k_gat_edge_attn_stats_generic")
    # a table 4 bytes off: el / er / V ask 16 bytes at every h; ee asks 4 * min(h, 4)
    assert G.expected_kernels(_case(h=1, d=64, misaligned=ee)) == fast
    assert G.expected_kernels(_case(h=1, d=64, misaligned=el)) == generic
    for h, d in ((2, 32), (4, 16), (8, 8)):
        assert G.expected_kernels(_case(h=h, d=d, misaligned=ee)) == generic
        assert G.expected_kernels(_case(h=h, d=d, misaligned=ee, p=0.5)) == drop_generic
    assert list(G.FAST_HD) == T.FAST_HD and G.OUTPUTS == E.NAMES


def test_edge_numberings():
    """The three numberings on one small graph: which orientation reads eid == arange, and the edge list in edge-id
    order names the same edges through both orientations' eid arrays."""
    case = dataclasses.replace(G.draw(0), large=False, n_src=50, n_dst=40, n_edges=300, chunk_size=3, hub=0)
    g0 = G.F.drawn_graph(case, N_CU)
    ar = torch.arange(g0.n_edges)
    for numbering, row_id, col_id in (("row_identity", True, False), ("col_identity", False, True),
                                      ("permuted", False, False)):
        g, src, dst = G.number_edges(dataclasses.replace(case, numbering=numbering), g0)
        assert torch.equal(g.eid_r, ar) == row_id and torch.equal(g.eid_c, ar) == col_id, numbering
        assert torch.equal(torch.sort(g.eid_r)[0], ar) and torch.equal(torch.sort(g.eid_c)[0], ar)
        assert torch.equal(src[g.eid_r], g0.src) and torch.equal(dst[g.eid_r], g0.dst)          # row-major slots
        assert torch.equal(dst[g.eid_c], torch.repeat_interleave(torch.arange(g.n_dst), g.indptr_c[1:] - g.indptr_c[:-1]))
        assert torch.equal(src[g.eid_c], g.indices_c)                                            # column-major slots
