"""CPU tier of the GAT family's randomised battery (tests/gat_fuzz.py): the draw is stable, seeds 0..47 cover what the
battery is there to cover (conditions, not measurements: gat_fuzz.BASE was chosen so that all of them hold), torch's own
fp32 evaluation of every case's reference uses at most half of every bound, and expected_kernels agrees with the kernel
tables of the families' own modules.

Measured by test_fp32_references_use_at_most_half_of_every_bound (the worst used fraction of a bound over the family's
eight seeds, large stratum at 256 CUs):
    gat_scores          y 0.00  del 0.09  der 0.09
    gatv2_scores        y 0.04  dxl 0.16  dxr 0.05  datt 0.03
    fused_gat           o 0.13  del 0.30  der 0.07  dV 0.17
    fused_gat_dropout   o 0.15  del 0.17  der 0.07  dV 0.02
    fused_gatv2         o 0.04  stats 0.03  dxl 0.29  dxr 0.07  datt 0.03
    fused_gatv2_dropout o 0.05  stats 0.02  dxl 0.10  dxr 0.07  datt 0.08
The largest, del at 0.30, is the fused GAT layer at slope 1 and d = 64 with a hub row of 1500 slots: del is zero there up to
the rounding of D = <dO, o>."""
import dataclasses

import torch

import gat_fuzz as F
import fused_gatv2_reference as R

N_CU = 256
SEEDS = range(F.N_SUITE)
MARGIN = 0.5


def test_draw_is_deterministic_and_depends_on_the_seed_alone():
    first = [F.draw(s) for s in SEEDS]
    torch.manual_seed(123)      # (no global generator takes part)
    assert [F.draw(s) for s in SEEDS] == first
    assert len(set(first)) == len(first)
    assert [c.family for c in first[:6]] == list(F.FAMILIES)
    for c in first:
        assert c.family == F.FAMILIES[c.seed % 6] and c.large == ((c.seed // 6) % 4 == 3)
        assert c.dtype in ("float32", "float64") and c.entry in F.BINDINGS + ("autograd",)
        if c.large:
            assert c.dtype == "float32" and F.fast_shape(c) and not c.force_generic and c.misaligned < 0, c
            assert c.spmm_cpg in (0, 16) and c.chunk_size == 1 and c.target_cpg in (2, 3) and (c.d == 0 or c.h * c.d <= 128), c
    a, b = F.build(first[0], N_CU), F.build(first[0], N_CU)
    assert all(torch.equal(u, v) for u, v in zip(a.csr + a.inputs + (a.grad,), b.csr + b.inputs + (b.grad,)))


def test_the_48_suite_draws_are_pinned():
    """gat_edge_fuzz.py shares this module's helpers: whatever is refactored for it, draw(seed) of this battery returns
    what it returned when the battery was written, field for field, for every suite seed."""
    import hashlib
    digest = hashlib.sha256(repr([F.draw(s) for s in range(48)]).encode()).hexdigest()
    assert digest == "60ac2b6b979c26693c10348f60cab203bde3422f828cae014697d7c1f9ce2ce3"
    assert F.BASE == 36088 and F.N_SUITE == 48


def coverage_failures(cases):
    """the coverage conditions over the suite's seeds that do NOT hold -> list of strings"""
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    for fam in F.FAMILIES:
        cs = [c for c in cases if c.family == fam]
        count = lambda f: sum(1 for c in cs if f(c))
        need(len(cs) == 8 and count(lambda c: c.large) == 2, "%s: 8 seeds, 2 of them large" % fam)
        need(count(lambda c: c.dtype == "float64") >= 1, "%s: an fp64 seed" % fam)
        need(count(lambda c: c.shuffled) >= 1, "%s: a shuffled seed" % fam)
        need(count(lambda c: not F.fast_shape(c)) >= 1, "%s: a seed that is generic by shape" % fam)
        need(count(lambda c: not c.large and c.n_src != c.n_dst) >= 1, "%s: a rectangular seed" % fam)
        need(count(lambda c: c.hub == 1500) >= 1, "%s: a seed with hub == 1500" % fam)
        need(count(lambda c: c.force_generic or c.misaligned >= 0) >= 1, "%s: force_generic or a misaligned table" % fam)
        need(count(F.all_fast) >= 3, "%s: 3 seeds whose kernels are all fast" % fam)
        if fam in F.DROPOUT_FAMILIES:
            need(count(lambda c: c.p == 0.9) >= 1, "%s: p = 0.9" % fam)
            need(count(lambda c: c.p == 0.0) >= 1, "%s: p = 0" % fam)
            need(count(lambda c: c.philox_seed >= 2 ** 32) >= 1, "%s: a Philox seed >= 2^32" % fam)
            need(count(lambda c: c.offset == 2 ** 32 - 1) >= 1, "%s: offset = 2^32 - 1" % fam)
    for entry in F.BINDINGS + ("autograd",):
        need(len({c.family for c in cases if c.entry == entry}) >= 4, "entry %s in 4 families" % entry)
    return bad


def test_coverage_of_the_suite_seeds():
    cases = [F.draw(s) for s in SEEDS]
    assert coverage_failures(cases) == []
    assert all(0 <= c.philox_seed < 2 ** 63 and 0 <= c.offset < 2 ** 32 and 0 <= c.p < 1 for c in cases)


def test_fp32_references_use_at_most_half_of_every_bound():
    """Every seed's formula in plain torch fp32 on the CPU (the references in their dtype=torch.float32 mode) against the
    float64 reference: at most MARGIN = 0.5 of every bound, datt's included, so a correct fp32 kernel that sums in
    another order has the other half.  The fp32 evaluation runs on one thread, so that the figures repeat.  fp64 cases are
    measured on their inputs rounded to fp32, against the fp32 bounds."""
    worst = {fam: {} for fam in F.FAMILIES}
    for seed in SEEDS:
        case, built, want = F.case_data(seed, N_CU)
        if case.dtype == "float64":
            case = dataclasses.replace(case, dtype="float32")
            built = F.Built(built.g, built.csr, tuple(t.float() for t in built.inputs), built.grad.float())
            want = F.reference(case, built)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)      # (with several, torch's backward of x[src] adds in an order that changes from run to
        try:                          #  run: the used fraction of one hub row's bound moved between 0.07 and 0.46)
            got = F.reference(case, built, dtype=torch.float32)
        finally:
            torch.set_num_threads(threads)
        used = F.ratios(case, got, want)
        assert set(used) == set(F.OUTPUTS[case.family])
        for name, r in used.items():
            assert got[name].dtype == torch.float32
            worst[case.family][name] = max(worst[case.family].get(name, 0.0), r)
            assert r <= MARGIN, "seed %d %s: fp32 torch uses %.3f of the bound\n%s" % (seed, name, r, case)
    for fam in F.FAMILIES:
        print("%-20s" % fam + "  ".join("%s %.2f" % (n, worst[fam][n]) for n in F.OUTPUTS[fam]))


def _case(**kw):
    return dataclasses.replace(F.draw(0), **kw)


def test_expected_kernels_against_the_tables_of_the_family_modules():
    import test_fused_gatv2 as TF
    import test_gat_launch_geometry as TG
    import test_gatv2_dropout as TD
    base = dict(h=4, d=16, dtype="float32", shuffled=False, force_generic=False, misaligned=-1, p=0.0)
    # 1. fused GATv2, aligned fast shape / shuffled chunk lists / a generic shape
    assert F.expected_kernels(_case(family="fused_gatv2", **base)) == TF.FAST_NAMES
    assert F.expected_kernels(_case(family="fused_gatv2", **dict(base, shuffled=True))) == \
        dict(TF.FAST_NAMES, gv2attn_fwd="k_gv2attn_fwd_generic")
    assert F.expected_kernels(_case(family="fused_gatv2", **dict(base, h=3, d=5))) == TF.GENERIC_NAMES
    # 2. its dropout form: p > 0 on the fast and in fp64 on the generic kernels, p = 0 under the undropped tags
    drop = dict(base, p=0.5)
    assert F.expected_kernels(_case(family="fused_gatv2_dropout", **drop)) == TD.FAST_NAMES
    assert F.expected_kernels(_case(family="fused_gatv2_dropout", **dict(drop, dtype="float64"))) == TD.GENERIC_NAMES
    assert F.expected_kernels(_case(family="fused_gatv2_dropout", **base)) == TD.UNDROPPED_FAST
    # 3. the fused GAT layer and the two score ops
    assert F.expected_kernels(_case(family="fused_gat", **base)) == TG.FUSED_FAST
    assert F.expected_kernels(_case(family="fused_gat_dropout", **dict(drop, shuffled=True))) == \
        TG._generic(TG.DROP_FAST, "gat_attn_stats")
    assert F.expected_kernels(_case(family="fused_gat_dropout", **dict(drop, force_generic=True))) == TG._generic(TG.DROP_FAST)
    assert F.expected_kernels(_case(family="gatv2_scores", **dict(base, misaligned=2))) == TG._generic(TG.GATV2_FAST)
    assert F.expected_kernels(_case(family="gat_scores", **dict(base, h=16, d=0))) == TG.GAT_FAST
    assert F.expected_kernels(_case(family="gat_scores", **dict(base, h=1, d=0, misaligned=0))) == TG.GAT_FAST
    assert F.expected_kernels(_case(family="gat_scores", **dict(base, h=2, d=0, misaligned=0))) == TG._generic(TG.GAT_FAST)
    assert R.FAST == TG.FAST_HD
