"""CPU tier of the dot-product attention family's randomised battery (tests/attention_fuzz.py): the draw is stable, seeds
0..47 cover what the battery is there to cover (conditions, not measurements: attention_fuzz.BASE was chosen so that all
of them hold), torch's own fp32 evaluation of every case's reference uses at most half of every bound, and expected_forms
agrees with the launch tables and tag sets of the ops' own modules.

Measured by test_fp32_references_use_at_most_half_of_every_bound (the worst used fraction of a bound over the family's
eight seeds, large stratum at 256 CUs):
    plain    o 0.07  dQ 0.03  dK 0.01  dV 0.01  stats 0.02
    dropout  o 0.06  dQ 0.02  dK 0.00  dV 0.00  stats 0.01
    bias     o 0.03  dQ 0.02  dK 0.01  dV 0.00  db 0.01  stats 0.02
    edge     o 0.05  dQ 0.05  dK 0.01  dV 0.00  dxe 0.01  stats 0.04
    etype    o 0.07  dQ 0.28  dK 0.01  dV 0.00  dR 0.10  stats 0.02
    weights  a 0.04  o 0.03  dQ 0.06  dK 0.02  dV 0.00  db 0.03  stats 0.02  dxe 0.01
The output gradients are / 4 (attention_fuzz.GRAD_SCALE says which two seeds went over the half at unit scale)."""
import dataclasses
import hashlib

import torch

import attention_etype_reference as T
import attention_fuzz as F

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
        assert c.dtype in ("float32", "float64") and c.entry in F.ENTRIES and c.route in F.ROUTES
        assert 0 <= c.philox_seed < 2 ** 63 and 0 <= c.offset < 2 ** 32 and 0 <= c.p < 1 and 0 <= c.head0 < 2 ** 32
        assert c.dO or c.ga, c
        assert c.misaligned < 0 or c.op in ("edge", "etype"), c          # (attention.hip looks at no pointer's alignment)
        assert c.head0 == 0 or (c.raw and c.p > 0 and c.family in ("dropout", "bias", "edge", "etype")), c
        assert (c.n_types >= 1) == (c.family == "etype") and (c.mode in F.MODES) == (c.family == "weights"), c
        if c.large:
            assert c.dtype == "float32" and c.route == "fused" and c.misaligned < 0 and c.chunk_size == 1, c
            assert ((c.h, c.d) in F.HD and c.h * c.d <= 128) and c.target_cpg in (2, 3), c
            assert c.shuffled == ((c.seed // 24) % 2 == 1), c
    a, b = F.build(first[0], N_CU), F.build(first[0], N_CU)
    assert all(torch.equal(u, v) for u, v in zip(a.csr + tuple(a.t.values()), b.csr + tuple(b.t.values())))


def test_the_48_suite_draws_are_pinned():
    """Whatever is refactored later, draw(seed) returns what it returned when the battery was written, field for field,
    for every suite seed."""
    digest = hashlib.sha256(repr([F.draw(s) for s in range(48)]).encode()).hexdigest()
    assert digest == "b27999446b10efe543855bdc06d4242c6c8e4424d0e624c39ea0bc1b3a9bc2cd"
    assert F.N_SUITE == 48 and F.FAMILIES == ("plain", "dropout", "bias", "edge", "etype", "weights")


def single_fused(case):
    """the case alone decides its forms, and every pass is a fused or fast one"""
    forms = F.expected_forms(case)
    return len(forms) == 1 and forms[0].fused


def coverage_failures(cases):
    """the coverage conditions over the suite's seeds that do NOT hold -> list of strings"""
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)

    def families(f):
        return len({c.family for c in cases if f(c)})
    for fam in F.FAMILIES:
        cs = [c for c in cases if c.family == fam]
        count = lambda f: sum(1 for c in cs if f(c))
        need(len(cs) == 8 and count(lambda c: c.large) == 2, "%s: 8 seeds, 2 of them large" % fam)
        need(count(lambda c: c.dtype == "float64") >= 1, "%s: an fp64 seed" % fam)
        need(count(lambda c: c.shuffled) >= 1, "%s: a shuffled seed" % fam)
        need(count(lambda c: not F.in_set(c)) >= 1, "%s: a seed that is generic by shape" % fam)
        need(count(lambda c: not c.large and c.n_dst < c.n_src) >= 1, "%s: n_dst < n_src" % fam)
        need(count(lambda c: not c.large and c.n_dst > c.n_src) >= 1, "%s: n_dst > n_src" % fam)
        need(count(lambda c: c.hub == 1500) >= 1, "%s: a seed with hub == 1500" % fam)
        need(count(lambda c: c.chunk_size == 1) >= 1, "%s: chunk_size == 1" % fam)
        need(count(lambda c: c.chunk_size >= 32) >= 1, "%s: chunk_size >= 32" % fam)
        need(count(single_fused) >= 3, "%s: 3 seeds whose single admissible pair is fully fused or fast" % fam)
    need(families(lambda c: c.family != "plain" and c.p == 0.0) >= 3, "p = 0 in 3 families")
    need(families(lambda c: c.p == 0.9) >= 3, "p = 0.9 in 3 families")
    need(families(lambda c: c.philox_seed >= 2 ** 32) >= 3, "a Philox seed >= 2^32 in 3 families")
    need(families(lambda c: c.p > 0 and c.offset == 2 ** 32 - 1) >= 3, "offset = 2^32 - 1 in 3 families")
    for numbering in F.NUMBERINGS:
        need(families(lambda c: c.family not in ("plain", "dropout") and c.numbering == numbering) >= 2,
             "numbering %s in 2 families" % numbering)
    for entry in F.ENTRIES:
        need(families(lambda c: c.entry == entry) >= 4, "entry %s in 4 families" % entry)
    for route in F.ROUTES:
        need(families(lambda c: c.route == route) >= 4, "route %s in 4 families" % route)
    need(families(lambda c: c.op in ("bias", "edge", "etype") and not c.need_dx) >= 2, "need_d* = False in 2 families")
    for fam in ("edge", "etype", "weights"):
        need(any(c.family == fam and c.misaligned >= 0 for c in cases), "%s: a misaligned operand" % fam)
    et = [c for c in cases if c.family == "etype"]
    need(any(c.n_types == T.max_types(c.h, c.d) for c in et), "n_types == max_types")
    need(any(c.n_types == T.max_types(c.h, c.d) + 1 for c in et), "n_types == max_types + 1")
    ws = [c for c in cases if c.family == "weights"]
    need({c.mode for c in ws} == set(F.MODES), "all three weights modes")
    need(any(not c.ga for c in ws) and any(c.ga for c in ws), "weights seeds with and without ga")
    need(any(not c.dO for c in ws), "a weights seed without dO")
    # the routes meet calls that could fuse, so that what they set decides something
    fusable = lambda c: c.dtype == "float32" and not c.shuffled and F.in_set(c) and c.misaligned < 0
    for fam in ("plain", "dropout", "bias"):
        cs = [c for c in cases if c.family == fam and fusable(c)]
        need(any(c.h == 1 for c in cs) and any(c.h > 1 for c in cs), "%s: a fusable one-head and a several-head seed" % fam)
        need(any(c.route == "default" for c in cs), "%s: a fusable seed on the default route" % fam)
        need(any(c.route == "windows" and c.h == 1 for c in cs), "%s: a fusable one-head seed on the windows route" % fam)
    need(any(c.route == "composed" and fusable(c) and c.op in ("plain", "bias") for c in cases),
         "a fusable seed of the plain or bias op on the composed route")
    need(any(c.route == "generic" and fusable(c) and c.op in ("plain", "bias") for c in cases),
         "a fusable seed of the plain or bias op on the generic route")
    need(any(c.route == "windows" and c.h > 1 and fusable(c) and c.op in ("plain", "bias") for c in cases),
         "a fusable several-head seed of the plain or bias op on the windows route")
    windows = [c for c in cases if c.route == "windows" and c.h == 1 and fusable(c) and c.op in ("plain", "bias")]
    need(sum(any(f.bwd == "Windows" for f in F.expected_forms(c, F.build(c, N_CU))) for c in windows) >= 2,
         "two seeds whose graph and knobs admit the window-owner backward")
    for fam in ("edge", "etype", "weights"):          # alignment alone decides there
        need(any(c.family == fam and c.misaligned >= 0 and c.dtype == "float32" and not c.shuffled and F.in_set(c)
                 and c.route != "generic" for c in cases), "%s: a misaligned operand in an otherwise fast seed" % fam)
    need(all(c.dO for c in cases if c.large), "every large seed runs its backward")
    return bad


def test_coverage_of_the_suite_seeds():
    assert coverage_failures([F.draw(s) for s in SEEDS]) == []


def test_fp32_references_use_at_most_half_of_every_bound():
    """Every seed's formula in plain torch fp32 on the CPU (the references in their dtype=torch.float32 mode) against the
    float64 reference: at most MARGIN = 0.5 of every bound, so a correct fp32 kernel that sums in another order has the
    other half.  The fp32 evaluation runs on one thread, so that the figures repeat.  fp64 cases are measured on their
    inputs rounded to fp32, against the fp32 bounds."""
    worst = {fam: {} for fam in F.FAMILIES}
    for seed in SEEDS:
        case, built, want = F.case_data(seed, N_CU)
        if case.dtype == "float64":
            case = dataclasses.replace(case, dtype="float32")
            built = dataclasses.replace(built, t={k: (v.float() if v.is_floating_point() else v) for k, v in built.t.items()})
            want = F.reference(case, built)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            got = F.reference(case, built, dtype=torch.float32)
        finally:
            torch.set_num_threads(threads)
        used = F.ratios(dataclasses.replace(case, entry="ctypes", need_dx=case.op != "plain"), got, want, built)
        for name, r in used.items():
            assert got[name].dtype == torch.float32
            worst[case.family][name] = max(worst[case.family].get(name, 0.0), r)
            assert r <= MARGIN, "seed %d %s: fp32 torch uses %.3f of the bound\n%s" % (seed, name, r, case)
    for fam in F.FAMILIES:
        print("    %-9s" % fam + "  ".join("%s %.2f" % (n, r) for n, r in worst[fam].items()))


def _case(**kw):
    base = dict(dtype="float32", large=False, shuffled=False, numbering="row_identity", p=0.0, philox_seed=0, offset=0,
                head0=0, need_dx=False, n_types=0, mode="", ga=False, dO=True, route="fused", misaligned=-1, entry="ctypes",
                sddmm_cpg=0)
    base.update(kw)
    if base["family"] in ("bias", "edge", "etype") or base["mode"] in ("bias", "edge"):
        base.setdefault("need_dx", True)
    return dataclasses.replace(F.draw(0), **base)


def _tags(case, built=None):
    forms = F.expected_forms(case, built)
    assert len(forms) == 1, forms
    return dict(forms[0].tags)


def test_expected_forms_against_the_tables_of_the_op_modules():
    import test_attention_bias as TB
    import test_attention_edge as TE
    import test_attention_etype as TT
    import test_attention_heads as TH
    import test_attention_launches as TL
    import test_attention_weights as TW
    half = dict(p=0.5, philox_seed=TL.HALF[1], offset=TL.HALF[2])
    # 1. the seven launch tables of test_attention_launches.py (route "fused": its knobs), but for the zero fills
    g = TL._graph()
    built = F.Built(g, g.csr_args(), g.src, g.dst, {}, 0)
    for name, (op, h, d, drop, need_dx, table) in TL.CASES.items():
        family = {"plain": "dropout" if drop[0] > 0 else "plain", "bias": "bias", "edge": "edge"}[op]
        case = _case(family=family, h=h, d=d, need_dx=need_dx and op != "plain", **(half if drop[0] > 0 else {}))
        want = {t: k for t, (k, calls) in table.items() if t != "zero_fill"}
        got = [dict(f.tags) for f in F.expected_forms(case, built)]
        assert want in got, (name, got)
        if name in ("plain", "dropout"):          # whether plan_get_walk takes the layout is not mirrored
            assert sorted((f.fwd, f.bwd) for f in F.expected_forms(case, built)) == [("composed", "Rows"), ("walk", "Rows")]
        else:
            assert got == [want], (name, got)
    assert F.knobs(_case(family="plain", h=1, d=64)) == F.FUSED_KNOBS
    # 2. the several-head tag sets of test_attention_heads.py, sorted and shuffled, and its default-knob case
    heads = _tags(_case(family="bias", h=4, d=16, need_dx=True, **half))
    assert TH.NEW <= set(heads) and not (TH.COMPOSED & set(heads))
    shuffled = _tags(_case(family="bias", h=4, d=16, need_dx=True, shuffled=True, **half))
    assert TH.BWD <= set(shuffled) and "attn_heads_fwd_rows" not in shuffled and "attn_bias_add" in shuffled
    g = TH._graph()
    built = F.Built(g, g.csr_args(), g.src, g.dst, {}, 0)
    for h, d in ((4, 16), (8, 32)):          # test_knobs: the cost rule fails on that graph
        assert [(f.fwd, f.bwd) for f in F.expected_forms(_case(family="bias", h=h, d=d, route="default"), built)] == \
            [("composed", "Composed")]
    # 3. the one-head bias passes of test_attention_bias.py
    one = _tags(_case(family="bias", h=1, d=256, need_dx=True))
    assert TB.FAST_BWD <= set(one) and "attn_bias_fwd_rows" in one and not ({"attn_rows_row", "attn_bwd_row", "attn_fwd"} & set(one))
    assert not (TB.FAST & set(_tags(_case(family="bias", h=1, d=16, route="composed"))))
    assert not (TB.FAST & set(_tags(_case(family="bias", h=5, d=12))))
    # 4. the fast and generic tag sets of the edge, etype and weights modules
    for family, M in (("edge", TE), ("etype", TT)):
        extra = dict(n_types=5) if family == "etype" else {}
        fast = set(_tags(_case(family=family, h=4, d=16, need_dx=True, route="default", **extra)))
        assert M.FAST <= fast and not M._generic(fast)
        shuffled = set(_tags(_case(family=family, h=4, d=16, need_dx=True, shuffled=True, **extra)))
        assert M.FAST_BWD <= shuffled and M._generic(shuffled) == M.GENERIC_FWD
        for kw in (dict(dtype="float64"), dict(h=3, d=5), dict(h=1, d=16), dict(route="generic"), dict(misaligned=4)):
            generic = set(_tags(_case(**dict(dict(family=family, h=4, d=16, need_dx=True, **extra), **kw))))
            assert not (M.FAST & generic) and M.GENERIC_FWD | M.GENERIC_BWD | {"attn_%s_generic_pack" % family} <= generic, kw
    mt = T.max_types(4, 16)
    over = set(_tags(_case(family="etype", h=4, d=16, need_dx=True, n_types=mt + 1)))
    assert {"attn_etype_generic_bwd_row", "attn_etype_rows_col", "attn_etype_pack", "attn_etype_fwd_rows"} <= over
    assert "attn_etype_dr_reduce" not in over and "attn_etype_rows_row" not in over
    assert "attn_etype_dr_reduce" in _tags(_case(family="etype", h=4, d=16, need_dx=True, n_types=mt))
    assert "attn_etype_rows_row" in _tags(_case(family="etype", h=4, d=16, need_dx=False, n_types=mt + 1))
    for mode in F.MODES:
        w = set(_tags(_case(family="weights", mode=mode, h=4, d=16))) & TW.TAGS
        assert w == ({"attn_weights_norm"} if mode != "edge" else {"attn_weights_xe"})
    for kw in (dict(dtype="float64"), dict(h=3, d=5), dict(route="generic"), dict(misaligned=5), dict(misaligned=0)):
        assert set(_tags(_case(**dict(dict(family="weights", mode="edge", h=4, d=16), **kw)))) & TW.TAGS == {"attn_weights_xe_generic"}
    assert set(_tags(_case(family="weights", mode="edge", h=4, d=16, misaligned=2))) & TW.TAGS == {"attn_weights_xe"}   # (V)


def test_head_multipliers_of_a_far_head_are_those_of_the_full_statement():
    """attention_dropout_reference.head_multipliers leaves out the Philox blocks below a large head0; where both are
    affordable it is dropout_reference.keep over all the heads."""
    import numpy as np
    import attention_dropout_reference as A
    import dropout_reference as DR
    rng = np.random.RandomState(0)
    src, dst = rng.randint(0, 50, 400), rng.randint(0, 60, 400)
    for g0, hg in ((61, 8), (66, 4), (127, 2), (1003, 1)):
        got = A.head_multipliers(src, dst, g0, hg, 0.5, 2 ** 40 + 7, 3)
        assert torch.equal(got > 0, torch.from_numpy(DR.keep(src, dst, g0 + hg, 0.5, 2 ** 40 + 7, 3)[:, g0:g0 + hg]))


def test_chunks_per_group_is_the_rule_of_the_gat_family():
    """host.h has ONE chunks_per_group; at eight rounds it is test_gat_launch_geometry._cpg"""
    from test_gat_launch_geometry import _cpg
    for n_chunks in (1, 4095, 65536, 81921, 200000, 10 ** 7):
        for lanes, cap in ((16, 16), (16, 3), (64, 16), (8, 16)):
            assert F.chunks_per_group(n_chunks, lanes, cap, 8, 256) == _cpg(n_chunks, 256, lanes, cap)
            assert F.chunks_per_group(2 * n_chunks, lanes, 10 ** 9, 4, 304) == max(1, 2 * n_chunks // (304 * (256 // lanes) * 4))
