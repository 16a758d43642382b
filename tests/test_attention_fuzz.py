"""GPU tier of the dot-product attention family's randomised battery (tests/attention_fuzz.py), and the family's raw ops on
a side stream without a host synchronisation, which the family's own modules do not run.

Every expected value is the float64 reference of attention_fuzz.reference; the bounds are those of the ops' own modules
(attention_fuzz.bound), none widened.  Every used fraction of a bound is printed."""
import dataclasses

import pytest
import torch

import attention_edge_reference as E
import attention_fuzz as F
from custom_op_benchmark_amd import _lib, graphop as ops
from test_gat_launch_geometry import _profiled
from util import random_graph

pytestmark = pytest.mark.gpu


def _check(case, got, want, built, what):
    """shapes and dtypes, then every output inside attention_fuzz.bound(case, name) of the float64 reference"""
    for name in F.outputs(case):
        x, y = got[name], want[name]
        assert x.dtype == case.torch_dtype and x.shape == y.reshape(x.shape).shape, (what, name, x.dtype, x.shape, y.shape)
    used = F.ratios(case, got, want, built)
    assert set(used) == set(F.outputs(case)), (what, used)
    print("%s: %s" % (what, "  ".join("%s %.3f" % (n, r) for n, r in used.items())))
    for name, r in used.items():
        assert r <= 1.0, "%s %s: %.3f of the bound" % (what, name, r)
    return used


# ---- 1. the battery ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(F.N_SUITE))
def test_attention_family_fuzz(dev, seed):
    """One drawn case: family, shape, dtype, graph (n_k below and above n_q, empty rows, a hub row, chunks of 1 to 64 slots,
    shuffled chunk lists, the large stratum at 2 or 3 chunks per lane group), edge numbering, dropout triple and head0,
    need_d*, the type table's size, the weights' mode and gradients, the route's knobs, a misaligned operand, binding or
    autograd entry with a non-contiguous output gradient.  The launches form one admissible pair, then the results are
    the reference's."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    case, built, want = F.case_data(seed, n_cu)
    what = "seed %d %s" % (seed, case)
    try:
        F.set_knobs(case)
        _lib.clear_plan_cache()
        got, profile = _profiled(lambda: F.run(case, built, dev))
        raw = case
        if not F.forms_checked(case):
            # FusedAttention / -Dropout / -Bias may run head groups or keep `a` for an unfused backward: the forms are those
            # of ONE raw call of the same op on the same operands, made here for its launch profile alone
            raw = dataclasses.replace(case, entry="ctypes", grad_view="contiguous")
            _, profile = _profiled(lambda: F.run(raw, built, dev))
        seen, forms = F.seen_forms(profile), F.expected_forms(raw, built)
        print("seed %d %s %s admits %s" % (seed, case.family, case.route, [(f.fwd, f.bwd) for f in forms]))
        match = [f for f in forms if f.tags == seen]
        assert len(match) == 1, "%s\nlaunched %s\nadmissible %s" % (what, seen, [f.tags for f in forms])
        print("seed %d ran %s / %s" % (seed, match[0].fwd, match[0].bwd))
        if case.family in ("plain", "dropout"):
            a8 = tuple(t.to(dev) for t in built.csr)
            fused = ops.attention_backward_is_fused(*a8, built.t["Q"].to(dev), built.t["K"].to(dev))
            assert fused == (match[0].bwd != "Composed"), (what, fused, match[0].bwd)
        if case.large:
            F.assert_cpg(case, built, n_cu)
        empty = torch.bincount(built.src, minlength=built.g.n_src) == 0
        assert got["o"].shape[0] == built.g.n_src and not got["o"].detach().cpu()[empty].any(), what
        gname = {"bias": "db", "edge": "dxe", "etype": "dR"}.get(case.op)
        if gname and not case.need_dx and case.dO:
            x = got[gname]
            assert x is None if not case.raw else (x.numel() == 0 and x.dtype == case.torch_dtype), (what, gname)
        if "stats" in got:
            assert got["stats"].shape == (built.g.n_src, case.h, 2) and got["stats"].dtype == case.torch_dtype, what
        _check(case, got, want, built, what)
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()


# ---- 2. a side stream, no host synchronisation between the ops --------------------------------------------------------------
@pytest.mark.parametrize("family", F.FAMILIES)
def test_raw_ops_on_a_side_stream(dev, family):
    """The family's raw forward (the weights pass) and backward on a non-default stream, nothing synchronising between
    them: an op that launched a kernel or a fill on another stream would read inputs that are not written yet, or race
    its own zero fill.  Index arrays and inputs are on the device before (the plans are built by a first call), so the
    calls copy and allocate nothing that would wait for the device.  Compared with the same calls on the default stream
    at twice the bound (two fp32 results, which differ in the order of their atomic adds), and the side-stream result
    with the float64 reference at the bound."""
    g0 = random_graph(900, 700, 9000, seed=4, chunk_size=32, zero_rows=0.1, hub=1100)
    case = dataclasses.replace(
        F.draw(0), family=family, h=4, d=16, dtype="float32", large=False, shuffled=False, numbering="row_identity",
        p=0.0 if family == "plain" else 0.5, philox_seed=0 if family == "plain" else 2 ** 40 + 3,
        offset=0 if family == "plain" else 7, head0=0, need_dx=family in ("bias", "edge", "etype", "weights"),
        n_types=5 if family == "etype" else 0, mode="bias" if family == "weights" else "", ga=False, dO=True,
        route="fused", misaligned=-1, entry="ctypes", grad_view="contiguous", sddmm_cpg=0, input_seed=11)
    built = F.Built(g0, g0.csr_args(), g0.src, g0.dst, *F.make_inputs(case, g0, g0.src))
    want = F.reference(case, built)
    on_dev = dataclasses.replace(built, csr=tuple(x.to(dev) for x in built.csr), t={k: v.to(dev) for k, v in built.t.items()})
    try:
        F.set_knobs(case)
        _lib.clear_plan_cache()
        F.run(case, on_dev, dev)                   # (building the plans synchronises: done before the side stream starts)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = F.run(case, on_dev, dev)
        side.synchronize()
        ref = F.run(case, on_dev, dev)
        torch.cuda.synchronize()
        for name in F.outputs(case):
            assert bool(torch.isfinite(got[name]).all()), name
            tol = F.bound(case, name, built.n_max)
            r = E.error_ratio(got[name].cpu(), ref[name].cpu(), rtol=2 * tol["rtol"], atol=2 * tol["atol"])
            print("%s side stream vs default stream %s: %.3f of twice the bound" % (family, name, r))
            assert r <= 1.0, (family, name, r)
        _check(case, got, want, built, "%s on a side stream" % family)
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()
