"""GPU tier of the bfloat16 attention battery (tests/attention_bf16_fuzz.py).  Every expected value is the float64 reference
of attention_bf16_reference.py; the bounds are BF_TOL and the fp32 TOL, neither widened.  Every used fraction of a bound
is printed."""
import dataclasses

import pytest
import torch

import attention_bf16_fuzz as F
from custom_op_benchmark_amd import _lib
from test_gat_launch_geometry import _profiled

pytestmark = pytest.mark.gpu


def attn_tags(profile):
    """{tag: kernel} of every attn_* launch of a profile"""
    return {t: k for t, k in profile.items() if t.startswith("attn_")}


def check(case, got, fwd, built, what):
    """dtypes and shapes, the rows without edges, every output inside its bound, and what the `equal` recipe makes exact
    -> the used fractions"""
    g = built.g
    live = F.live_rows(built)
    for name in F.OUTPUTS:
        want_shape = (g.n_src if name in ("o", "dQ") else g.n_dst, case.h, case.d)
        assert got[name].dtype == F.BF and tuple(got[name].shape) == want_shape, (what, name, got[name].dtype, got[name].shape)
    o = got["o"].detach().cpu()
    assert not o[~live].any(), what
    st = None
    if "stats" in got:
        assert got["stats"].dtype == torch.float32 and got["stats"].numel() == g.n_src * case.h * 2, what
        st = got["stats"].cpu().reshape(g.n_src, case.h, 2)
        assert not st[~live][..., 1].any(), what
    bwd = F.reference_backward(case, built, got["o"])
    used = F.ratios(case, got, fwd, built, bwd)
    print("%s: %s" % (what, "  ".join("%s %.3f" % (n, r) for n, r in used.items())))
    for name, r in used.items():
        assert r <= 1.0, "%s %s: %.3f of the bound" % (what, name, r)
    if case.recipe == "equal":
        zero = bwd["dQ"] == 0
        assert zero[~live].all() and not got["dQ"].cpu()[zero].any(), what
        if st is not None:
            deg = torch.bincount(g.src, minlength=g.n_src)
            pow2 = live & ((deg & (deg - 1)) == 0)
            assert not st[..., 0].any(), what
            assert torch.equal(st[pow2][..., 1], (1.0 / deg[pow2].float())[:, None].expand(-1, case.h)), what
    return used


@pytest.mark.parametrize("seed", range(F.N_SUITE))
def test_attention_bf16_fuzz(dev, seed):
    """One drawn case: pair, graph (n_k below and above n_q, empty rows, a hub row, chunks of 1 to 64 slots, the large
    stratum at 2 or 3 chunks per lane group), input recipe, entry and the output gradient's view.  The launches are the
    bf16 form's and no other attention kernel's; the results are the reference's; a second run, and the other bindings,
    agree bit for bit."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    case, built, fwd = F.case_data(seed, n_cu)
    what = "seed %d %s" % (seed, case)
    on_dev = F.on_device(built, dev)
    try:
        _lib.clear_plan_cache()
        if case.large:
            F.assert_cpg(case, built, n_cu)
        got, profile = _profiled(lambda: F.run(case, on_dev, dev))
        assert attn_tags(profile) == dict(F.KERNELS, **F.SETUP), "%s\nlaunched %s" % (what, attn_tags(profile))
        check(case, got, fwd, built, what)
        again = F.run(case, on_dev, dev)
        assert set(again) == set(got)
        for name in got:
            assert torch.equal(got[name], again[name]), "%s: %s differs between two runs" % (what, name)
        # the two raw bindings agree bit for bit (one of them is `got` where the case drew a raw entry), and the autograd
        # class returns what they return
        raw = {e: (got if e == case.entry else F.run(dataclasses.replace(case, entry=e, grad_view="contiguous"), on_dev, dev))
               for e in ("ctypes", "torch_ops")}
        for name in F.OUTPUTS + ("stats",):
            assert torch.equal(raw["ctypes"][name], raw["torch_ops"][name]), "%s: %s differs between the bindings" % (what, name)
        if not case.raw:
            check(dataclasses.replace(case, entry="ctypes"), raw["ctypes"], fwd, built, what + " (raw)")
            for name in F.OUTPUTS:
                assert torch.equal(raw["ctypes"][name], got[name]), "%s: %s differs behind autograd" % (what, name)
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()
