"""The guard of tests/guarded.py on CPU tensors: the harness must itself be able to fail.  Then a census of the allocations
in custom_op_benchmark_amd/graphop.py -- one that the stand-in does not replace would escape the guard -- and the coverage
conditions of the GPU tier's cases (tests/test_guarded.py), computed from their draws."""
import collections
import os
import re

import pytest
import torch

import guarded as G
from custom_op_benchmark_amd import graphop

GRAPHOP_PY = os.path.join(os.path.dirname(os.path.abspath(graphop.__file__)), "graphop.py")


# ---- the stand-in ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8, torch.int32])
@pytest.mark.parametrize("shape", [(7,), (5, 3), (4, 3, 2), (0,), ()])
def test_views_have_the_asked_shape_dtype_strides_and_offset(shape, dtype):
    g = G.GuardedTorch()
    like = torch.ones(shape, dtype=dtype)
    views = [g.empty(shape, dtype=dtype, device="cpu"), g.zeros(shape, dtype=dtype, device="cpu"),
             g.empty_like(like), g.zeros_like(like)] + ([g.empty(*shape, dtype=dtype)] if shape else [])
    for v, (buf, nbytes, view, kind) in zip(views, g.records):
        want = torch.empty(shape, dtype=dtype)
        assert isinstance(v, torch.Tensor) and isinstance(v, g.Tensor) and v is view
        assert v.shape == want.shape and v.dtype == dtype and v.stride() == want.stride() and v.is_contiguous()
        assert nbytes == want.numel() * want.element_size() and buf.dtype == torch.uint8
        assert buf.numel() == nbytes + 2 * G.GUARD and G.GUARD % 512 == 0
        assert v.storage_offset() * v.element_size() == G.GUARD
        assert not v.numel() or v.data_ptr() - buf.data_ptr() == G.GUARD          # (an empty tensor's data_ptr is 0)
        assert bool((buf[:G.GUARD] == G.POISON).all()) and bool((buf[G.GUARD + nbytes:] == G.POISON).all())
        if kind.startswith("zeros"):
            assert not v.any()
        elif dtype.is_floating_point:
            assert bool(torch.isnan(v).all())
        else:
            assert bool((buf == G.POISON).all())
    assert [r[3] for r in g.records][:4] == ["empty", "zeros", "empty_like", "zeros_like"]
    assert g.violations(views) == [] or dtype.is_floating_point          # (an untouched float empty* view IS a violation)
    assert g.float32 is torch.float32 and g.library is torch.library


def test_the_stand_in_serves_graphops_own_helper():
    with G.guarded_ops() as g:
        one, many = graphop._edge_out(9, 1, torch.float32, "cpu"), graphop._edge_out(9, 3, torch.float64, "cpu")
    assert one.shape == (9,) and many.shape == (9, 3) and many.dtype == torch.float64 and len(g.records) == 2
    assert graphop.torch is torch


@pytest.mark.parametrize("side,byte,offset", [("before", G.GUARD - 1, -1), ("after", None, 0), ("before", 0, -G.GUARD),
                                              ("after", -1, G.GUARD - 1)])
def test_a_write_into_a_band_is_reported_with_its_place(side, byte, offset):
    """the last band byte before a view, the first after it, and the outermost byte of either band"""
    g = G.GuardedTorch()
    g.empty((3,), dtype=torch.int32, device="cpu")
    v = g.zeros((5, 3), dtype=torch.float32, device="cpu")
    buf, nbytes = g.records[1][:2]
    assert g.violations([v]) == []
    buf[G.GUARD + nbytes if byte is None else byte] = 0
    bad = g.violations([v])
    assert len(bad) == 1, bad
    assert "allocation 1 " in bad[0] and "(5, 3)" in bad[0] and "band %s it" % side in bad[0], bad
    assert "1 byte(s)" in bad[0] and "first at byte offset %d," % offset in bad[0], bad


def test_an_untouched_element_of_an_empty_float_view_is_reported():
    g = G.GuardedTorch()
    out, ws, z = g.empty((4, 3), dtype=torch.float32), g.empty(6, dtype=torch.float64), g.zeros(4, dtype=torch.float32)
    out.fill_(1.0)
    out[2, 1] = float("nan")
    assert g.violations([z]) == []                           # not returned: a workspace, exempt from the NaN rule
    bad = g.violations({"o": out.detach().reshape(-1), "z": z})          # matched by storage
    assert len(bad) == 1 and "allocation 0 " in bad[0] and "1 element(s)" in bad[0] and "flat index 7" in bad[0], bad
    assert len(g.violations([out, ws])) == 2                 # a returned workspace would be held to it too
    assert g.guarded_bytes() == 48 + 48 + 16


def test_one_flipped_bit_in_an_input_is_reported():
    a, b, i = torch.randn(5, 3), torch.randn(7, dtype=torch.float64), torch.arange(6)
    a[0, 0] = float("nan")
    snap = G.snapshot([a, {"b": b}, (i,)])
    assert G.unchanged(snap) == []
    b.view(torch.int64)[3] ^= 1 << 17
    bad = G.unchanged(snap)
    assert len(bad) == 1 and "input 1 " in bad[0] and "1 byte(s) changed" in bad[0] and "offset %d" % (3 * 8 + 2) in bad[0], bad
    b.view(torch.int64)[3] ^= 1 << 17
    a.view(torch.int32)[0, 0] ^= 1                            # another NaN: equal as a float comparison sees it, not as bits
    assert len(G.unchanged(snap)) == 1
    banded = G.banded(b)
    pad = G.GUARD // 8
    assert torch.equal(banded, b) and banded.is_contiguous() and banded.storage_offset() == pad
    whole = torch.empty(0, dtype=b.dtype).set_(banded.untyped_storage())
    assert whole.numel() == b.numel() + 2 * pad and bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[-pad:]).all())
    assert G.banded(i) is i


def test_graphops_torch_is_the_real_module_again_after_a_body_that_raises():
    with pytest.raises(ZeroDivisionError):
        with G.guarded_ops() as g:
            assert graphop.torch is g
            1 / 0
    assert graphop.torch is torch


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_every_allocation_of_the_binding_is_one_the_stand_in_replaces():
    """graphop.py names torch only for the four spellings the stand-in replaces, for types and for the registration; it makes
    no tensor through a method of another tensor except the contiguous copy of an output gradient (an input).  A binding
    added later that allocates another way fails here instead of escaping the guard."""
    src = open(GRAPHOP_PY).read()
    used = collections.Counter(re.findall(r"\btorch\.([A-Za-z_]\w*)", src))
    other = {"Tensor", "float32", "float64", "int32", "int64", "uint8", "library", "ops"}
    assert set(used) <= set(G.SPELLINGS) | other, sorted(set(used) - set(G.SPELLINGS) - other)
    assert all(used[s] for s in G.SPELLINGS), used
    assert re.findall(r"^\s*(?:from\s+torch\b.*|import\s+torch\.\S+.*|import\s+torch\s+as.*)$", src, re.M) == []
    for banned in ("new_empty", "new_zeros", "new_full", "new_ones", "new_tensor", "torch.full", "torch.ones", "torch.tensor",
                   "torch.as_tensor", "torch.arange"):
        assert banned not in src, banned
    makers = re.findall(r"(\w+)\s*=\s*(\w+)\.(clone|contiguous|to|float|double|repeat|expand|reshape|view|cpu|cuda)\(", src)
    assert makers and all(a == b and a in ("dy", "dO") and m == "contiguous" for a, b, m in makers), makers
    assert not re.findall(r"ptr\([^()]*\.(?:clone|contiguous|to|new_\w+)\(", src)


# ---- the GPU tier's cases --------------------------------------------------------------------------------------------------------
def test_the_guarded_cases_cover_odd_sized_edge_outputs_and_fp64():
    """For every edge-sized fp32 output name at least one guarded case returns it with a byte size that is no multiple of
    16 (a 16-byte tail store would then cross its end), and every family that has fp64 kernels has an fp64 case."""
    import attention_fuzz as AF
    import gat_fuzz as GF
    sizes, fp64 = G.edge_outputs()
    odd = collections.defaultdict(list)
    for name, case, dtype, nbytes in sizes:
        if dtype == "float32" and nbytes % 16:
            odd[name].append(case)
    for name in G.EDGE_OUTPUTS:
        assert odd[name], "no guarded case returns %s with a byte size off a multiple of 16" % name
    assert (G.outside_graph().n_edges * 15 * 4) % 16 and "attention_edge 3 x 5" in odd["dxe"]
    families = {f for f, _ in fp64}
    assert families >= set(GF.FAMILIES) | set(AF.FAMILIES) | {"fused_gat_edge", "core"}, families
